"""CPU: the host side of agdiff_amd/rings.py and of the ring terms in agdiff_amd/torsions.py -- which cycles are rings, how they are
walked and ordered, where the symmetry mappings send them, the scales, the six-ring classes, the header's two new entries and the
switches.  Nothing here computes on a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import rings_ref as RR
import tfd_ref as TR
from agdiff_amd import _lib, rings, torsions

VP, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float


def _item(mol, **kw):
    at, bi, bt = mol
    return dict(atom_type=at, bond_index=bi, bond_type=bt, **kw)


MOLECULES = [("naphthalene", RR.naphthalene, [6, 6]), ("bicyclo[2.2.2]octane", RR.bicyclo222octane, [6, 6, 6]),
             ("norbornane", RR.norbornane, [5, 5, 6]), ("spiro[4.4]nonane", RR.spiro44nonane, [5, 5]),
             ("cubane", RR.cubane, [4] * 6 + [6] * 4)]


@pytest.mark.parametrize("name,build,sizes", MOLECULES, ids=[m[0] for m in MOLECULES])
def test_ring_sets_of_the_named_molecules(name, build, sizes):
    mol = build()
    found = rings.find_rings(*mol)
    assert [len(r) for r in found] == sizes
    assert found == RR.chordless_cycles(len(mol[0]), RR.heavy_bonds(mol))        # brute force over the atom subsets
    ptr, idx = rings.ring_table(_item(mol))
    assert ptr.dtype == np.int32 and idx.dtype == np.int32 and ptr.tolist() == np.cumsum([0] + sizes).tolist()
    assert rings.unpack_rings(ptr, idx) == found


def test_a_chord_excludes_the_perimeter_and_three_rings_are_left_out():
    assert all(len(r) == 6 for r in rings.find_rings(*RR.naphthalene()))          # not the 10-perimeter, which the 0 - 5 bond chords
    assert [len(r) for r in rings.find_rings(*RR.ring_graph(10))] == [10]         # the same perimeter without the chord is a ring
    assert rings.find_rings(*RR.ring_graph(3)) == []
    # bicyclo[1.1.0]butane: two fused three-rings; their 4-perimeter has the chord 0 - 2
    assert rings.find_rings(*TR.graph([6] * 4, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 0, 1), (0, 2, 1)])) == []
    # max_size bounds the search; 13 atoms are not found by default
    assert rings.find_rings(*RR.ring_graph(13)) == [] and len(rings.find_rings(*RR.ring_graph(13), max_size=13)) == 1
    assert rings.find_rings(*RR.ring_graph(8), max_size=7) == []
    # chains, hydrogens and 2- / 3-hop entries take no part
    assert rings.find_rings(*TR.butane_with_hydrogens_and_hops()) == []
    assert rings.find_rings(*RR.cyclohexane_with_hydrogens()) == [(0, 1, 2, 3, 4, 5)]
    assert rings.find_rings(*TR.toluene()) == [(0, 1, 2, 3, 4, 5)]


def test_the_walk_rule_and_the_order():
    # a six-ring numbered so that the lowest atom's neighbours are 4 and 2: walked 0 -> 2 (the lower neighbour) -> ...
    cyc = [0, 4, 1, 5, 3, 2]
    mol = TR.graph([6] * 6, [(cyc[i], cyc[(i + 1) % 6], 1) for i in range(6)])
    assert rings.find_rings(*mol) == [(0, 2, 3, 5, 1, 4)]
    # ordered by (size, atoms): spiro[4.4]nonane's rings share atom 0
    assert rings.find_rings(*RR.spiro44nonane()) == [(0, 1, 2, 3, 4), (0, 5, 6, 7, 8)]
    assert rings.find_rings(*RR.norbornane()) == [(0, 2, 3, 1, 6), (0, 4, 5, 1, 6), (0, 2, 3, 1, 5, 4)]


def test_a_callers_ring_of_33_atoms_is_refused():
    ptr, idx = rings.pack_rings([tuple(range(32)), (40, 41, 42, 43)])
    assert ptr.tolist() == [0, 32, 36] and idx.tolist() == list(range(32)) + [40, 41, 42, 43]
    with pytest.raises(_lib.AgdiffLimitError):
        rings.pack_rings([tuple(range(33))])
    with pytest.raises(_lib.AgdiffLimitError):
        rings.pack_rings([(0, 1, 2)])
    with pytest.raises(ValueError):
        rings.pack_rings([(0, 1, 2, 1)])
    with pytest.raises(_lib.AgdiffLimitError):
        torsions.torsion_table(_item(RR.ring_graph(40)), rings=[tuple(range(33))])
    # a macrocycle named by hand goes through
    table = torsions.torsion_table(_item(RR.ring_graph(20)), rings=[tuple(range(20))])
    assert table[4].tolist() == [0, 20] and table[1].shape[1] == 1


@pytest.mark.parametrize("build,P", [(TR.biphenyl, 8), (RR.bicyclo222octane, 12)], ids=["biphenyl", "bicyclo[2.2.2]octane"])
def test_every_automorphism_sends_rings_to_rings(build, P):
    from agdiff_amd.evaluation import selection_of
    item = _item(build())
    _, heavy, pa = selection_of(item)
    assert pa.shape[0] == P
    found = rings.find_rings(*build())
    sets = {frozenset(r) for r in found}
    for p in pa:
        assert {frozenset(int(heavy[p[a]]) for a in r) for r in found} == sets
    quads, tmap, scale, even, ring_ptr, ring_idx = torsions.torsion_table(item, rings=True)
    Q, T, Rg = quads.shape[0], tmap.shape[1] - len(found), len(found)
    plain_quads, plain_tmap = torsions.torsion_table(item)
    assert np.array_equal(quads, plain_quads) and T == plain_tmap.shape[1]
    assert tmap[0].tolist() == plain_tmap[0].tolist() + [Q + r for r in range(Rg)]
    assert all(sorted(row[T:]) == [Q + r for r in range(Rg)] for row in tmap.tolist())       # each mapping permutes the rings
    assert len({tuple(r) for r in tmap.tolist()}) == tmap.shape[0]
    assert scale.dtype == np.float32 and even.dtype == np.int32 and even.tolist() == [0] * T + [1] * Rg
    assert np.allclose(scale[:T], np.pi) and np.allclose(scale[T:], RR.ring_scale(6), rtol=1e-6)
    assert rings.unpack_rings(ring_ptr, ring_idx) == found
    if build is TR.biphenyl:                                                      # the swap of the two rings is among the mappings
        assert any(row[T:] == [Q + 1, Q] for row in tmap.tolist())
    else:                                                                         # all six orders of the three bridges' rings
        assert len({tuple(row[T:]) for row in tmap.tolist()}) == 6


def test_a_mapping_that_is_no_automorphism_is_refused_and_the_default_table_is_unchanged():
    item = _item(RR.spiro44nonane(), perms=np.array([[0, 1, 2, 3, 5, 4, 6, 7, 8]], dtype=np.int32))
    with pytest.raises(ValueError):
        torsions.torsion_table(item, rings=True)
    quads, tmap = torsions.torsion_table(_item(RR.ring_graph(6)))
    assert quads.shape == (0, 4) and tmap.shape == (1, 0)                          # T = 0, as before: nothing in a ring rotates
    table = torsions.torsion_table(_item(RR.ring_graph(6)), rings=True)
    assert table[0].shape == (0, 4) and table[1].tolist() == [[0]] and table[3].tolist() == [1]
    assert inspect.signature(torsions.torsion_table).parameters["rings"].default is False


def test_scales_are_the_published_ones():
    deg = np.degrees(rings.ring_scales(np.array([0, 4, 9, 15, 29])).astype(np.float64))
    assert np.abs(deg - [14.78, 23.76, 36.34, 180.0]).max() <= 0.01
    assert np.abs(deg - np.degrees([RR.ring_scale(N) for N in (4, 5, 6, 14)])).max() <= 1e-4


def test_six_ring_classes():
    ring = list(range(6))
    cases = [(RR.chair(), "chair"), (RR.chair(q3=-0.63), "chair"), (RR.boat(), "boat"), (RR.twist_boat(), "twist-boat"),
             (RR.construct(6, [0.45], [0.0], 0.45), "half-chair/envelope"), (RR.construct(6, [0.45], [np.pi / 6], -0.45), "half-chair/envelope"),
             (RR.construct(6, [0.7], [np.pi / 3], 0.0), "boat"), (RR.construct(6, [0.7], [np.pi / 2], 0.05), "twist-boat")]
    for pos, want in cases:
        _, row = RR.cremer_pople(pos[None], ring)
        code = rings.six_ring_class(row[:, 0], row[:, 1], row[:, 2])
        assert code.dtype == np.int8 and rings.CLASS_NAMES[int(code[0])] == want
    assert abs(rings.six_ring_theta(0.0, 0.63)) <= 1e-12 and abs(rings.six_ring_theta(0.0, -0.63) - 180.0) <= 1e-12
    assert abs(rings.six_ring_theta(0.7, 0.0) - 90.0) <= 1e-12 and abs(rings.six_ring_theta(0.45, 0.45) - 45.0) <= 1e-12
    assert rings.six_ring_class(np.nan, 0.0, 0.1).tolist() == 0
    # a table with a five-ring in front: classes for the six-ring only
    pk = np.zeros((2, 2 + 3), dtype=np.float32)
    pk[:, 2:] = [[0.0, 0.0, 0.63], [0.7, np.pi / 6, 0.0]]
    assert rings.ring_classes([0, 5, 11], pk).tolist() == [[0, 1], [0, 3]]
    assert rings.pucker_columns([0, 5, 11]).tolist() == [0, 2, 5]


def test_header_declares_the_two_entries():
    assert _lib.DEFINES["AGDIFF_RING_MAX_ATOMS"] == 32 and rings.MAX_ATOMS == 32
    assert _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    assert _lib.EXPORTS["agdiff_ring_coords"] == [VP, VP, VP, I32, I32, I32, VP, VP, VP, VP]
    assert _lib.EXPORTS["agdiff_tfd_matrix_terms"] == [VP, VP, VP, VP, VP, VP, I32, I32, I32, I32, I32, F32, VP, VP, VP, VP]
    lib = _lib.load()
    for name in ("agdiff_ring_coords", "agdiff_tfd_matrix_terms"):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == _lib.EXPORTS[name]


def test_switches_are_off_by_default_and_last():
    from agdiff_amd import clusters, evaluation
    for fn, name in ((clusters.cluster_conformers, "tfd_rings"), (evaluation.get_tfd_confusion_matrix, "rings"),
                     (evaluation.CovMatEvaluator.__init__, "tfd_rings"), (torsions.tfd_from_angles, "rings"), (torsions.tfd_matrix, "rings"),
                     (torsions._self_tfd, "rings"), (torsions.tfd_self, "rings"), (torsions.torsion_table, "rings")):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == name and last.default is False, fn.__name__
    assert clusters._parser().parse_args(["--samples", "s", "--testset", "t", "--tfd", "0.2", "--out", "o"]).tfd_rings is False
    assert clusters._parser().parse_args(["--samples", "s", "--testset", "t", "--tfd", "0.2", "--tfd-rings", "--out", "o"]).tfd_rings is True
    with pytest.raises(ValueError):
        evaluation.CovMatEvaluator(metric="rmsd", tfd_rings=True)
    with pytest.raises(ValueError):
        clusters.cluster_conformers(_item(RR.ring_graph(6), pos_gen=np.zeros((1, 6, 3), dtype=np.float32)), 0.2, tfd_rings=True)
