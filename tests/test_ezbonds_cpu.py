"""Host side of the E/Z fix (agdiff_amd/ezbonds.py) on hand-written graphs: which double bonds are stereogenic, their quads, the side
tables, the majority parity, the checks of an item's tags, the command line and the export.  No GPU."""
import ctypes

import numpy as np
import pytest

import ez_cases as EC
import ez_ref as ER
import planarity_ref as PR
from agdiff_amd import _lib, driver
from agdiff_amd import ezbonds as EZ


def _rows(ptr, idx):
    return [idx[ptr[k]:ptr[k + 1]].tolist() for k in range(len(ptr) - 1)]


def _found(mol):
    quads, in_ring = EZ.stereo_double_bonds(*mol)
    assert quads.dtype == np.int32 and quads.ndim == 2 and quads.shape[1] == 4 and in_ring.dtype == np.bool_
    return quads.tolist(), in_ring.tolist()


def _butene():
    """H0 and C1 (methyl) on C2, C2 = C3, C4 (methyl) and H5 on C3, methyl hydrogens 6 .. 8 on C1 and 9 .. 11 on C4"""
    bonds = [(2, 0, 1), (2, 1, 1), (2, 3, 2), (3, 4, 1), (3, 5, 1)] + [(1, k, 1) for k in (6, 7, 8)] + [(4, k, 1) for k in (9, 10, 11)]
    return PR.graph([1, 6, 6, 6, 6, 1] + [1] * 6, bonds)


def test_two_butene_is_found_with_the_lowest_index_neighbours_and_the_smaller_side():
    mol = _butene()
    assert _found(mol) == ([[0, 2, 3, 4]], [False])             # a = H0 < C1, d = C4 < H5
    quads = EZ.stereo_double_bonds(*mol)[0]
    ptr, idx = EZ.flip_sides(12, mol[1], mol[2], quads)
    assert ptr.dtype == idx.dtype == np.int32 and ptr.tolist() == [0, 6]
    assert idx.tolist() == [3, 4, 5, 9, 10, 11]                   # six atoms either side: the tie goes to j's
    # an ethyl in the methyl's place on j's side: i's side is the smaller one; on i's side: j's is
    longer_j = PR.graph([1, 6, 6, 6, 6, 1, 6], [(2, 0, 1), (2, 1, 1), (2, 3, 2), (3, 4, 1), (3, 5, 1), (4, 6, 1)])
    longer_i = PR.graph([1, 6, 6, 6, 6, 1, 6], [(2, 0, 1), (2, 1, 1), (2, 3, 2), (3, 4, 1), (3, 5, 1), (1, 6, 1)])
    for mol, want in ((longer_j, [0, 1, 2]), (longer_i, [3, 4, 5])):
        quads, _ = EZ.stereo_double_bonds(*mol)
        assert quads.tolist() == [[0, 2, 3, 4]]
        assert _rows(*EZ.flip_sides(7, mol[1], mol[2], quads)) == [want]


def test_what_is_not_stereogenic_is_not_found():
    propene = PR.graph([6, 6, 6] + [1] * 6, [(0, 1, 2), (1, 2, 1), (0, 3, 1), (0, 4, 1), (1, 5, 1), (2, 6, 1), (2, 7, 1), (2, 8, 1)])
    assert _found(propene) == ([], [])                           # =CH2: two equal substituents
    allene = PR.graph([6, 6, 6, 9, 1, 17, 1], [(0, 1, 2), (1, 2, 2), (0, 3, 1), (0, 4, 1), (2, 5, 1), (2, 6, 1)])
    assert _found(allene) == ([], [])                            # the middle carbon carries a second double bond
    enyne = PR.graph([6, 6, 6, 6, 9, 1], [(0, 1, 2), (1, 2, 1), (2, 3, 3), (0, 4, 1), (0, 5, 1)])
    assert _found(enyne)[0] == [[4, 0, 1, 2]]                    # a triple bond NEXT to an end does not matter ...
    ynene = PR.graph([6, 6, 6, 9], [(0, 1, 2), (1, 2, 3), (0, 3, 1)])
    assert _found(ynene) == ([], [])                             # ... one AT an end does
    bare = PR.graph([6, 6, 9], [(0, 1, 2), (0, 2, 1)])
    assert _found(bare) == ([], [])                              # an end without another neighbour
    three = PR.graph([6, 15, 9, 17, 35, 1], [(0, 1, 2), (1, 2, 1), (1, 3, 1), (1, 4, 1), (0, 5, 1)])
    assert _found(three) == ([], [])                             # an end with three other neighbours
    single = PR.graph([6, 6, 9, 17], [(0, 1, 1), (0, 2, 1), (1, 3, 1)])
    assert _found(single) == ([], [])


def test_an_oxime_with_one_substituent_on_the_nitrogen_is_found():
    # C0 (H3, CH3 = C2) = N1 - O4 - H5, methyl hydrogens 6 .. 8
    mol = PR.graph([6, 7, 6, 1, 8, 1, 1, 1, 1], [(0, 1, 2), (0, 2, 1), (0, 3, 1), (1, 4, 1), (4, 5, 1), (2, 6, 1), (2, 7, 1), (2, 8, 1)])
    assert _found(mol) == ([[2, 0, 1, 4]], [False])
    assert _rows(*EZ.flip_sides(9, mol[1], mol[2], [[2, 0, 1, 4]])) == [[1, 4, 5]]


def _ring(size, hydrogens=True):
    bonds = [(k, (k + 1) % size, 2 if k == 0 else 1) for k in range(size)]
    atoms = [6] * size
    if hydrogens:
        bonds += [(0, size, 1), (1, size + 1, 1)]
        atoms += [1, 1]
    return PR.graph(atoms, bonds)


def test_ring_double_bonds_small_rings_never_large_rings_judged_only():
    for size in (5, 6, 7):
        assert _found(_ring(size)) == ([], [])
    for size in (8, 9):
        mol = _ring(size)
        quads, in_ring = _found(mol)
        assert quads == [[size - 1, 0, 1, 2]] and in_ring == [True]
        ptr, idx = EZ.flip_sides(size + 2, mol[1], mol[2], quads)
        assert ptr.tolist() == [0, 0] and idx.shape == (0,)
    # a double bond in a ring of 6 AND a ring of 10 (a fused pair): the small ring decides
    fused = PR.graph([6] * 14, [(k, (k + 1) % 10, 2 if k == 0 else 1) for k in range(10)] + [(1, 10, 1), (10, 11, 1), (11, 12, 1), (12, 13, 1), (13, 0, 1)])
    assert _found(fused) == ([], [])


def test_a_styrene_like_bond_keeps_the_ring_in_one_side():
    # ring carbons 0 .. 5 (aromatic), C6 (H9) on C0, C6 = C7 (H10), C8 on C7
    bonds = [(k, (k + 1) % 6, 12) for k in range(6)] + [(0, 6, 1), (6, 7, 2), (7, 8, 1), (6, 9, 1), (7, 10, 1)]
    mol = PR.graph([6] * 9 + [1, 1], bonds)
    quads, in_ring = _found(mol)
    assert quads == [[0, 6, 7, 8]] and in_ring == [False]        # the aromatic bonds are not of type 2 and are never candidates
    assert _rows(*EZ.flip_sides(11, mol[1], mol[2], quads)) == [[7, 8, 10]]
    frozen = np.zeros(11, dtype=bool)
    frozen[8] = True
    assert _rows(*EZ.flip_sides(11, mol[1], mol[2], quads, frozen=frozen)) == [[0, 1, 2, 3, 4, 5, 6, 9]]


def test_a_conjugated_triene_gives_three_bonds_with_nested_or_disjoint_sides_that_split_no_quad():
    mol, _, _ = EC.molecule("c14")
    quads, in_ring = _found(mol)
    assert quads == [[0, 1, 2, 3], [2, 3, 4, 5], [4, 5, 6, 7]] and in_ring == [False] * 3
    rows = [set(r) for r in _rows(*EZ.flip_sides(14, mol[1], mol[2], quads))]
    assert rows == [{0, 1, 8}, {4, 5, 6, 7, 11, 12, 13}, {6, 7, 13}]
    for x in range(3):
        for y in range(3):
            if x != y:
                assert rows[x] <= rows[y] or rows[y] <= rows[x] or not (rows[x] & rows[y])
                assert len(rows[x] & set(quads[y])) in (0, 4)     # the other bond's four atoms turn together or not at all
    for name in EC.NAMES:                                          # and so in every molecule the GPU tests use
        q, _, ptr, idx = EC.tables(name)
        rr = [set(r) for r in _rows(ptr, idx)]
        for x in range(len(rr)):
            assert int(q[x, 2]) in rr[x] or int(q[x, 1]) in rr[x]
            for y in range(len(rr)):
                assert x == y or len(rr[x] & set(q[y].tolist())) in (0, 4)


def test_frozen_atoms_pick_the_other_side_or_none():
    mol = _butene()
    quads = [[0, 2, 3, 4]]
    mask = lambda *atoms: np.isin(np.arange(12), atoms)
    assert _rows(*EZ.flip_sides(12, mol[1], mol[2], quads, frozen=mask(11))) == [[0, 1, 2, 6, 7, 8]]
    assert _rows(*EZ.flip_sides(12, mol[1], mol[2], quads, frozen=mask(0))) == [[3, 4, 5, 9, 10, 11]]
    assert _rows(*EZ.flip_sides(12, mol[1], mol[2], quads, frozen=mask(2))) == [[3, 4, 5, 9, 10, 11]]    # an end atom counts
    assert _rows(*EZ.flip_sides(12, mol[1], mol[2], quads, frozen=mask(0, 11))) == [[]]
    assert _rows(*EZ.flip_sides(12, mol[1], mol[2], quads, frozen=mask())) == [[3, 4, 5, 9, 10, 11]]
    assert _rows(*EZ.flip_sides(12, mol[1], mol[2], quads, frozen=mask(0).astype(np.uint8))) == [[3, 4, 5, 9, 10, 11]]
    with pytest.raises(ValueError, match="frozen"):
        EZ.flip_sides(12, mol[1], mol[2], quads, frozen=np.zeros(5, dtype=bool))
    with pytest.raises(ValueError, match="outside"):
        EZ.flip_sides(12, mol[1], mol[2], [[0, 2, 3, 12]])
    with pytest.raises(ValueError, match="no bond"):
        EZ.flip_sides(12, mol[1], mol[2], [[0, 2, 4, 9]])


def _butene_conformers(kinds):
    """one conformer per entry: +1 trans, -1 cis, 0 collinear a - i - j (undecided)"""
    _, pos, _ = EC.molecule("c6")
    out = []
    for k in kinds:
        p = pos.copy()
        if k < 0:
            ER.rotate_side(p, 1, 2, [2, 3, 5])
        if k == 0:
            p[:3] = [[-1.0, -1.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 0.0]]      # (small integers: the normal is zero exactly)
        out.append(p)
    return np.stack(out)


def test_parities_from_conformers_majority_tie_and_undecided():
    quads = [[0, 1, 2, 3]]
    for kinds, want, minority in (([1, 1, -1], 1, 1), ([-1, -1, 1, -1], -1, 1), ([1, -1], 0, 1), ([1], 1, 0), ([0, 0], 0, 0), ([0, -1], -1, 0)):
        target, disagree = EZ.parities_from_conformers(_butene_conformers(kinds), quads)
        assert target.dtype == np.int8 and disagree.dtype == np.int32
        assert (target.tolist(), disagree.tolist()) == ([want], [minority]), kinds
    target, disagree = EZ.parities_from_conformers(_butene_conformers([1, -1]), np.zeros((0, 4), np.int32))
    assert target.shape == disagree.shape == (0,)
    # the same parity as the restatement's, conformer by conformer, on the GPU tests' inputs
    for name in ("c14", "centre"):
        quads, _, _, _ = EC.tables(name)
        pos = EC.conformers(name, 3)
        for g in range(3):
            assert EZ.parities_from_conformers(pos[g:g + 1], quads)[0].tolist() == ER.states(pos[g:g + 1], quads, np.ones(len(quads)))[0].tolist()


def test_ez_table_reads_the_tags_and_refuses_what_does_not_fit_the_molecule():
    mol = _butene()
    item = lambda quads, ez: dict(atom_type=mol[0], edge_index=mol[1], edge_type=mol[2], ez_quads=quads, ez=ez)
    quads, target = EZ.ez_table(item([[0, 2, 3, 4]], [1]))
    assert quads.dtype == np.int32 and quads.tolist() == [[0, 2, 3, 4]] and target.dtype == np.int8 and target.tolist() == [1]
    assert EZ.ez_table(item([[1, 2, 3, 5]], [-3]))[1].tolist() == [-1]          # any other neighbours; the sign is what counts
    quads, target = EZ.ez_table(item(np.zeros((0, 4), np.int32), np.zeros(0, np.int8)))
    assert quads.shape == (0, 4) and target.shape == (0,)
    with pytest.raises(ValueError, match="ez_quads"):
        EZ.ez_table(dict(atom_type=mol[0], edge_index=mol[1], edge_type=mol[2]))
    with pytest.raises(ValueError, match="ez_quads"):
        EZ.ez_table(dict(atom_type=mol[0], edge_index=mol[1], edge_type=mol[2], ez=[1]))
    for quads, ez, message in (([[0, 2, 3]], [1], r"\[D, 4\]"),
                               ([[0, 2, 3, 4]], [1, 1], "2 entries for 1 quads"),
                               ([[0, 2, 3, 12]], [1], r"outside \[0, 12\)"),
                               ([[-1, 2, 3, 4]], [1], r"outside \[0, 12\)"),
                               ([[2, 1, 6, 0]], [1], "no double bond"),
                               ([[6, 1, 2, 3]], [1], "no double bond"),
                               ([[4, 2, 3, 5]], [1], "atom 4 is no other bonded neighbour of atom 2"),
                               ([[3, 2, 3, 4]], [1], "atom 3 is no other bonded neighbour of atom 2"),
                               ([[0, 2, 3, 1]], [1], "atom 1 is no other bonded neighbour of atom 3"),
                               ([[0, 2, 3, 2]], [1], "atom 2 is no other bonded neighbour of atom 3")):
        with pytest.raises(ValueError, match=message):
            EZ.ez_table(item(quads, ez))
    with pytest.raises(ValueError, match="no bonds"):
        EZ.ez_table(dict(atom_type=mol[0], ez_quads=[[0, 2, 3, 4]], ez=[1]))


def test_the_command_line_tags_a_test_set_from_its_references(tmp_path, capsys):
    butene, (triene, tri_pos, _) = _butene(), EC.molecule("c14")
    propene = PR.graph([6, 6, 6] + [1] * 6, [(0, 1, 2), (1, 2, 1), (0, 3, 1), (0, 4, 1), (1, 5, 1), (2, 6, 1), (2, 7, 1), (2, 8, 1)])
    mols = [dict(atom_type=m[0], edge_index=m[1], edge_type=m[2], num_refs=2, name=name)
            for m, name in ((butene, "butene"), (triene, "triene"), (propene, "propene"), (butene, "no_refs"))]
    driver.save_testset(str(tmp_path / "test.npz"), mols)
    quads = EC.tables("c14")[0]
    refs = np.stack([tri_pos] * 3)
    ER.rotate_side(refs[2], 3, 4, [4, 5, 6, 7, 11, 12, 13])            # one of three references has the middle bond the other way
    rng = np.random.default_rng(0)
    np.savez(str(tmp_path / "refs.npz"), pos_ref_0=rng.normal(size=(2, 12, 3)), pos_ref_1=refs, pos_ref_2=rng.normal(size=(2, 9, 3)))
    out = EZ.main(["--testset", str(tmp_path / "test.npz"), "--refs", str(tmp_path / "refs.npz"), "--out", str(tmp_path / "tagged.npz")])
    lines = capsys.readouterr().out.splitlines()
    assert lines[1] == "triene: 3 stereogenic double bonds (0 in a ring), 1 with disagreeing references (3 tagged)"
    assert lines[2].startswith("propene: 0 stereogenic double bonds") and "no_refs: no pos_ref_3" in lines[3]
    z = np.load(str(tmp_path / "tagged.npz"))
    before = np.load(str(tmp_path / "test.npz"))
    assert sorted(set(z.files) - set(before.files)) == ["ez_0", "ez_1", "ez_2", "ez_quads_0", "ez_quads_1", "ez_quads_2"]
    for k in before.files:
        assert np.array_equal(z[k], before[k])
    assert z["ez_quads_1"].dtype == np.int32 and z["ez_quads_1"].tolist() == quads.tolist() and z["ez_1"].dtype == np.int8
    assert z["ez_1"].tolist() == EC.tables("c14")[1].tolist() == out["ez_1"].tolist()
    assert z["ez_quads_0"].tolist() == [[0, 2, 3, 4]] and z["ez_quads_2"].shape == (0, 4) and z["ez_2"].shape == (0,)
    # the tagged file is a test set: the tags come back with the molecules, pass ez_table, and survive a save
    loaded = driver.load_testset(str(tmp_path / "tagged.npz"))
    assert [("ez" in m, "ez_quads" in m) for m in loaded] == [(True, True)] * 3 + [(False, False)]
    assert EZ.ez_table(loaded[1])[0].tolist() == quads.tolist()
    driver.save_testset(str(tmp_path / "again.npz"), loaded)
    again = np.load(str(tmp_path / "again.npz"))
    assert np.array_equal(again["ez_quads_1"], z["ez_quads_1"]) and np.array_equal(again["ez_1"], z["ez_1"]) and "ez_3" not in again.files


def test_the_export_is_declared_and_the_abi_version_stays():
    args = _lib.EXPORTS["agdiff_flip_double_bonds"]
    assert args == [ctypes.c_void_p] * 5 + [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 3
    lib = _lib.load()
    assert hasattr(lib, "agdiff_flip_double_bonds") and list(lib.agdiff_flip_double_bonds.argtypes) == args
    assert lib.agdiff_abi_version() == _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    # nothing to do is no launch and no error, whatever the pointers
    null = ctypes.c_void_p(0)
    assert lib.agdiff_flip_double_bonds(null, null, null, null, null, 4, 6, 0, null, null, null) == 0
    assert lib.agdiff_flip_double_bonds(null, null, null, null, null, 0, 6, 2, null, null, null) == 0
    assert lib.agdiff_flip_double_bonds(null, null, null, null, null, 4, 0, 2, null, null, null) == -1
    assert lib.agdiff_flip_double_bonds(null, null, null, null, null, 4, 6, 2, null, null, null) == -1


def test_the_bridge_search_moved_and_kept_its_old_name():
    from agdiff_amd import molecule, torsions
    assert torsions._bridges is molecule.bridges
    assert molecule.bridges([[1], [0, 2, 3], [1, 3], [1, 2, 4], [3]]) == {(0, 1), (3, 4)}


def test_the_fp32_rounding_between_nested_flips_is_what_the_gpu_test_allows_for():
    """max |ez_ref rounding - ez_ref exact| over the atoms that two or more flips moved, in every shape of the GPU test: the figure
    tests/test_hip_ezbonds.py takes four times of for those atoms."""
    worst, entries = EC.nested_deviation()
    print("nested flips: max |rounding - exact| = %.3e A over %d (conformer, atom) entries" % (worst, entries))
    assert entries > 1000 and 0.5 * EC.NESTED_MEASURED <= worst <= 2.0 * EC.NESTED_MEASURED
