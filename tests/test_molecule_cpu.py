"""No GPU: what the post-sampling modules share on the host (agdiff_amd/molecule.py) -- field access, the bond lookup, the
bonded-neighbour graph, colour refinement, host copies, the threshold check and the item loops of the command lines."""
import types

import numpy as np
import pytest

from agdiff_amd import molecule as M

NO_BONDS = "the item carries no bonds (bond_index + bond_type, or edge_index + edge_type)"


def _graph(atoms, bonds):
    """(atom_type [n], bond_index [2, 2e], bond_type [2e]) from (i, j, type) triples, both directions listed"""
    bi = np.array([[i, j] for i, j, _ in bonds] + [[j, i] for i, j, _ in bonds]).T
    bt = np.array([t for _, _, t in bonds] * 2)
    return np.array(atoms), bi, bt


@pytest.mark.parametrize("make", [dict, lambda **kw: types.SimpleNamespace(**kw)], ids=["dict", "object"])
def test_field_num_atoms_and_bonds_of(make):
    bi, bt, ei, et = np.array([[0], [1]]), np.array([1]), np.array([[0, 1], [1, 2]]), np.array([1, 23])
    item = make(atom_type=np.array([[6, 6, 8]]), edge_index=ei, edge_type=et)
    assert M.field(item, "atom_type").shape == (1, 3) and M.field(item, "perms") is None
    assert M.num_atoms(item) == 3
    got = M.bonds_of(item)
    assert got[0] is ei and got[1] is et
    both = make(atom_type=np.array([6, 6, 8]), edge_index=ei, edge_type=et, bond_index=bi, bond_type=bt)
    got = M.bonds_of(both)
    assert got[0] is bi and got[1] is bt                                   # bond_* wins over edge_*
    for bare in (make(atom_type=np.array([6])), make(atom_type=np.array([6]), edge_index=ei), make(atom_type=np.array([6]), bond_type=bt)):
        assert M.bonds_of(bare, required=False) == (None, None)
        with pytest.raises(ValueError) as e:
            M.bonds_of(bare)
        assert str(e.value) == NO_BONDS
    with pytest.raises(KeyError):
        M.num_atoms(make(pos_gen=np.zeros((1, 3))))


def test_the_modules_raise_the_shared_text_for_an_item_without_bonds():
    from agdiff_amd.stereo import stereo_quads
    from agdiff_amd.validity import check_geometry
    item = dict(atom_type=np.array([6, 1, 9, 17, 35]), stereo=np.array([1, 0, 0, 0, 0], dtype=np.int8), pos_gen=np.zeros((1, 5, 3)))
    for fn in (stereo_quads, check_geometry):
        with pytest.raises(ValueError) as e:
            fn(item)
        assert str(e.value) == NO_BONDS


def test_heavy_atoms():
    h = M.heavy_atoms(np.array([[1, 6, 1, 8, 1]]))
    assert h.dtype == np.int32 and h.tolist() == [1, 3]
    for none in ([], [1, 1]):
        with pytest.raises(ValueError, match="molecule without heavy atoms"):
            M.heavy_atoms(np.array(none))


def test_bonded_neighbours_on_a_five_atom_graph():
    # 0 - 1 listed in both directions, 1 -> 2 in one direction only, 2 = 3 double; a type 0 entry, a type 22 entry and a self loop
    bi = np.array([[0, 1, 1, 2, 3, 0, 0, 4], [1, 0, 2, 3, 2, 4, 3, 4]])
    bt = np.array([1, 1, 1, 2, 2, 0, 22, 1])
    adj = M.bonded_neighbours(5, bi, bt)
    assert adj == [{1: 1}, {0: 1, 2: 1}, {1: 1, 3: 2}, {2: 2}, {}]
    assert all(type(k) is int and type(v) is int for a in adj for k, v in a.items())
    for bad in (5, -1):
        with pytest.raises(ValueError) as e:
            M.bonded_neighbours(5, np.array([[0, 1], [1, bad]]), np.array([1, 1]))
        assert str(e.value) == "bond (1, %d) outside the molecule's 5 atoms" % bad
    # an entry that is no bond is never looked at, whatever it names
    assert M.bonded_neighbours(2, np.array([[0, 0], [1, 7]]), np.array([1, 23])) == [{1: 1}, {0: 1}]


def test_automorphisms_range_check_their_bonds():
    from agdiff_amd.evaluation import heavy_atom_automorphisms
    for bad in (3, -1):
        with pytest.raises(ValueError, match="outside the molecule's 3 atoms"):
            heavy_atom_automorphisms(np.array([6, 6, 8]), np.array([[0, 1], [1, bad]]), np.array([1, 1]))


def test_refine_colours():
    # ethanol: C0 H3 - C1 H2 - O2 H; H3-5 on C0, H6-7 on C1, H8 on O2
    at, bi, bt = _graph([6, 6, 8] + [1] * 6, [(0, 1, 1), (1, 2, 1), (0, 3, 1), (0, 4, 1), (0, 5, 1), (1, 6, 1), (1, 7, 1), (2, 8, 1)])
    c = M.refine_colours(at, M.bonded_neighbours(9, bi, bt))
    assert len({c[0], c[1], c[2]}) == 3                                     # the heavy atoms are all distinct
    assert c[3] == c[4] == c[5] and c[6] == c[7] and len({c[3], c[6], c[8]}) == 3
    assert sorted(set(c)) == list(range(6)) and all(type(x) is int for x in c)         # dense numbering
    # benzene's heavy ring: one class
    at, bi, bt = _graph([6] * 6, [(i, (i + 1) % 6, 12) for i in range(6)])
    assert len(set(M.refine_colours(at, M.bonded_neighbours(6, bi, bt)))) == 1
    # a bond type separates what the elements do not: C - C = C
    at, bi, bt = _graph([6] * 3, [(0, 1, 1), (1, 2, 2)])
    assert len(set(M.refine_colours(at, M.bonded_neighbours(3, bi, bt)))) == 3
    assert M.refine_colours([], []) == []


def test_as_host_copies_when_a_dtype_is_given():
    import torch
    ro = np.arange(6, dtype=np.int64).reshape(2, 3)
    ro.setflags(write=False)
    assert M.as_host(ro) is ro
    for src in (ro, np.asfortranarray(ro), ro[:, ::2], torch.arange(6).reshape(2, 3), torch.arange(6).reshape(3, 2).t()):
        got = M.as_host(src, np.int32)
        assert got.dtype == np.int32 and got.flags.writeable and got.flags.c_contiguous and got.flags.owndata
        assert np.array_equal(got, np.asarray(src))
    same = M.as_host(ro, np.int64)                                          # (a copy even when nothing has to be converted)
    assert same.flags.writeable and not np.shares_memory(same, ro)
    t = torch.arange(4, dtype=torch.float32)
    got = M.as_host(t, np.float32)
    got[0] = 9.0
    assert t[0] == 0.0
    assert M.as_host(torch.ones(2, requires_grad=True)).tolist() == [1.0, 1.0]
    assert M.as_host([1, 2]).tolist() == [1, 2]


def test_check_threshold_carries_both_messages():
    assert M.check_threshold(0.0, "RMSD") == 0.0 and M.check_threshold("0.25", "TFD") == 0.25
    for bad in (-1e-9, float("nan")):
        with pytest.raises(ValueError) as e:
            M.check_threshold(bad, "RMSD")
        assert str(e.value) == "the RMSD threshold must be >= 0 (got %r)" % (bad,)
        with pytest.raises(ValueError) as e:
            M.check_threshold(bad, "TFD")
        assert str(e.value) == "the TFD threshold must be >= 0 (got %r)" % (bad,)
    from agdiff_amd.ensemble import threshold_bits
    from agdiff_amd.torsions import tfd_self
    with pytest.raises(ValueError, match="the RMSD threshold must be >= 0"):
        threshold_bits({}, -1.0)
    with pytest.raises(ValueError, match="the TFD threshold must be >= 0"):
        tfd_self({}, threshold=-1.0)


def test_sampled_and_reference_items(tmp_path):
    from agdiff_amd.driver import save_testset
    e0, e1 = np.array([[0, 1], [1, 0]]), np.array([[0, 1, 1, 2], [1, 0, 2, 1]])
    save_testset(tmp_path / "test.npz", [dict(atom_type=[6, 8], edge_index=e0, edge_type=[1, 1], name="a"),
                                         dict(atom_type=[6, 6, 8], edge_index=e1, edge_type=[1, 1, 2, 2], name="b", stereo=[0, 1, 0])])
    gen1 = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    np.savez(tmp_path / "samples.npz", pos_gen_1=gen1)                      # molecule 0 was not sampled
    got = list(M.sampled_items(tmp_path / "test.npz", tmp_path / "samples.npz"))
    assert len(got) == 1
    mol, item = got[0]
    assert mol["index"] == 1 and mol["name"] == "b" and mol["stereo"].tolist() == [0, 1, 0]
    assert sorted(item) == ["atom_type", "edge_index", "edge_type", "pos_gen"]
    assert item["atom_type"].tolist() == [6, 6, 8] and np.array_equal(item["pos_gen"], gen1)
    assert np.array_equal(item["edge_index"], e1) and item["edge_type"].tolist() == [1, 1, 2, 2]

    ref0, ref1 = np.zeros((1, 2, 3), dtype=np.float32), np.ones((3, 3, 3), dtype=np.float32)
    np.savez(tmp_path / "refs.npz", pos_ref_0=ref0, atom_type_0=np.array([6, 8]), pos_ref_1=ref1, atom_type_1=np.array([6, 6, 8]),
             smiles_1=np.str_("CC=O"), perms_1=np.array([[0, 1, 2]], dtype=np.int32), bond_index_1=e1, bond_type_1=np.array([1, 1, 2, 2]),
             edge_index_1=e1, edge_type_1=np.array([1, 1, 2, 2]), unrelated=np.zeros(1))
    got = dict(M.reference_items(tmp_path / "refs.npz", tmp_path / "samples.npz"))
    assert sorted(got) == ["0", "1"]
    assert sorted(got["0"]) == ["atom_type", "pos_ref"] and np.array_equal(got["0"]["pos_ref"], ref0)      # yielded, without pos_gen
    assert sorted(got["1"]) == ["atom_type", "bond_index", "bond_type", "edge_index", "edge_type", "perms", "pos_gen", "pos_ref", "smiles"]
    assert got["1"]["smiles"] == "CC=O" and type(got["1"]["smiles"]) is str
    assert np.array_equal(got["1"]["pos_gen"], gen1) and np.array_equal(got["1"]["pos_ref"], ref1)
    assert got["1"]["perms"].tolist() == [[0, 1, 2]] and np.array_equal(got["1"]["bond_index"], e1)
