"""No GPU: the host side of the handedness fix (agdiff_amd/stereo.py) -- tetrahedral centres by colour refinement, target
parities from reference conformers -- the C ABI of the three entry points as the header declares it, their host-side argument
checks (every one returns before any launch), and `stereo_<i>` in the test set files."""
import ctypes

import numpy as np
import pytest

from agdiff_amd import _lib

VP, I32 = ctypes.c_void_p, ctypes.c_int32


def _graph(atoms, bonds):
    """(atom_type [n], bond_index [2, 2e], bond_type [2e]) from (i, j, type) triples, both directions listed"""
    bi = np.array([[i, j] for i, j, _ in bonds] + [[j, i] for i, j, _ in bonds]).T
    bt = np.array([t for _, _, t in bonds] * 2)
    return np.array(atoms), bi, bt


def chfclbr():
    return _graph([6, 1, 9, 17, 35], [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1)])


def butan_2_ol():
    """C0 H3 - C1 H(OH) - C2 H2 - C3 H3; O4; H5-7 on C0, H8 on C1, H9-10 on C2, H11-13 on C3, H14 on O4"""
    bonds = [(0, 1, 1), (1, 2, 1), (2, 3, 1), (1, 4, 1), (0, 5, 1), (0, 6, 1), (0, 7, 1), (1, 8, 1), (2, 9, 1), (2, 10, 1),
             (3, 11, 1), (3, 12, 1), (3, 13, 1), (4, 14, 1)]
    return _graph([6, 6, 6, 6, 8] + [1] * 10, bonds)


def dichlorobutane_2_3():
    """C0 H3 - C1 HCl - C2 HCl - C3 H3; Cl4 on C1, Cl5 on C2; H6-8 on C0, H9 on C1, H10 on C2, H11-13 on C3"""
    bonds = [(0, 1, 1), (1, 2, 1), (2, 3, 1), (1, 4, 1), (2, 5, 1), (0, 6, 1), (0, 7, 1), (0, 8, 1), (1, 9, 1), (2, 10, 1),
             (3, 11, 1), (3, 12, 1), (3, 13, 1)]
    return _graph([6, 6, 6, 6, 17, 17] + [1] * 8, bonds)


def neopentane():
    bonds = [(0, k, 1) for k in range(1, 5)] + [(c, 5 + 3 * (c - 1) + h, 1) for c in range(1, 5) for h in range(3)]
    return _graph([6] * 5 + [1] * 12, bonds)


def test_tetrahedral_centres_of_four_molecules():
    from agdiff_amd.stereo import tetrahedral_centres
    c, q = tetrahedral_centres(*chfclbr())
    assert c.dtype == np.int32 and q.dtype == np.int32 and c.tolist() == [0] and q.tolist() == [[1, 2, 3, 4]]
    c, q = tetrahedral_centres(*butan_2_ol())
    assert c.tolist() == [1] and q.tolist() == [[0, 2, 4, 8]]
    c, q = tetrahedral_centres(*dichlorobutane_2_3())
    assert c.tolist() == [1, 2] and q.tolist() == [[0, 2, 4, 9], [1, 3, 5, 10]]
    c, q = tetrahedral_centres(*neopentane())
    assert c.shape == (0,) and q.shape == (0, 4)


@pytest.mark.parametrize("mol", [chfclbr, butan_2_ol, dichlorobutane_2_3, neopentane])
def test_centres_follow_a_relabelling_of_the_atoms(mol):
    from agdiff_amd.stereo import tetrahedral_centres
    at, bi, bt = mol()
    c0, q0 = tetrahedral_centres(at, bi, bt)
    rng = np.random.default_rng(len(at))
    for _ in range(3):
        new = rng.permutation(len(at))                     # atom i becomes atom new[i]
        at2 = np.empty_like(at)
        at2[new] = at
        shuffle = rng.permutation(bi.shape[1])
        c1, q1 = tetrahedral_centres(at2, new[bi][:, shuffle], bt[shuffle])
        assert c1.tolist() == sorted(new[c0].tolist())
        want = {int(new[c]): sorted(new[q].tolist()) for c, q in zip(c0, q0)}
        assert {int(c): q.tolist() for c, q in zip(c1, q1)} == want


def test_two_and_three_hop_edges_change_nothing():
    from agdiff_amd.stereo import tetrahedral_centres
    for mol in (butan_2_ol, dichlorobutane_2_3, neopentane):
        at, bi, bt = mol()
        c0, q0 = tetrahedral_centres(at, bi, bt)
        n = len(at)
        extra = np.array([[i, j] for i in range(n) for j in range(n) if i != j and (i + j) % 3 == 0]).T
        # (hop entries never duplicate a bond in a real edge list; here they may, and must still be ignored: they come last)
        bi2 = np.concatenate([bi, extra], axis=1)
        bt2 = np.concatenate([bt, np.where(np.arange(extra.shape[1]) % 2 == 0, 22, 23)])
        c1, q1 = tetrahedral_centres(at, bi2, bt2)
        assert np.array_equal(c0, c1) and np.array_equal(q0, q1)


def _tetrahedron(sign):
    """five atoms: a centre at the origin and four neighbours 1..4 whose signed volume (quad (1, 2, 3, 4)) has the given sign"""
    p = np.array([[0, 0, 0], [1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64)
    from agdiff_amd.stereo import signed_volumes
    if np.sign(signed_volumes(p[None], [[1, 2, 3, 4]])[0, 0]) != sign:
        p = -p
    return p


def test_parities_from_conformers():
    from agdiff_amd.stereo import parities_from_conformers, signed_volumes
    quads = np.array([[1, 2, 3, 4]], dtype=np.int32)
    plus, minus = _tetrahedron(+1), _tetrahedron(-1)
    assert signed_volumes(plus[None], quads)[0, 0] > 0 > signed_volumes(minus[None], quads)[0, 0]
    # the definition, spelled out: (p_b - p_a) . ((p_c - p_a) x (p_d - p_a))
    a, b, c, d = plus[1:5]
    assert np.isclose(signed_volumes(plus[None], quads)[0, 0], np.dot(b - a, np.cross(c - a, d - a)))
    for p, s in ((plus, 1), (minus, -1)):
        t, dis = parities_from_conformers(p[None], quads)
        assert t.dtype == np.int8 and dis.dtype == np.int32 and t.tolist() == [s] and dis.tolist() == [0]
    t, dis = parities_from_conformers(np.stack([plus, minus, plus]), quads)
    assert t.tolist() == [1] and dis.tolist() == [1]
    t, dis = parities_from_conformers(np.stack([minus, plus, minus]), quads)
    assert t.tolist() == [-1] and dis.tolist() == [1]
    t, dis = parities_from_conformers(np.stack([plus, minus]), quads)
    assert t.tolist() == [0] and dis.tolist() == [1]
    flat = plus.copy(); flat[:, 2] = 0.0
    t, dis = parities_from_conformers(np.stack([flat, flat]), quads)
    assert t.tolist() == [0] and dis.tolist() == [0]
    t, dis = parities_from_conformers(plus[None], np.zeros((0, 4), dtype=np.int32))
    assert t.shape == (0,) and dis.shape == (0,)


def test_stereo_quads_reads_the_tags_of_an_item():
    from agdiff_amd.stereo import stereo_quads
    at, bi, bt = dichlorobutane_2_3()
    st = np.zeros(len(at), dtype=np.int8)
    st[1], st[2] = 1, -1
    q, t = stereo_quads(dict(atom_type=at, edge_index=bi, edge_type=bt, stereo=st))
    assert q.tolist() == [[0, 2, 4, 9], [1, 3, 5, 10]] and t.tolist() == [1, -1] and t.dtype == np.int8
    with pytest.raises(ValueError, match="stereo"):
        stereo_quads(dict(atom_type=at, edge_index=bi, edge_type=bt))
    st[4] = 1                                               # a chlorine: one neighbour
    with pytest.raises(ValueError, match="four"):
        stereo_quads(dict(atom_type=at, edge_index=bi, edge_type=bt, stereo=st))


def test_exports_and_abi_version():
    assert _lib.EXPORTS["agdiff_rmsd_matrix_hands"] == [VP, VP, VP, VP, I32, I32, I32, I32, I32, VP, VP, VP, VP]
    assert _lib.EXPORTS["agdiff_chiral_verdict"] == [VP, VP, VP, I32, I32, I32, VP, VP, VP]
    assert _lib.EXPORTS["agdiff_mirror_conformers"] == [VP, VP, I32, I32, VP]
    assert _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    lib = _lib.load()
    assert lib.agdiff_abi_version() == 48
    for name in ("agdiff_rmsd_matrix_hands", "agdiff_chiral_verdict", "agdiff_mirror_conformers"):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == _lib.EXPORTS[name]


def test_the_three_entry_points_check_their_arguments_on_the_host():
    lib = _lib.load()
    keep = (ctypes.c_uint64 * 8)()
    keep2 = (ctypes.c_uint64 * 8)()
    p, p2, null = ctypes.c_void_p(ctypes.addressof(keep)), ctypes.c_void_p(ctypes.addressof(keep2)), ctypes.c_void_p(0)
    ok = dict(ref=p, gen=p, idx=p, perms=null, R=2, G=4, n=5, m=3, P=0, scratch=p, proper=p, mirror=p2)

    def hands(**kw):
        a = dict(ok, **kw)
        return lib.agdiff_rmsd_matrix_hands(a["ref"], a["gen"], a["idx"], a["perms"], a["R"], a["G"], a["n"], a["m"], a["P"],
                                            a["scratch"], a["proper"], a["mirror"], null)
    for bad in (dict(ref=null), dict(gen=null), dict(idx=null), dict(scratch=null), dict(proper=null), dict(mirror=null),
                dict(mirror=p), dict(R=-1), dict(G=-1), dict(n=0), dict(m=0), dict(m=6), dict(perms=p, P=0)):
        assert hands(**bad) == -1, bad
    big = _lib.DEFINES["AGDIFF_RMSD_MAX_ATOMS"] + 1
    assert hands(n=big + 10, m=big) == -2
    assert hands(G=0) == 0 and hands(R=0) == 0

    verdict = lambda pos=p, quads=p, target=p, G=2, n=5, C=1, vol=null, out=p: lib.agdiff_chiral_verdict(pos, quads, target, G, n, C,
                                                                                                       vol, out, null)
    for bad in (dict(pos=null), dict(quads=null), dict(target=null), dict(out=null), dict(G=-1), dict(n=0), dict(C=-1)):
        assert verdict(**bad) == -1, bad
    assert verdict(G=0) == 0 and verdict(G=0, C=0, quads=null, target=null) == 0

    mirror = lambda pos=p, flags=p, G=2, n=5: lib.agdiff_mirror_conformers(pos, flags, G, n, null)
    for bad in (dict(pos=null), dict(flags=null), dict(G=-1), dict(n=0)):
        assert mirror(**bad) == -1, bad
    assert mirror(G=0) == 0
    del keep, keep2


def test_testset_files_carry_stereo(tmp_path):
    from agdiff_amd.driver import load_testset, save_testset
    mols = []
    for k, mol in enumerate((butan_2_ol, neopentane)):
        at, bi, bt = mol()
        mols.append(dict(atom_type=at, edge_index=bi, edge_type=bt, num_refs=2 + k, name="m%d" % k))
    st = np.zeros(len(mols[0]["atom_type"]), dtype=np.int8)
    st[1] = -1
    mols[0]["stereo"] = st
    save_testset(str(tmp_path / "with.npz"), mols)
    back = load_testset(str(tmp_path / "with.npz"))
    assert back[0]["stereo"].dtype == np.int8 and np.array_equal(back[0]["stereo"], st) and "stereo" not in back[1]
    assert "stereo_1" not in np.load(str(tmp_path / "with.npz")).files
    save_testset(str(tmp_path / "without.npz"), [{k: v for k, v in m.items() if k != "stereo"} for m in mols])
    plain = load_testset(str(tmp_path / "without.npz"))
    assert all("stereo" not in m for m in plain)
    assert sorted(plain[0]) == ["atom_type", "edge_index", "edge_type", "index", "name", "num_refs"]
    assert sorted(np.load(str(tmp_path / "without.npz")).files) == sorted(
        ["count"] + ["%s_%d" % (k, i) for i in range(2) for k in ("atom_type", "edge_index", "edge_type", "num_refs", "name")])


def test_cli_tags_a_test_set_from_its_references(tmp_path, capsys):
    from agdiff_amd import stereo
    from agdiff_amd.driver import load_testset, save_testset
    at, bi, bt = chfclbr()
    at2, bi2, bt2 = neopentane()
    save_testset(str(tmp_path / "t.npz"), [dict(atom_type=at, edge_index=bi, edge_type=bt, num_refs=3, name="chfclbr"),
                                           dict(atom_type=at2, edge_index=bi2, edge_type=bt2, num_refs=1, name="neo")])
    plus, minus = _tetrahedron(+1), _tetrahedron(-1)
    np.savez(str(tmp_path / "r.npz"), pos_ref_0=np.stack([minus, minus, plus]).astype(np.float32),
             pos_ref_1=np.zeros((1, len(at2), 3), np.float32))
    stereo.main(["--testset", str(tmp_path / "t.npz"), "--refs", str(tmp_path / "r.npz"), "--out", str(tmp_path / "o.npz")])
    said = capsys.readouterr().out
    assert "chfclbr: 1 tetrahedral centres, 1 with disagreeing references" in said and "neo: 0 tetrahedral centres" in said
    back = load_testset(str(tmp_path / "o.npz"))
    assert back[0]["stereo"].tolist() == [-1, 0, 0, 0, 0] and not back[1]["stereo"].any()
    assert back[0]["num_refs"] == 3 and np.array_equal(back[0]["edge_index"], bi)


def test_the_driver_switch_needs_the_tags(tmp_path):
    from agdiff_amd import driver
    at, bi, bt = chfclbr()
    mols = [dict(atom_type=at, edge_index=bi, edge_type=bt, num_refs=1, name="untagged", index=0)]
    with pytest.raises(ValueError, match="stereo"):
        driver.run_job(object(), mols, str(tmp_path / "o"), driver.num_confs("2x"), 1000, {}, "cpu", fix_handedness=True)
