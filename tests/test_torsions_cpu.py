"""No GPU: the host side of the torsion fingerprint deviation (agdiff_amd/torsions.py) -- rotatable bonds, columns and the column
mappings under the molecule's symmetry -- the float64 restatement of the definitions (tests/tfd_ref.py) on the cases the contract
pins, the C ABI of the two entry points as the header declares it, their host-side argument checks (every one returns before any
launch) and the command lines' refusal of two thresholds."""
import ctypes

import numpy as np
import pytest

import tfd_ref as TR
from agdiff_amd import _lib

VP, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float


def _item(mol):
    at, bi, bt = mol
    return dict(atom_type=at, bond_index=bi, bond_type=bt)


# (molecule, T, Q, heavy-atom automorphisms, distinct tmap rows)
COUNTS = [(TR.alkane(4), 1, 1, 2, 1), (TR.alkane(5), 2, 2, 2, 2), (TR.alkane(6), 3, 3, 2, 2), (TR.alkane(3), 0, 0, 2, 1),
          (TR.but_2_yne(), 0, 0, 2, 1), (TR.toluene(), 0, 0, 2, 1), (TR.cyclohexane(), 0, 0, 12, 1), (TR.biphenyl(), 1, 4, 8, 4)]


@pytest.mark.parametrize("k", range(len(COUNTS)))
def test_rotatable_bonds_and_tables_of_small_molecules(k):
    from agdiff_amd.evaluation import heavy_atom_automorphisms
    from agdiff_amd.torsions import rotatable_bonds, torsion_table
    mol, T, Q, A, rows = COUNTS[k]
    bonds, canon = rotatable_bonds(*mol)
    quads, tmap = torsion_table(_item(mol))
    assert bonds.dtype == canon.dtype == quads.dtype == tmap.dtype == np.int32
    assert bonds.shape == (T, 2) and canon.shape == (T, 4) and quads.shape == (Q, 4) and tmap.shape == (rows, T)
    assert heavy_atom_automorphisms(*mol).shape[0] == A
    assert np.array_equal(bonds, canon[:, 1:3]) and (bonds[:, 0] < bonds[:, 1]).all()
    assert bonds.tolist() == sorted(bonds.tolist())
    # row 0 is the canonical columns; every row names columns, and columns of the right bond's image
    assert np.array_equal(quads[tmap[0]], canon)
    assert (tmap >= 0).all() and (tmap < max(Q, 1)).all()
    assert len({tuple(r) for r in tmap.tolist()}) == tmap.shape[0]
    # the columns are ordered by bond, then a, then b
    assert quads[:, [1, 2, 0, 3]].tolist() == sorted(quads[:, [1, 2, 0, 3]].tolist())


def test_named_results():
    from agdiff_amd.torsions import rotatable_bonds, torsion_table
    bonds, canon = rotatable_bonds(*TR.alkane(6))
    assert bonds.tolist() == [[1, 2], [2, 3], [3, 4]] and canon.tolist() == [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5]]
    assert torsion_table(_item(TR.alkane(6)))[1].tolist() == [[0, 1, 2], [2, 1, 0]]
    quads, tmap = torsion_table(_item(TR.biphenyl()))
    assert quads.tolist() == [[1, 0, 6, 7], [1, 0, 6, 11], [5, 0, 6, 7], [5, 0, 6, 11]]
    assert tmap[0].tolist() == [0] and sorted(tmap[:, 0].tolist()) == [0, 1, 2, 3]
    # an isopropyl end: three columns at one end, and perms given directly are honoured in place of the bonds
    mol = TR.graph([6] * 5 + [8], [(0, 1, 1), (1, 2, 1), (1, 3, 1), (3, 4, 1), (4, 5, 1)])
    quads, tmap = torsion_table(_item(mol))
    assert quads.tolist() == [[0, 1, 3, 4], [2, 1, 3, 4], [1, 3, 4, 5]] and tmap.tolist() == [[0, 2], [1, 2]]
    ident = dict(_item(mol), perms=np.arange(6, dtype=np.int32)[None])
    assert torsion_table(ident)[1].tolist() == [[0, 2]]
    with pytest.raises(ValueError, match="automorphism"):
        torsion_table(dict(_item(mol), perms=np.array([[0, 1, 2, 3, 4, 5], [1, 0, 2, 3, 4, 5]], dtype=np.int32)))
    with pytest.raises(ValueError, match="bonds"):
        torsion_table(dict(atom_type=mol[0]))


def test_hydrogens_and_hop_entries_change_nothing():
    from agdiff_amd.torsions import rotatable_bonds, torsion_table
    full, bare = TR.butane_with_hydrogens_and_hops(), TR.alkane(4)
    assert (full[2] >= 22).sum() > 20 and (full[0] == 1).sum() == 10
    for a, b in zip(rotatable_bonds(*full), rotatable_bonds(*bare)):
        assert np.array_equal(a, b)
    for a, b in zip(torsion_table(_item(full)), torsion_table(_item(bare))):
        assert np.array_equal(a, b)
    # a ring bond, a double bond and a bond next to a triple bond are not rotatable; the bond beside them is
    mol = TR.graph([6] * 9, [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 1), (4, 5, 1), (5, 6, 3), (3, 7, 1), (7, 8, 1), (8, 3, 1)])
    assert rotatable_bonds(*mol)[0].tolist() == [[2, 3], [3, 4]]


def test_reference_pins_the_sign_reversal_and_mirror_of_a_dihedral():
    for phi in (0.0, 1.0, np.pi / 2, -2.5, np.pi):
        p = np.array([[1, 0, 0], [0, 0, 0], [0, 0, 1], [np.cos(phi), np.sin(phi), 1]])
        th = TR.dihedrals(p[None], [[0, 1, 2, 3], [3, 2, 1, 0]])[0]
        assert TR.circular_difference(th[0], phi) < 1e-15 and TR.circular_difference(th[0], th[1]) < 1e-15
        assert TR.circular_difference(TR.dihedrals(-p[None], [[0, 1, 2, 3]])[0, 0], -phi) < 1e-15
    p = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [2, 1, 0], [2, 1, 0], [np.nan, 0, 0]])
    th = TR.dihedrals(p[None], [[0, 1, 2, 3], [0, 1, 3, 4], [0, 1, 3, 5], [0, 1, 3, 6], [1, 2, 3, 0]])[0]
    assert np.isnan(th[:4]).all() and np.isfinite(th[4])
    # the chain builder the GPU tests construct rotamers with follows the same convention
    want = np.array([np.pi, np.pi / 3, -np.pi / 3, 2.0])
    got = TR.dihedrals(TR.chain_positions(want)[None], [[i, i + 1, i + 2, i + 3] for i in range(4)])[0]
    assert np.abs(got - want).max() < 1e-12


def test_reference_tfd_is_symmetric_only_with_both_directions():
    from agdiff_amd.torsions import torsion_table
    quads, tmap = torsion_table(_item(TR.biphenyl()))
    rng = np.random.default_rng(0)
    ang = TR.dihedrals(rng.normal(size=(6, 12, 3)), quads)
    two = TR.tfd(ang, ang, tmap)
    one = TR.tfd(ang, ang, tmap, one_way=True)
    assert np.array_equal(two, two.T) and not np.diag(two).any() and (two >= 0).all() and (two <= 1).all()
    assert np.abs(one - one.T).max() > 0.05 and (two <= one).all()
    # butane: anti / gauche+ / gauche-
    a = np.array([[np.pi], [np.pi / 3], [-np.pi / 3]])
    t = TR.tfd(a, a, np.zeros((1, 1), dtype=np.int32))
    assert np.allclose(t, [[0, 2 / 3, 2 / 3], [2 / 3, 0, 2 / 3], [2 / 3, 2 / 3, 0]], atol=1e-15)
    assert np.allclose(TR.tfd(a, a, np.zeros((1, 1), dtype=np.int32), mirror=True)[1, 2], 0.0, atol=1e-15)
    a[0, 0] = np.nan
    assert TR.tfd(a, a, np.zeros((1, 1), dtype=np.int32))[0].tolist() == [1.0, 1.0, 1.0]
    assert not TR.tfd(a, a, np.zeros((1, 0), dtype=np.int32)).any()


def test_exports_and_abi_version():
    assert _lib.EXPORTS["agdiff_torsion_angles"] == [VP, VP, I32, I32, I32, VP, VP]
    assert _lib.EXPORTS["agdiff_tfd_matrix"] == [VP, VP, VP, VP, I32, I32, I32, I32, I32, F32, VP, VP, VP, VP]
    assert _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48 and _lib.DEFINES["AGDIFF_TFD_MAX_COLUMNS"] == 512
    lib = _lib.load()
    assert lib.agdiff_abi_version() == 48
    for name in ("agdiff_torsion_angles", "agdiff_tfd_matrix"):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == _lib.EXPORTS[name]


def test_the_two_entry_points_check_their_arguments_on_the_host():
    lib = _lib.load()
    keep = (ctypes.c_uint64 * 8)()
    keep2 = (ctypes.c_uint64 * 8)()
    p, p2, null = ctypes.c_void_p(ctypes.addressof(keep)), ctypes.c_void_p(ctypes.addressof(keep2)), ctypes.c_void_p(0)
    odd = ctypes.c_void_p(ctypes.addressof(keep) + 4)

    angles = lambda pos=p, quads=p, G=2, n=5, Q=3, out=p: lib.agdiff_torsion_angles(pos, quads, G, n, Q, out, null)
    for bad in (dict(pos=null), dict(quads=null), dict(out=null), dict(G=-1), dict(n=0), dict(n=-3), dict(Q=-1)):
        assert angles(**bad) == -1, bad
    assert angles(G=0) == 0 and angles(Q=0) == 0 and angles(Q=0, quads=null) == 0

    ok = dict(x=p, y=p, tmap=p, w=null, R=2, G=4, Q=6, T=3, P=2, thresh=0.2, out=p, mirror=null, bits=null)

    def tfd(**kw):
        a = dict(ok, **kw)
        return lib.agdiff_tfd_matrix(a["x"], a["y"], a["tmap"], a["w"], a["R"], a["G"], a["Q"], a["T"], a["P"], a["thresh"], a["out"],
                                     a["mirror"], a["bits"], null)
    for bad in (dict(x=null), dict(y=null), dict(tmap=null), dict(R=-1), dict(G=-1), dict(Q=-1), dict(T=-1), dict(P=0), dict(P=-2),
                dict(T=7), dict(out=null), dict(mirror=p), dict(out=null, mirror=null, bits=null), dict(bits=p2, thresh=-0.1),
                dict(bits=p2, thresh=float("nan")), dict(bits=odd)):
        assert tfd(**bad) == -1, bad
    big = _lib.DEFINES["AGDIFF_TFD_MAX_COLUMNS"] + 1
    assert tfd(Q=big) == -2 and tfd(Q=big, T=big) == -2
    assert tfd(G=0) == 0 and tfd(R=0) == 0 and tfd(R=0, out=null, bits=p2) == 0 and tfd(G=0, mirror=p2) == 0
    assert tfd(G=0, Q=0, T=0, x=null, y=null, tmap=null) == 0
    del keep, keep2


def test_wrapper_checks_come_before_any_launch():
    from agdiff_amd import driver
    from agdiff_amd.evaluation import CovMatEvaluator
    from agdiff_amd.ensemble import prune_conformers
    with pytest.raises(ValueError, match="metric"):
        prune_conformers(dict(atom_type=np.array([6, 6]), pos_gen=np.zeros((2, 2, 3))), 0.1, metric="angle")
    with pytest.raises(ValueError, match="metric"):
        CovMatEvaluator(metric="angle")
    assert np.allclose(CovMatEvaluator(metric="tfd").thresholds, np.arange(1, 61) * 0.01, atol=1e-15, rtol=0)
    assert np.array_equal(CovMatEvaluator().thresholds, np.arange(0.05, 3.05, 0.05))
    assert CovMatEvaluator(metric="tfd", thresholds=[0.2]).thresholds.tolist() == [0.2]
    at, bi, bt = TR.alkane(4)
    mols = [dict(atom_type=at, edge_index=bi, edge_type=bt, num_refs=1, name="butane", index=0)]
    with pytest.raises(ValueError, match="prune_tfd"):
        driver.run_job(object(), mols, "unused", driver.num_confs("2x"), 1000, {}, "cpu", prune_rms=0.5, prune_tfd=0.2)
    with pytest.raises(ValueError, match="prune_tfd"):
        driver.run_job(object(), mols, "unused", driver.num_confs("2x"), 1000, {}, "cpu", prune_tfd=-0.2)


def test_ensemble_command_line_takes_exactly_one_threshold(tmp_path, capsys):
    from agdiff_amd import ensemble
    common = ["--samples", str(tmp_path / "none.npz"), "--testset", str(tmp_path / "none.npz"), "--out", str(tmp_path / "o.npz")]
    for extra in (["--prune-rms", "0.5", "--prune-tfd", "0.2"], []):
        with pytest.raises(SystemExit) as e:
            ensemble.main(common + extra)
        assert e.value.code == 2
    said = capsys.readouterr().err
    assert "not allowed with" in said and "one of the arguments --prune-rms --prune-tfd is required" in said
    assert not (tmp_path / "o.npz").exists()
