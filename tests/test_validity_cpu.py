"""No GPU: the host side of the geometry checks (agdiff_amd/validity.py) -- exclusions, the two bound tables -- the float64 restatement
of the definitions (tests/validity_ref.py) on cases worked out by hand, the C ABI of the two entry points as the header declares it,
their host-side argument checks (every one returns before any launch), and the wrappers' and command lines' own refusals."""
import ctypes

import numpy as np
import pytest

import validity_ref as VR
from agdiff_amd import _lib

VP, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float


def _item(mol, **kw):
    at, ei, et = mol
    return dict(atom_type=at, edge_index=ei, edge_type=et, **kw)


def _rows(ex_ptr, ex_idx):
    return [ex_idx[ex_ptr[i]:ex_ptr[i + 1]].tolist() for i in range(len(ex_ptr) - 1)]


def test_exports_and_the_slice_define():
    assert _lib.EXPORTS["agdiff_pair_bounds"] == [VP, VP, VP, VP, I32, I32, I32, VP, VP, VP, VP, VP]
    assert _lib.EXPORTS["agdiff_clash_scan"] == [VP, VP, VP, VP, I32, I32, F32, VP, VP, VP, VP, VP]
    assert _lib.DEFINES["AGDIFF_CLASH_SLICE"] == 256
    lib = _lib.load()
    assert lib.agdiff_abi_version() == _lib.DEFINES["AGDIFF_ABI_VERSION"]
    for name in ("agdiff_pair_bounds", "agdiff_clash_scan"):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == _lib.EXPORTS[name]


def test_the_two_entry_points_check_their_arguments_on_the_host():
    lib = _lib.load()
    keep = (ctypes.c_uint64 * 8)()
    p, null = ctypes.c_void_p(ctypes.addressof(keep)), ctypes.c_void_p(0)

    ok = dict(pos=p, pairs=p, lo=p, hi=p, G=2, n=5, K=3, dist=null, worst=p, worst_pair=p, n_bad=p)

    def bounds(**kw):
        a = dict(ok, **kw)
        return lib.agdiff_pair_bounds(a["pos"], a["pairs"], a["lo"], a["hi"], a["G"], a["n"], a["K"], a["dist"], a["worst"],
                                      a["worst_pair"], a["n_bad"], null)
    for bad in (dict(pos=null), dict(worst=null), dict(worst_pair=null), dict(n_bad=null), dict(pairs=null), dict(lo=null), dict(hi=null),
                dict(G=-1), dict(K=-1), dict(n=-2), dict(n=0)):
        assert bounds(**bad) == -1, bad
    assert bounds(G=0) == 0 and bounds(G=0, dist=p) == 0
    assert bounds(G=0, K=0, pairs=null, lo=null, hi=null) == 0

    ok = dict(pos=p, radius=p, ex_ptr=p, ex_idx=p, G=2, n=5, thresh=0.6, scratch=p, min_ratio=p, min_pair=p, n_clash=p)

    def clash(**kw):
        a = dict(ok, **kw)
        return lib.agdiff_clash_scan(a["pos"], a["radius"], a["ex_ptr"], a["ex_idx"], a["G"], a["n"], a["thresh"], a["scratch"],
                                     a["min_ratio"], a["min_pair"], a["n_clash"], null)
    for bad in (dict(pos=null), dict(radius=null), dict(ex_ptr=null), dict(scratch=null), dict(min_ratio=null), dict(min_pair=null),
                dict(n_clash=null), dict(G=-1), dict(n=-1), dict(n=0), dict(thresh=float("nan")), dict(thresh=-0.1),
                dict(thresh=float("inf")), dict(G=0, thresh=float("nan")), dict(G=0, n=0)):
        assert clash(**bad) == -1, bad
    big = _lib.DEFINES["AGDIFF_MAX_ATOMS_LARGE"] + 1
    assert big == 16385 and clash(n=big) == -2 and clash(n=big, G=0) == -2
    assert clash(G=0) == 0 and clash(G=0, ex_idx=null) == 0 and clash(G=0, n=big - 1, thresh=0.0) == 0
    del keep


def test_exclusions_of_small_graphs():
    from agdiff_amd.validity import _check_exclusions, exclusions
    # ethane: C0 - C1, hydrogens 2 3 4 on C0 and 5 6 7 on C1; raw bonds extended to order 3 reach every pair (H - C - C - H)
    bonds = [(0, 1, 1)] + [(0, h, 1) for h in (2, 3, 4)] + [(1, h, 1) for h in (5, 6, 7)]
    raw = VR.graph([6, 6] + [1] * 6, bonds, order=1)
    ptr, idx = exclusions(8, raw[1], raw[2])
    assert ptr.dtype == idx.dtype == np.int32
    assert _rows(ptr, idx) == [[1, 2, 3, 4], [0, 5, 6, 7], [0], [0], [0], [1], [1], [1]]
    ext = VR.graph([6, 6] + [1] * 6, bonds)
    assert sorted(set(ext[2].tolist())) == [1, 23, 24]
    ptr, idx = exclusions(8, ext[1], ext[2])
    assert _rows(ptr, idx) == [[j for j in range(8) if j != i] for i in range(8)]
    # methane excludes every pair; so does the 40-neighbour star (everything is within two bonds)
    for mol, n in ((VR.graph([6, 1, 1, 1, 1], [(0, h, 1) for h in range(1, 5)]), 5), (VR.star(40), 41)):
        ptr, idx = exclusions(n, mol[1], mol[2])
        rows = _rows(ptr, idx)
        assert rows == [[j for j in range(n) if j != i] for i in range(n)]
        _check_exclusions(n, ptr, idx)
    # the star's raw bonds: a row of 40, sorted; symmetric; no self entries; duplicates and zero-typed entries change nothing
    raw = VR.graph([6] * 41, [(0, a, 1) for a in range(40, 0, -1)], order=1)
    ei = np.concatenate([raw[1], raw[1][:, :7], np.array([[3, 5], [9, 9]]).T], axis=1)
    et = np.concatenate([raw[2], raw[2][:7], [0, 1]])
    ptr, idx = exclusions(41, ei, et)
    rows = _rows(ptr, idx)
    assert rows[0] == list(range(1, 41)) and all(r == [0] for r in rows[1:])
    for i, r in enumerate(rows):
        assert r == sorted(set(r)) and i not in r and all(i in rows[j] for j in r)
    # a random chain: the same three properties, and the pairs are exactly those within three bonds
    (at, ei, et), _ = VR.random_chain(np.random.default_rng(5), 37)
    ptr, idx = exclusions(37, ei, et)
    _check_exclusions(37, ptr, idx)
    assert VR.excluded_set(ptr, idx) == {(int(a), int(b)) for a, b in ei.T}
    with pytest.raises(ValueError, match="outside"):
        exclusions(3, np.array([[0, 3], [3, 0]]), np.array([1, 1]))


def test_bounds_from_table_values_and_order():
    from agdiff_amd.validity import bounds_from_table
    # H3C - C(=O) - C#N with an iodine and an unknown element (Se) on the methyl carbon; bonds listed out of order
    atoms = [6, 6, 8, 6, 7, 53, 34, 1]
    bonds = [(3, 4, 3), (1, 2, 2), (0, 1, 1), (1, 3, 1), (0, 7, 1), (0, 5, 1), (0, 6, 1)]
    pairs, lo, hi = bounds_from_table(_item(VR.graph(atoms, bonds)))
    assert pairs.dtype == np.int32 and lo.dtype == hi.dtype == np.float32
    assert pairs.tolist() == [[0, 1], [0, 5], [0, 6], [0, 7], [1, 2], [1, 3], [3, 4]]          # bonds only, i < j, (i, j) order
    sums = {(0, 1): 0.76 + 0.76, (0, 5): 0.76 + 1.39, (0, 6): 0.76 + 1.50, (0, 7): 0.76 + 0.31, (1, 2): 0.76 + 0.66, (1, 3): 1.52,
            (3, 4): 0.76 + 0.71}
    for (i, j), l, h in zip(pairs.tolist(), lo, hi):
        assert l == np.float32(0.72 * sums[(i, j)]) and h == np.float32(1.20 * sums[(i, j)])
    # the bond lengths the defaults are argued from lie inside: C-H 1.09, C=O 1.21, C#N 1.16, C-I 2.14, C-C 1.53
    for (i, j), d in {(0, 7): 1.09, (1, 2): 1.21, (3, 4): 1.16, (0, 5): 2.14, (0, 1): 1.53}.items():
        k = pairs.tolist().index([i, j])
        assert lo[k] < d < hi[k]
    pairs, lo, hi = bounds_from_table(_item(VR.graph(atoms, bonds)), bond_lo=0.5, bond_hi=2.0)
    assert lo[0] == np.float32(0.5 * 1.52) and hi[0] == np.float32(2.0 * 1.52)
    with pytest.raises(ValueError, match="bond_lo"):
        bounds_from_table(_item(VR.graph(atoms, bonds)), bond_lo=1.3)
    with pytest.raises(ValueError, match="bonds"):
        bounds_from_table(dict(atom_type=np.array(atoms)))


def test_bounds_from_references_cover_bonds_and_two_hop_pairs_only():
    from agdiff_amd.validity import bounds_from_references
    mol = VR.graph([6] * 5, [(i, i + 1, 1) for i in range(4)])
    refs = np.stack([VR.backbone(5, [a] * 3, [t, -t]) for a, t in ((1.9, 3.0), (1.95, 1.1), (2.0, -1.0))])
    pairs, lo, hi = bounds_from_references(_item(mol, pos_ref=refs), slack=0.05)
    assert pairs.tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3], [2, 4], [3, 4]]          # no (0, 3), (1, 4): three hops
    assert (lo < hi).all() and lo.dtype == hi.dtype == np.float32
    d = np.linalg.norm(refs[:, pairs[:, 0]] - refs[:, pairs[:, 1]], axis=-1)
    assert np.array_equal(lo, (0.95 * d.min(0)).astype(np.float32)) and np.array_equal(hi, (1.05 * d.max(0)).astype(np.float32))
    k = pairs.tolist().index([0, 2])
    assert hi[k] - lo[k] > 0.1 * 2 * 1.53 * np.sin(0.95)                                        # the bond angle moved between them
    assert np.allclose(lo[0], 0.95 * 1.53) and np.allclose(hi[0], 1.05 * 1.53)
    with pytest.raises(ValueError, match="pos_ref"):
        bounds_from_references(_item(mol))
    with pytest.raises(ValueError, match="slack"):
        bounds_from_references(_item(mol, pos_ref=refs), slack=1.0)


def test_wrapper_checks_come_before_any_launch():
    import torch
    from agdiff_amd import validity as V
    from agdiff_amd.ensemble import prune_conformers
    pos = torch.zeros((2, 3, 3))
    ptr, idx = np.array([0, 1, 2, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    with pytest.raises(ValueError, match="on the GPU"):
        V.pair_bounds(pos, np.zeros((0, 2), np.int32), [], [])
    with pytest.raises(ValueError, match="on the GPU"):
        V.clash_scan(pos, np.ones(3), ptr, idx, 0.6)
    with pytest.raises(ValueError, match="on the GPU"):
        V.pair_bounds(pos.double(), np.zeros((0, 2), np.int32), [], [])
    with pytest.raises(ValueError, match="on the GPU"):
        V.clash_scan(pos.numpy(), np.ones(3), ptr, idx, 0.6)
    mol = VR.graph([6] * 4, [(0, 1, 1), (1, 2, 1), (2, 3, 1)])
    with pytest.raises(ValueError, match="bonds"):
        V.check_geometry(dict(atom_type=mol[0], pos_gen=np.zeros((2, 4, 3))), device="cpu")
    with pytest.raises(ValueError, match="bounds"):
        V.check_geometry(_item(mol, pos_gen=np.zeros((2, 4, 3))), bounds="rdkit", device="cpu")
    with pytest.raises(ValueError, match="pos_ref"):
        V.check_geometry(_item(mol, pos_gen=np.zeros((2, 4, 3))), bounds="references", device="cpu")
    # the exclusion table is checked on the host: an unsorted row, a one-sided entry, a self entry, an entry out of range
    for bad_ptr, bad_idx, what in (([0, 2, 3, 4], [2, 1, 0, 0], "ascending"), ([0, 1, 1, 1], [1], "symmetric"),
                                   ([0, 1, 1, 1], [0], "self"), ([0, 1, 1, 1], [3], "outside"), ([0, 1, 2], [1, 0], "n \\+ 1"),
                                   ([0, 1, 2, 3], [1, 0], "end at")):
        with pytest.raises(ValueError, match=what):
            V._check_exclusions(3, np.array(bad_ptr, dtype=np.int32), np.array(bad_idx, dtype=np.int32))
    with pytest.raises(ValueError, match="int32"):
        V._check_exclusions(3, ptr.astype(np.int64), idx)
    V._check_exclusions(3, ptr, idx)
    # the prune's mask
    item = dict(atom_type=np.array([6, 6]), pos_gen=np.zeros((3, 2, 3)))
    for bad in (np.ones(2, dtype=bool), np.ones(3, dtype=np.int8), torch.ones(3), np.ones((3, 1), dtype=bool)):
        with pytest.raises(ValueError, match="valid"):
            prune_conformers(item, 0.1, valid=bad, device="cpu")


def test_command_lines_accept_the_new_switches(tmp_path):
    from agdiff_amd import driver, ensemble, validity
    missing = str(tmp_path / "none.npz")
    # (argument parsing only: each main gets past its parser and fails on the first file it opens)
    with pytest.raises(FileNotFoundError):
        ensemble.main(["--samples", missing, "--testset", missing, "--prune-rms", "0.5", "--drop-invalid", "--out", str(tmp_path / "o.npz")])
    with pytest.raises(FileNotFoundError):
        validity.main(["--samples", missing, "--testset", missing, "--clash", "0.55", "--refs", missing, "--out", str(tmp_path / "o.npz")])
    with pytest.raises(SystemExit) as e:
        validity.main(["--samples", missing, "--testset", missing, "--clash", "-1", "--out", str(tmp_path / "o.npz")])
    assert e.value.code == 2
    import argparse
    seen = {}
    real = argparse.ArgumentParser.parse_args

    def spy(self, argv=None, namespace=None):
        seen["args"] = real(self, argv, namespace)
        raise KeyboardInterrupt                        # (stop driver.main right after its parser: no checkpoint, no GPU)
    argparse.ArgumentParser.parse_args = spy
    try:
        for extra, want in (([], False), (["--check-geometry"], True)):
            with pytest.raises(KeyboardInterrupt):
                driver.main(["--ckpt", missing, "--testset", missing, "--out", str(tmp_path)] + extra)
            assert seen["args"].check_geometry is want
    finally:
        argparse.ArgumentParser.parse_args = real
    assert not (tmp_path / "o.npz").exists()


def test_run_job_and_prune_signatures_keep_their_positional_order():
    import inspect
    from agdiff_amd import driver, ensemble, postprocess
    for fn, name in ((driver.run_job, "check_geometry"), (ensemble.prune_conformers, "valid")):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == name and params[-1].default in (False, None)
    assert any("check_geometry" in step.switches for step in postprocess.STEPS)


def test_reference_on_pinned_cases():
    two = np.array([[[0.0, 0.0, 0.0], [0.6, 0.0, 0.8]]], dtype=np.float32)          # 1.0 apart (to rounding: 0.36 + 0.64)
    r, pair, cnt, vals = VR.clash_scan(two, [1.0, 1.0], set(), 0.6)
    assert abs(float(r[0]) - 0.5) < 1e-7 and pair.tolist() == [[0, 1]] and cnt.tolist() == [1]
    assert VR.clash_scan(two, [1.0, 1.0], set(), 0.5 - 1e-6)[2].tolist() == [0]
    r, pair, cnt, _ = VR.clash_scan(two, [1.0, 1.0], {(0, 1), (1, 0)}, 0.6)
    assert np.isposinf(r[0]) and pair.tolist() == [[-1, -1]] and cnt.tolist() == [0]
    bad = two.copy()
    bad[0, 1, 2] = np.nan
    r, pair, cnt, _ = VR.clash_scan(bad, [1.0, 1.0], set(), 0.6)
    assert r[0] == 0.0 and pair.tolist() == [[0, 1]] and cnt.tolist() == [1]
    dist, v, worst, wp, nbad = VR.pair_bounds(bad, [[0, 1]], [0.9], [1.1])
    assert np.isnan(dist[0, 0]) and np.isposinf(worst[0]) and wp.tolist() == [0] and nbad.tolist() == [1]
    bad[0, 1, 2] = np.inf
    assert VR.clash_scan(bad, [1.0, 1.0], set(), 0.6)[0][0] == 0.0 and np.isposinf(VR.pair_bounds(bad, [[0, 1]], [0.9], [1.1])[2][0])
    # bounds: inside, too short, too long, an atom outside the molecule; ties take the lowest index; K = 0
    p = np.array([[[0, 0, 0], [3, 0, 0], [3, 4, 0]]], dtype=np.float32)
    dist, v, worst, wp, nbad = VR.pair_bounds(p, [[0, 1], [1, 2], [0, 2], [0, 2], [0, 3]], [2, 5, 1, 1, 0], [4, 6, 3, 3, 9])
    assert dist[0, :4].tolist() == [3.0, 4.0, 5.0, 5.0] and np.isnan(dist[0, 4])
    assert v[0].tolist() == [0.0, 1.0, 2.0, 2.0, np.inf] and wp.tolist() == [4] and nbad.tolist() == [4]
    assert VR.pair_bounds(p, [[0, 1], [1, 2], [0, 2], [0, 2]], [2, 5, 1, 1], [4, 6, 3, 3])[3].tolist() == [2]
    _, _, worst, wp, nbad = VR.pair_bounds(p, np.zeros((0, 2)), [], [])
    assert worst.tolist() == [0.0] and wp.tolist() == [-1] and nbad.tolist() == [0]
    # the clash minimum's tie rule: (0, 2) and (1, 2) are both 4 apart... (0, 1) at 3 wins; with it excluded the lowest (i, j) of the tie
    q = np.array([[[0, 0, 0], [0, 0, 0], [4, 0, 0]]], dtype=np.float32)
    assert VR.clash_scan(q, [1, 1, 1], {(0, 1), (1, 0)}, 0.1)[1].tolist() == [[0, 2]]


def test_hand_built_alkanes_under_the_defaults():
    """the molecules of the GPU test, through the reference alone: the ideal chains pass, a stretched C-H is the one bad pair, folded
    butane (ends three bonds apart: excluded) passes, folded pentane (four bonds apart) clashes at C1 ... C5"""
    from agdiff_amd.validity import bounds_from_table, exclusions, vdw_radii

    def judge(mol, pos):
        pairs, lo, hi = bounds_from_table(_item(mol))
        _, _, worst, wp, nbad = VR.pair_bounds(pos.astype(np.float32)[None], pairs, lo, hi)
        ex = VR.excluded_set(*exclusions(len(mol[0]), mol[1], mol[2]))
        r, pair, cnt, _ = VR.clash_scan(pos.astype(np.float32)[None], vdw_radii(mol[0]), ex, 0.6)
        return int(nbad[0]), pairs[wp[0]].tolist(), int(cnt[0]), pair[0].tolist(), float(r[0])
    mol, pos = VR.alkane(4)
    assert judge(mol, pos)[0] == 0 and judge(mol, pos)[2] == 0
    stretched = pos.copy()
    stretched[5] = pos[0] + (pos[5] - pos[0]) * (1.8 / 1.09)
    assert judge(mol, stretched)[:3] == (1, [0, 5], 0)
    mol, pos = VR.folded_butane(1.9)
    assert abs(np.linalg.norm(pos[0] - pos[3]) - 1.9) < 1e-9 and judge(mol, pos)[0] == 0 and judge(mol, pos)[2] == 0
    mol, pos = VR.folded_pentane(1.9)
    nbad, _, cnt, pair, r = judge(mol, pos)
    assert abs(np.linalg.norm(pos[0] - pos[4]) - 1.9) < 1e-9 and nbad == 0 and cnt >= 1 and pair == [0, 4] and abs(r - 1.9 / 3.4) < 1e-6
