"""No GPU: the host side of the geometry repair (agdiff_amd/validity.py: bounds_csr, relax_tables), the C ABI of agdiff_relax_bounds
as the header declares it and its host-side argument checks (every one returns before any launch), the switches of the command lines,
and the float64 restatement of the rule (tests/relax_ref.py) on hand-built molecules: what it repairs, in how many updates.  The
counts are what the restatement gives for these inputs on the CPU (table bounds, pad 0.02, at most 200 updates); the kernel is not
asked here."""
import ctypes
import inspect

import numpy as np
import pytest

import relax_ref as RR
import validity_ref as VR
from agdiff_amd import _lib

VP, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float


def test_export_defines_and_abi_version():
    assert _lib.EXPORTS["agdiff_relax_bounds"] == [VP] * 8 + [I32] * 3 + [F32] * 3 + [I32] + [VP] * 6
    assert _lib.DEFINES["AGDIFF_RELAX_MAX_ATOMS"] == 1024 and _lib.DEFINES["AGDIFF_RELAX_MAX_ITERS"] == 10000
    assert _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    lib = _lib.load()
    assert lib.agdiff_abi_version() == 48
    assert hasattr(lib, "agdiff_relax_bounds") and list(lib.agdiff_relax_bounds.argtypes) == _lib.EXPORTS["agdiff_relax_bounds"]


def test_the_entry_point_checks_its_arguments_on_the_host():
    lib = _lib.load()
    keep, other = (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)()
    p, q, null = ctypes.c_void_p(ctypes.addressof(keep)), ctypes.c_void_p(ctypes.addressof(other)), ctypes.c_void_p(0)
    names = ("pos", "bd_ptr", "bd_idx", "bd_lo", "bd_hi", "radius", "ex_ptr", "ex_idx", "G", "n", "K", "clash", "pad", "omega", "max_iter",
             "pos_out", "status", "iters", "resid", "moved")
    ok = dict(dict.fromkeys(names, p), G=2, n=5, K=3, clash=0.6, pad=0.02, omega=1.0, max_iter=200, pos_out=q)

    def relax(**kw):
        a = dict(ok, **kw)
        return lib.agdiff_relax_bounds(*[a[k] for k in names], null)
    nan, inf = float("nan"), float("inf")
    for bad in ([{k: null} for k in ("pos", "bd_ptr", "bd_idx", "bd_lo", "bd_hi", "radius", "ex_ptr", "pos_out", "status", "iters", "resid",
                                     "moved")]
                + [dict(pos_out=p), dict(G=-1), dict(n=0), dict(n=-3), dict(K=-1), dict(max_iter=0), dict(max_iter=-1),
                   dict(max_iter=10001), dict(pad=0.0), dict(pad=-0.02), dict(pad=nan), dict(pad=inf), dict(omega=0.0), dict(omega=2.0),
                   dict(omega=-1.0), dict(omega=nan), dict(clash=-0.1), dict(clash=nan), dict(clash=inf), dict(G=0, max_iter=0),
                   dict(G=0, pad=nan)]):
        assert relax(**bad) == -1, bad
    big = _lib.DEFINES["AGDIFF_RELAX_MAX_ATOMS"] + 1
    assert relax(n=big) == -2 and relax(n=big, G=0) == -2 and relax(n=big, max_iter=0) == -1
    # G = 0 returns at once; K = 0 goes with null bound tables, and ex_idx may be null
    assert relax(G=0) == 0 and relax(G=0, n=big - 1, max_iter=10000, clash=0.0, omega=1.999) == 0
    assert relax(G=0, K=0, bd_idx=null, bd_lo=null, bd_hi=null, ex_idx=null) == 0
    del keep, other


def test_bounds_csr_rows_keep_the_order_of_the_pair_list():
    from agdiff_amd.validity import bounds_csr
    ptr, idx, lo, hi = bounds_csr(4, np.zeros((0, 2), np.int32), [], [])
    assert ptr.tolist() == [0] * 5 and idx.shape == lo.shape == hi.shape == (0,)
    assert ptr.dtype == idx.dtype == np.int32 and lo.dtype == hi.dtype == np.float32
    # pairs out of (i, j) order, one of them listed twice (with other bounds), one written backwards
    pairs = [[2, 3], [0, 2], [3, 1], [0, 2], [0, 1]]
    ptr, idx, lo, hi = bounds_csr(5, pairs, [1, 2, 3, 4, 5], [11, 12, 13, 14, 15])
    rows = [list(zip(idx[ptr[i]:ptr[i + 1]].tolist(), lo[ptr[i]:ptr[i + 1]].tolist(), hi[ptr[i]:ptr[i + 1]].tolist())) for i in range(5)]
    assert rows == [[(2, 2.0, 12.0), (2, 4.0, 14.0), (1, 5.0, 15.0)], [(3, 3.0, 13.0), (0, 5.0, 15.0)],
                    [(3, 1.0, 11.0), (0, 2.0, 12.0), (0, 4.0, 14.0)], [(2, 1.0, 11.0), (1, 3.0, 13.0)], []]
    assert ptr.tolist() == [0, 3, 5, 8, 10, 10]
    # a molecule's table bounds: b_i is the atom's number of bonds
    mol, _ = VR.alkane(4)
    tab = RR.tables(mol)
    ptr = bounds_csr(14, *tab[:3])[0]
    assert np.diff(ptr).tolist() == [4] * 4 + [1] * 10


def test_relax_tables_refuse_bad_input_before_any_launch():
    import torch
    from agdiff_amd import validity as V
    mol, _ = VR.alkane(4)
    pairs, lo, hi, radius, ex_ptr, ex_idx = RR.tables(mol)
    good = lambda **kw: V.relax_tables(14, **dict(dict(pairs=pairs, lo=lo, hi=hi, radius=radius, ex_ptr=ex_ptr, ex_idx=ex_idx), **kw))
    out = good()
    assert len(out) == 8 and out[7] == 13 and out[1].shape == (26,)
    swapped = lo.copy()
    swapped[3] = hi[3] + 1
    far, twice = pairs.copy(), pairs.copy()
    far[2, 1], twice[2] = 14, (5, 5)
    nan_lo = lo.copy()
    nan_lo[0] = np.nan
    for kw, what in ((dict(lo=swapped), "lo <= hi"), (dict(lo=nan_lo), "lo <= hi"), (dict(pairs=far), "outside"), (dict(pairs=twice), "twice"),
                     (dict(pairs=-pairs - 1), "outside"), (dict(lo=lo[:-1]), "13 pairs but 12"), (dict(pad=0.0), "pad"), (dict(pad=-0.01), "pad"),
                     (dict(pad=float("nan")), "pad"), (dict(pad=float("inf")), "pad"), (dict(omega=0.0), "omega"), (dict(omega=2.0), "omega"),
                     (dict(omega=float("nan")), "omega"), (dict(clash=-0.1), "clash"), (dict(clash=float("inf")), "clash"),
                     (dict(radius=radius[:-1]), "radius"), (dict(radius=-radius), "radius"),
                     (dict(ex_idx=ex_idx[::-1].copy()), "ascending|symmetric|self"), (dict(ex_ptr=ex_ptr[:-1]), "n \\+ 1"),
                     (dict(ex_ptr=ex_ptr.astype(np.int64)), "int32")):
        with pytest.raises(ValueError, match=what):
            good(**kw)
    one_sided = (np.array([0, 1] + [1] * 13, dtype=np.int32), np.array([1], dtype=np.int32))
    with pytest.raises(ValueError, match="symmetric"):
        good(ex_ptr=one_sided[0], ex_idx=one_sided[1])
    with pytest.raises(ValueError, match="on the GPU"):
        V.relax_bounds(torch.zeros((2, 14, 3)), pairs, lo, hi, radius, ex_ptr, ex_idx)
    item = dict(atom_type=mol[0], edge_index=mol[1], edge_type=mol[2], pos_gen=np.zeros((2, 14, 3)))
    with pytest.raises(ValueError, match="bounds"):
        V.repair_geometry(item, bounds="mmff", device="cpu")
    with pytest.raises(ValueError, match="pos_ref"):
        V.repair_geometry(item, bounds="references", device="cpu")
    # not MMFF: the evaluator's switch still refuses
    from agdiff_amd import evaluation
    assert "NotImplementedError" in inspect.getsource(evaluation) and "use_force_field" in inspect.getsource(evaluation)


def test_signatures_and_command_line_switches(tmp_path):
    import argparse
    from agdiff_amd import driver, postprocess, validity
    assert inspect.signature(driver.run_job).parameters["repair_geometry"].default is False
    assert any("repair_geometry" in step.switches for step in postprocess.STEPS)
    sig = inspect.signature(validity.relax_bounds).parameters
    assert list(sig) == ["pos", "pairs", "lo", "hi", "radius", "ex_ptr", "ex_idx", "clash", "pad", "omega", "max_iter"]
    assert [sig[k].default for k in ("clash", "pad", "omega", "max_iter")] == [0.60, 0.02, 1.0, 200]
    sig = inspect.signature(validity.repair_geometry).parameters
    assert list(sig) == ["item", "bounds", "clash", "pad", "omega", "max_iter", "device", "table_kw"]
    assert [sig[k].default for k in ("bounds", "clash", "pad", "omega", "max_iter", "device")] == ["table", 0.60, 0.02, 1.0, 200, "cuda"]
    missing = str(tmp_path / "none.npz")
    base = ["--samples", missing, "--testset", missing, "--out", str(tmp_path / "o.npz"), "--repair", str(tmp_path / "r.npz")]
    with pytest.raises(FileNotFoundError):            # (past the parser: fails on the first file it opens)
        validity.main(base + ["--pad", "0.03", "--omega", "1.5", "--max-iter", "50", "--refs", missing])
    for bad in (["--pad", "0"], ["--omega", "2"], ["--max-iter", "0"]):
        with pytest.raises(SystemExit) as e:
            validity.main(base + bad)
        assert e.value.code == 2
    seen = {}
    real = argparse.ArgumentParser.parse_args

    def spy(self, argv=None, namespace=None):
        seen["args"] = real(self, argv, namespace)
        raise KeyboardInterrupt                        # (stop driver.main right after its parser: no checkpoint, no GPU)
    argparse.ArgumentParser.parse_args = spy
    try:
        for extra, want in (([], False), (["--repair-geometry"], True)):
            with pytest.raises(KeyboardInterrupt):
                driver.main(["--ckpt", missing, "--testset", missing, "--out", str(tmp_path)] + extra)
            assert seen["args"].repair_geometry is want and seen["args"].check_geometry is False
    finally:
        argparse.ArgumentParser.parse_args = real
    assert not (tmp_path / "o.npz").exists() and not (tmp_path / "r.npz").exists()


def _judge(inputs, pos):
    """(n_bad, n_clash) per conformer by the float64 restatement of the two CHECKS (validity_ref), at the true bounds"""
    _, pairs, lo, hi, radius, ex_ptr, ex_idx = inputs
    nbad = VR.pair_bounds(pos, pairs, lo, hi)[4]
    ncl = VR.clash_scan(pos, radius, VR.excluded_set(ex_ptr, ex_idx), RR.CLASH)[2]
    return nbad.tolist(), ncl.tolist()


# (case, omega) -> (status, iters) per conformer
PINNED = {
    ("hexane", 1.0): ([0], [0]),
    ("hexane_shifted", 1.0): ([1], [20]),
    ("hexane_short_ch", 1.0): ([1], [9]),
    ("butane_folded", 1.0): ([0], [0]),
    ("pentane_folded_1.9", 1.0): ([1], [13]),
    ("pentane_folded_1.2", 1.0): ([1], [15]),
    ("star40", 1.0): ([1, 1, 1], [15, 15, 15]),
    ("tree23", 1.0): ([1, 1, 1, 1], [58, 25, 34, 40]),
    ("tree61", 1.0): ([1, 1, 2], [152, 168, 200]),
    ("tree130", 1.0): ([2, 1], [200, 169]),
    ("tree130", 1.5): ([1, 1], [142, 113]),
    ("pentane_refs", 1.0): ([1], [96]),
}


@pytest.mark.parametrize("key,omega", sorted(PINNED))
def test_the_reference_repairs_what_it_should(key, omega):
    inputs, fwd, rev = RR.solved(key, omega=omega)
    status, iters = PINNED[(key, omega)]
    assert fwd["status"].tolist() == status and fwd["iters"].tolist() == iters
    assert rev["status"].tolist() == status and rev["iters"].tolist() == iters
    pos = inputs[0]
    before, after = _judge(inputs, pos), _judge(inputs, fwd["pos"])
    for g, st in enumerate(status):
        broken = before[0][g] > 0 or before[1][g] > 0
        assert broken == (st != 0)
        if st == 0:
            assert np.array_equal(fwd["pos"][g], pos[g]) and fwd["resid"][g] == 0.0 and fwd["moved"][g] == 0.0
        if st == 1:                                    # repaired: the fp32 result passes both checks, and little was moved
            assert after[0][g] == 0 and after[1][g] == 0 and fwd["resid"][g] <= RR.PAD / 2 and 0.0 < fwd["moved"][g] < 1.0
        if st == 2:
            assert fwd["iters"][g] == RR.MAX_ITER and fwd["resid"][g] > RR.PAD / 2
    # the two summation orders differ by accumulated float64 rounding only
    assert np.abs(fwd["pos64"] - rev["pos64"]).max() < 1e-12


def test_the_folded_pentane_is_pushed_apart_just_past_the_threshold():
    inputs, fwd, _ = RR.solved("pentane_folded_1.9")
    ratio = lambda p: np.linalg.norm(p[0, 0].astype(np.float64) - p[0, 4]) / 3.4
    assert abs(ratio(inputs[0]) - 0.559) < 1e-3 and abs(ratio(fwd["pos"]) - 0.603) < 1e-3
    # a narrower interval than 2 pad: p_k = (hi - lo) / 2, the target is the midpoint, and the stop rule tightens with it
    _, pairs, lo, hi, radius, ex_ptr, ex_idx = inputs
    mid = ((lo.astype(np.float64) + hi) / 2).astype(np.float32)
    res = RR.relax(inputs[0], pairs, mid - np.float32(0.005), mid + np.float32(0.005), radius, ex_ptr, ex_idx)
    assert res["status"].tolist() == [1] and res["resid"][0] <= 0.0025 + 1e-7
    d = VR.distances(res["pos"], pairs)[0]
    assert (np.abs(d - mid) <= 0.0026).all()


def test_coincident_atoms_part_along_x_with_the_lower_index_towards_plus_x():
    # two bonded atoms on one point, bounds [1, 3] and pad 0.5: the target interval is [1.5, 2.5], s = 1.5, each atom moves
    # omega / (1 + 1) x s / 2: the gap to 1.5 halves with every update, s = 1.5, 0.75, 0.375, 0.1875 <= p / 2 = 0.25 after three
    # updates, 1.3125 apart -- every number exact in binary
    pos = np.full((1, 2, 3), 2.0, dtype=np.float32)
    ptr, idx = np.array([0, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    res = RR.relax(pos, [[0, 1]], [1.0], [3.0], [1.0, 1.0], ptr, idx, pad=0.5)
    assert res["status"].tolist() == [1] and res["iters"].tolist() == [3] and res["resid"].tolist() == [0.1875]
    assert res["pos"].tolist() == [[[2.65625, 2.0, 2.0], [1.34375, 2.0, 2.0]]] and res["moved"].tolist() == [0.65625]
    back = RR.relax(pos, [[1, 0]], [1.0], [3.0], [1.0, 1.0], ptr, idx, pad=0.5)
    assert back["pos"].tolist() == res["pos"].tolist()
