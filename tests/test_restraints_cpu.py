"""CPU: host logic of the distance restraints (agdiff_amd/restraints.py, epsnet.LangevinRun's restraint_* keywords): the export
and its declaration, the refusals of the entry point and of the keyword checks, the test set's `restr_*_<i>` fields, packing and
the command line's defaults.  Nothing here computes on a GPU."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from agdiff_amd import _lib, driver, epsnet, restraints, synth, validity


def test_export_argtypes_and_header():
    lib = _lib.load()
    assert hasattr(lib, "agdiff_restrain_pairs")
    P, I, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    want = [P, P, P, P, P, P, P, P, I, I, I, I, F, I, P, P, P]
    assert _lib.EXPORTS["agdiff_restrain_pairs"] == want
    assert list(lib.agdiff_restrain_pairs.argtypes) == want and lib.agdiff_restrain_pairs.restype is ctypes.c_int
    src = open(_lib.HEADER).read()
    assert "int agdiff_restrain_pairs(float* pos /* [N][3], in place */, const int32_t* graph_ptr /* [G + 1] */" in src
    assert "x_a <- x_a + (w / c_a) sum s (-e) (x_a - x_b) / d" in src                     # the rule is stated in the header
    assert _lib.DEFINES["AGDIFF_RESTRAIN_MAX_ATOMS"] >= 129
    # a pure addition: the ABI version and the struct layouts are what they were
    assert lib.agdiff_abi_version() == _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    assert [name for name, _ in _lib.StepArgs._fields_] == ["pos_in", "pos_out", "scratch", "noise", "traj_out", "sigma", "step_size",
                                                            "noise_scale", "w_global", "clip", "clip_local", "clip_pos", "use_global"]
    assert ctypes.sizeof(_lib.StepArgs) == 72


def test_argument_errors_of_the_entry_point_need_no_gpu():
    lib = _lib.load()
    bufs = [(ctypes.c_float * 64)() for _ in range(7)]
    p, gp, rp, ri, rl, rh, other = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
    null = ctypes.c_void_p(0)
    cap = _lib.DEFINES["AGDIFF_RESTRAIN_MAX_ATOMS"]

    def call(pos=p, graph_ptr=gp, rs_ptr=rp, rs_idx=ri, rs_lo=rl, rs_hi=rh, G=1, N=4, R2=2, most=2, w=1.0, sweeps=1, copy_out=null):
        return lib.agdiff_restrain_pairs(pos, graph_ptr, rs_ptr, rs_idx, rs_lo, rs_hi, null, null, G, N, R2, most, w, sweeps, copy_out,
                                         null, null)

    for bad in (dict(pos=null), dict(graph_ptr=null), dict(rs_ptr=null), dict(rs_idx=null), dict(rs_lo=null), dict(rs_hi=null),
                dict(G=-1), dict(N=0), dict(N=-3), dict(R2=-1), dict(most=-1), dict(sweeps=-1), dict(sweeps=17), dict(copy_out=p)):
        assert call(**bad) == -1, bad
    for w in (0.0, -0.5, 1.5, float("nan"), float("inf")):               # weight outside (0, 1]
        assert call(w=w) == -1, w
    assert call(most=cap + 1) == -2 and call(most=cap + 1, G=0) == -2    # AGDIFF_ERR_LIMIT, before any launch
    assert call(most=cap + 1, w=2.0) == -1                                # (a bad argument first)
    assert call(G=0) == 0 and call(G=0, most=cap, sweeps=0, w=0.5, copy_out=other) == 0     # nothing to do: no launch
    assert call(G=0, R2=0, rs_idx=null, rs_lo=null, rs_hi=null) == 0     # an empty table needs no arrays


def _batch():
    return np.repeat(np.arange(3), [4, 5, 3])                            # 12 atoms in three graphs


def test_restraint_arguments_value_errors():
    N, batch = 12, _batch()
    ok = dict(pairs=[[0, 3], [4, 8], [5, 4]], lo=[1.0, 0.0, 2.0], hi=[2.0, 3.0, np.inf])
    ra = lambda **kw: restraints.restraint_arguments(N, *(kw.pop(k, ok[k]) for k in ("pairs", "lo", "hi")), kw.pop("batch", batch), **kw)
    bad = [dict(lo=[1.0, 0.0]), dict(hi=[2.0, 3.0]), dict(lo=None), dict(hi=None),                 # bounds of another length, or none
           dict(pairs=[[0, 3, 1]], lo=[1.0], hi=[2.0]), dict(pairs=[0, 3, 4], lo=[1.0], hi=[2.0]),      # not [R, 2]
           dict(pairs=[[0.5, 3.0]], lo=[1.0], hi=[2.0]),                                                 # not indices
           dict(lo=[-0.1, 0.0, 2.0]), dict(lo=[3.0, 0.0, 2.0]), dict(lo=[1.0, np.nan, 2.0]), dict(hi=[2.0, np.nan, np.inf]),
           dict(lo=[1.0, 0.0, np.inf]),                                                                  # an infinite lower bound
           dict(pairs=[[0, 3], [4, 8], [5, 5]]), dict(pairs=[[0, 3], [4, 8], [5, 12]]), dict(pairs=[[0, -1], [4, 8], [5, 4]]),
           dict(pairs=[[0, 4], [4, 8], [5, 4]]),                                                         # across two graphs
           dict(batch=None), dict(batch=batch[:-1]),
           dict(weight=0.0), dict(weight=1.0001), dict(weight=-1.0), dict(weight=float("nan")),
           dict(start_sigma=float("nan")), dict(sweeps=-1), dict(sweeps=17), dict(sweeps=1.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            ra(**dict(kw))
    with pytest.raises(ValueError):
        restraints.restraint_arguments(N, None, [1.0], [2.0], batch)      # bounds without pairs
    assert restraints.restraint_arguments(N, None, None, None, batch) is None
    assert restraints.restraint_arguments(N, np.zeros((0, 2), dtype=np.int64), [], [], batch) is None
    assert restraints.restraint_arguments(N, [], [], [], None) is None
    rs_ptr, rs_idx, rs_lo, rs_hi, most, w, start, sweeps = ra(weight=0.25, start_sigma=0.7, sweeps=4)
    table = validity.bounds_csr(N, ok["pairs"], ok["lo"], ok["hi"])       # exactly that table
    for got, want in zip((rs_ptr, rs_idx, rs_lo, rs_hi), table):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert rs_ptr.dtype == np.int32 and rs_idx.dtype == np.int32 and rs_lo.dtype == np.float32 and rs_hi.dtype == np.float32
    assert rs_ptr.tolist() == [0, 1, 1, 1, 2, 4, 5, 5, 5, 6, 6, 6, 6] and rs_idx.tolist() == [3, 0, 8, 5, 4, 4]
    assert (most, w, start, sweeps) == (3, 0.25, 0.7, 4)                  # graph 1: atoms 4, 5 and 8
    assert ra(sweeps=0)[-1] == 0                                          # measuring is legal for the stand-alone launch
    # more restrained atoms in one graph than the kernel stages
    cap = _lib.DEFINES["AGDIFF_RESTRAIN_MAX_ATOMS"]
    big = np.zeros(cap + 2, dtype=np.int64)
    chain = np.stack([np.arange(cap + 1), np.arange(1, cap + 2)], axis=1)
    with pytest.raises(_lib.AgdiffLimitError):
        restraints.restraint_arguments(cap + 2, chain, np.zeros(cap + 1), np.ones(cap + 1), big)
    assert restraints.restraint_arguments(cap + 2, chain[:-2], np.zeros(cap - 1), np.ones(cap - 1), big)[4] == cap


def test_the_six_keywords_are_real_parameters():
    params = inspect.signature(epsnet.LangevinRun.__init__).parameters
    for name, default in (("restraint_pairs", None), ("restraint_lo", None), ("restraint_hi", None), ("restraint_weight", 1.0),
                          ("restraint_start_sigma", float("inf")), ("restraint_sweeps", 1)):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default
    assert restraints.SAMPLER_KEYWORDS == ("restraint_pairs", "restraint_lo", "restraint_hi", "restraint_weight", "restraint_start_sigma",
                                           "restraint_sweeps")


class _NoGpu:
    """A model on which touching the device is an error: the keyword checks come first."""

    def _device(self):
        raise AssertionError("the run reached the device")

    def _require_gpu(self):
        raise AssertionError("the run reached the device")


def test_sampler_keyword_checks():
    N, batch = 12, torch.from_numpy(_batch())
    at = torch.full((N,), 6)
    pairs, lo, hi = [[0, 3], [4, 8]], [1.0, 0.0], [2.0, 3.0]
    good = dict(restraint_pairs=pairs, restraint_lo=lo, restraint_hi=hi)
    bad = [dict(restraint_pairs=pairs), dict(restraint_pairs=pairs, restraint_lo=lo), dict(restraint_lo=lo, restraint_hi=hi),
           dict(good, restraint_lo=[1.0]), dict(good, restraint_lo=[3.0, 0.0]), dict(good, restraint_lo=[-1.0, 0.0]),
           dict(good, restraint_hi=[2.0, float("nan")]), dict(good, restraint_pairs=[[0, 3], [4, 4]]), dict(good, restraint_pairs=[[0, 3], [4, 12]]),
           dict(good, restraint_pairs=[[0, 3], [3, 4]]), dict(good, restraint_weight=0.0), dict(good, restraint_weight=1.5),
           dict(good, restraint_weight=float("nan")), dict(good, restraint_start_sigma=float("nan")), dict(good, restraint_sweeps=0),
           dict(good, restraint_sweeps=17), dict(good, restraint_sweeps=2.5), dict(restraint_sweeps=0), dict(restraint_weight=2.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            epsnet.LangevinRun(_NoGpu(), at, None, None, None, batch, 3, False, 2, 1e-6, 1000.0, None, None, 0.5, 1.0, **kw)
        with pytest.raises(ValueError):
            epsnet.DualEncoderEpsNetwork.begin_sampling(_NoGpu(), at, None, None, None, batch, 3, False, **kw)
    with pytest.raises(AssertionError, match="reached the device"):      # good keywords pass the checks and go on
        epsnet.DualEncoderEpsNetwork.begin_sampling(_NoGpu(), at, None, None, None, batch, 3, False, **good)


def _mols(k=3):
    rng = np.random.default_rng(11)
    out = []
    for i in range(k):
        n = int(rng.integers(6, 14))
        at, r, c, t = synth.random_molecule(rng, n)
        out.append(dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=t, num_refs=1 + i, name="m%d" % i, index=i))
    return out


def test_restraints_round_trip_through_the_testset(tmp_path):
    mols = _mols()
    plain, with_r = str(tmp_path / "t.npz"), str(tmp_path / "r.npz")
    driver.save_testset(plain, mols)
    n0, n2 = mols[0]["atom_type"].shape[0], mols[2]["atom_type"].shape[0]
    given = {0: ([[0, n0 - 1], [1, 2]], [1.0, 0.0], [2.0, np.inf]), 2: (np.array([[n2 - 1, 0]]), [3.0], [3.5])}
    restraints.add_restraints(plain, with_r, given)
    z = np.load(with_r)
    assert z["restr_pairs_0"].dtype == np.int32 and z["restr_pairs_0"].shape == (2, 2) and z["restr_lo_0"].dtype == np.float32
    assert z["restr_hi_2"].dtype == np.float32 and "restr_pairs_1" not in z.files
    back = restraints.load_restraints(with_r)
    assert sorted(back) == [0, 2] and restraints.load_restraints(plain) == {}
    for i, (pr, lo, hi) in given.items():
        assert np.array_equal(back[i][0], np.asarray(pr, dtype=np.int32)) and np.array_equal(back[i][1], np.asarray(lo, dtype=np.float32))
        assert np.array_equal(back[i][2], np.asarray(hi, dtype=np.float32))
    # every other field is kept, and the driver's loader reads the file as before
    z0 = np.load(plain)
    assert all(np.array_equal(z[k], z0[k]) for k in z0.files)
    again = driver.load_testset(with_r)
    assert [m["name"] for m in again] == ["m0", "m1", "m2"] and np.array_equal(again[2]["atom_type"], mols[2]["atom_type"])
    for bad in ({3: ([[0, 1]], [0.0], [1.0])}, {1: ([[0, 99]], [0.0], [1.0])}, {1: ([[0, 1]], [2.0], [1.0])}, {1: ([[2, 2]], [0.0], [1.0])}):
        with pytest.raises(ValueError):
            restraints.add_restraints(plain, str(tmp_path / "bad.npz"), bad)


@pytest.mark.parametrize("spec", ["2x", "3"])
def test_pack_restraints_shifts_by_the_spans(spec):
    mols = _mols()
    confs = driver.num_confs(spec)
    packed = driver.pack_batch(mols, confs)
    n0, n2 = mols[0]["atom_type"].shape[0], mols[2]["atom_type"].shape[0]
    per = [([[0, n0 - 1], [1, 2]], [1.0, 0.0], [2.0, np.inf]), None, ([[n2 - 1, 0]], [3.0], [3.5])]
    pr, lo, hi = restraints.pack_restraints(packed, per)
    want_pr, want_lo, want_hi = [], [], []
    for r, (off, n, g) in zip(per, packed["spans"]):
        if r is None:
            continue
        for c in range(g):
            for (a, b), l, h in zip(*r):
                want_pr.append((off + c * n + a, off + c * n + b)); want_lo.append(l); want_hi.append(h)
    assert pr.dtype == np.int32 and lo.dtype == np.float32 and hi.dtype == np.float32
    assert pr.tolist() == [list(x) for x in want_pr] and lo.tolist() == want_lo and np.array_equal(hi, np.asarray(want_hi, dtype=np.float32))
    assert len(want_pr) == 2 * packed["spans"][0][2] + packed["spans"][2][2]
    # the packed pairs pass the sampler's checks on the packed batch: both atoms of every pair in one graph
    got = restraints.restraint_arguments(packed["atom_type"].shape[0], pr, lo, hi, packed["batch"])
    assert got[4] == 4 and got[1].shape[0] == 2 * len(want_pr)
    empty = restraints.pack_restraints(packed, [None, None, None])
    assert empty[0].shape == (0, 2) and restraints.restraint_arguments(packed["atom_type"].shape[0], *empty, packed["batch"]) is None
    with pytest.raises(ValueError):
        restraints.pack_restraints(packed, per[:2])
    with pytest.raises(ValueError):
        restraints.pack_restraints(packed, [([[0, n0]], [0.0], [1.0]), None, None])       # an atom outside its molecule


def test_parser_defaults():
    ap = restraints.build_parser()
    a = ap.parse_args(["--ckpt", "c.pt", "--testset", "t.npz", "--out", "o"])
    assert (a.num_confs, a.n_steps, a.w_global, a.global_start_sigma, a.clip) == ("2x", 5000, 1.0, 0.5, 1000.0)
    assert (a.weight, a.start_sigma, a.sweeps, a.seed, a.noise, a.precision) == (1.0, float("inf"), 1, 2021, "default", None)
    assert (a.start_idx, a.end_idx, a.trust_ckpt, a.report, a.samples) == (0, 200, False, False, None)
    r = ap.parse_args(["--report", "--samples", "s.npz", "--testset", "t.npz", "--out", "v.npz"])
    assert r.report and r.samples == "s.npz" and r.ckpt is None
    with pytest.raises(SystemExit):
        ap.parse_args(["--ckpt", "c.pt", "--testset", "t.npz", "--out", "o", "--noise", "other"])
