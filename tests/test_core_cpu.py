"""CPU: host logic of the rigid core hold (agdiff_amd/core.py, epsnet.LangevinRun's core_* keywords, driver --hold-core): the
export and its declaration, the test set's `core_pos_<i>` / `core_mask_<i>`, packing, and the refusals.  Nothing here computes on
a GPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from agdiff_amd import _lib, core, driver, epsnet, synth


def test_export_argtypes_and_header():
    lib = _lib.load()
    assert hasattr(lib, "agdiff_hold_core")
    P, I, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    assert _lib.EXPORTS["agdiff_hold_core"] == [P, P, P, P, P, I, I, F, P, P, P]
    assert list(lib.agdiff_hold_core.argtypes) == _lib.EXPORTS["agdiff_hold_core"] and lib.agdiff_hold_core.restype is ctypes.c_int
    src = open(_lib.HEADER).read()
    assert "int agdiff_hold_core(float* pos /* [N][3], in place */, const float* core_pos /* [N][3] */" in src
    # a pure addition: the ABI version and the struct layouts are what they were
    assert lib.agdiff_abi_version() == _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    assert "core" not in " ".join(name for name, _ in _lib.StepArgs._fields_)


def test_argument_errors_of_the_entry_point_need_no_gpu():
    lib = _lib.load()
    buf, other, third = ((ctypes.c_float * 64)() for _ in range(3))
    p, q, r, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(other, ctypes.c_void_p), ctypes.cast(third, ctypes.c_void_p), ctypes.c_void_p(0)
    call = lambda *a: lib.agdiff_hold_core(*a)
    assert call(null, q, r, r, null, 1, 4, 1.0, null, null, null) == -1
    assert call(p, null, r, r, null, 1, 4, 1.0, null, null, null) == -1
    assert call(p, q, null, r, null, 1, 4, 1.0, null, null, null) == -1
    assert call(p, q, r, null, null, 1, 4, 1.0, null, null, null) == -1
    assert call(p, q, r, r, null, -1, 4, 1.0, null, null, null) == -1
    assert call(p, q, r, r, null, 1, 0, 1.0, null, null, null) == -1
    for w in (0.0, -0.5, 1.5, float("nan"), float("inf")):               # weight outside (0, 1]
        assert call(p, q, r, r, null, 1, 4, w, null, null, null) == -1
    assert call(p, q, r, r, null, 1, 4, 1.0, p, null, null) == -1         # copy_out == pos
    assert call(p, p, r, r, null, 1, 4, 1.0, null, null, null) == -1      # core_pos == pos
    assert call(p, q, r, r, null, 0, 4, 0.5, null, null, null) == 0       # nothing to do: no launch


def test_the_four_keywords_are_real_parameters():
    params = inspect.signature(epsnet.LangevinRun.__init__).parameters
    for name, default in (("core_pos", None), ("core_select", None), ("core_weight", 1.0), ("core_start_sigma", float("inf"))):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default


class _NoGpu:
    """A model on which touching the device is an error: the keyword checks come first."""

    def _device(self):
        raise AssertionError("the run reached the device")

    def _require_gpu(self):
        raise AssertionError("the run reached the device")


def _bad_keywords(N):
    pos, sel = np.zeros((N, 3), dtype=np.float32), np.zeros(N, dtype=bool)
    return [dict(core_pos=pos),                                            # no selection
            dict(core_select=sel),                                         # no template
            dict(core_pos=pos[:-1], core_select=sel), dict(core_pos=np.zeros((N, 2), dtype=np.float32), core_select=sel),
            dict(core_pos=pos.reshape(-1), core_select=sel),
            dict(core_pos=pos, core_select=sel[:-1]), dict(core_pos=pos, core_select=np.zeros((N, 1), dtype=bool)),
            dict(core_pos=pos, core_select=sel, core_weight=0.0), dict(core_pos=pos, core_select=sel, core_weight=1.0001),
            dict(core_pos=pos, core_select=sel, core_weight=-1.0), dict(core_pos=pos, core_select=sel, core_weight=float("nan")),
            dict(core_pos=torch.zeros(N + 1, 3), core_select=torch.zeros(N, dtype=torch.bool))]


def test_sampler_keyword_checks():
    N = 7
    at = torch.full((N,), 6)
    for kw in _bad_keywords(N):
        with pytest.raises(ValueError):
            core.core_arguments(N, kw.get("core_pos"), kw.get("core_select"), kw.get("core_weight", 1.0))
        with pytest.raises(ValueError):
            epsnet.LangevinRun(_NoGpu(), at, None, None, None, None, 1, False, 2, 1e-6, 1000.0, None, None, 0.5, 1.0, **kw)
        with pytest.raises(ValueError):
            epsnet.DualEncoderEpsNetwork.begin_sampling(_NoGpu(), at, None, None, None, None, 1, False, **kw)
    assert core.core_arguments(N, None, None) is None
    pos, sel, w, start = core.core_arguments(N, torch.ones(N, 3, dtype=torch.float64), [0, 2, 0, 0, 1, 0, 0], 0.25, 0.7)
    assert pos.dtype == np.float32 and pos.shape == (N, 3) and sel.dtype == np.uint8 and sel.tolist() == [0, 1, 0, 0, 1, 0, 0]
    assert (w, start) == (0.25, 0.7)


def _mols(k=3, cores=(1,)):
    rng = np.random.default_rng(11)
    out = []
    for i in range(k):
        n = int(rng.integers(6, 14))
        at, r, c, t = synth.random_molecule(rng, n)
        m = dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=t, num_refs=1 + i, name="m%d" % i, index=i)
        if i in cores:
            m["core_pos"] = rng.normal(size=(n, 3)).astype(np.float32)
            m["core_mask"] = (np.arange(n) % 2 == 0)
        out.append(m)
    return out


def test_core_round_trips_through_the_testset(tmp_path):
    mols = _mols(cores=(0, 2))
    p = str(tmp_path / "t.npz")
    driver.save_testset(p, mols)
    z = np.load(p)
    assert z["core_pos_0"].dtype == np.float32 and z["core_mask_0"].dtype == np.uint8 and "core_pos_1" not in z.files
    back = driver.load_testset(p)
    assert back[1].get("core_pos") is None and back[1].get("core_mask") is None
    for k in (0, 2):
        assert back[k]["core_pos"].dtype == np.float32 and np.array_equal(back[k]["core_pos"], mols[k]["core_pos"])
        assert back[k]["core_mask"].dtype == np.uint8 and np.array_equal(back[k]["core_mask"] != 0, mols[k]["core_mask"])
    for spoil in ("short", "mask", "alone"):
        bad = _mols(1, cores=(0,))
        if spoil == "short":
            bad[0]["core_pos"] = bad[0]["core_pos"][:-1]
        elif spoil == "mask":
            bad[0]["core_mask"] = bad[0]["core_mask"][:-1]
        else:
            del bad[0]["core_mask"]
        with pytest.raises(ValueError):
            driver.save_testset(str(tmp_path / "bad.npz"), bad)


def test_pack_and_subset_carry_the_core():
    mols = _mols()
    confs = driver.num_confs("2x")
    packed = driver.pack_batch(mols, confs)
    cp, cs = packed["core_pos"], packed["core_select"]
    N = packed["atom_type"].shape[0]
    assert cp.dtype == np.float32 and cp.shape == (N, 3) and cs.dtype == np.uint8 and cs.shape == (N,)
    for k, (m, (off, n, g)) in enumerate(zip(mols, packed["spans"])):
        assert g == confs(m["num_refs"])
        for c in range(g):
            rows = slice(off + c * n, off + (c + 1) * n)
            if k == 1:
                assert np.array_equal(cp[rows], m["core_pos"]) and np.array_equal(cs[rows] != 0, m["core_mask"])
            else:                                                         # a molecule without a core: zeros, nothing selected
                assert not cp[rows].any() and not cs[rows].any()
    sub = driver.subset_batch(packed, [2, 1])
    ref = driver.pack_batch([mols[2], mols[1]], confs)
    assert np.array_equal(sub["core_pos"], ref["core_pos"]) and np.array_equal(sub["core_select"], ref["core_select"])
    assert np.array_equal(sub["atom_type"], ref["atom_type"])
    only = driver.subset_batch(packed, [0])
    assert only["core_select"].shape == (only["atom_type"].shape[0],) and not only["core_select"].any()
    # a batch without any core carries neither array, and what it carried before is unchanged
    plain = driver.pack_batch([{k: v for k, v in m.items() if not k.startswith("core_")} for m in mols], confs)
    assert "core_pos" not in plain and "core_select" not in plain and "core_pos" not in driver.subset_batch(plain, [1])
    for k in ("atom_type", "bond_index", "bond_type", "batch", "stream_ids"):
        assert np.array_equal(plain[k], packed[k]), k
    assert "core_pos" not in driver.pack_batch([mols[0], mols[2]], confs)


class _NeverSamples:
    """A model on which any sampling call is an error: run_job must refuse before it gets here."""

    def begin_sampling(self, *a, **k):
        raise AssertionError("sampling started")

    def langevin_dynamics_sample_diffusion(self, *a, **k):
        raise AssertionError("sampling started")


def test_run_job_refuses_before_sampling(tmp_path):
    confs = driver.num_confs("2")
    quiet = lambda s: None
    job = lambda mols, where, **kw: driver.run_job(_NeverSamples(), mols, str(tmp_path / where), confs, 200, dict(n_steps=2), "cpu",
                                                   log=quiet, hold_core=True, **kw)
    with pytest.raises(ValueError, match="core_pos_<i>"):
        job(_mols(cores=()), "a")                                       # no molecule carries a core
    empty = _mols(cores=(1,))
    empty[1]["core_mask"][:] = False
    with pytest.raises(ValueError, match="core_pos_<i>"):
        job(empty, "a")                                                   # ... nor does one whose mask selects nothing
    with pytest.raises(ValueError, match="shard"):
        job(_mols(), "b", shard=True, rank=0, world=2)
    for w in (0.0, 1.5, -1.0, float("nan")):
        with pytest.raises(ValueError, match="core_weight"):
            job(_mols(), "c", core_weight=w)
    short = _mols()
    short[1]["core_pos"] = short[1]["core_pos"][:-1]
    with pytest.raises(ValueError, match="m1"):
        job(short, "d")
    for where in "abcd":
        assert not os.path.exists(str(tmp_path / where / "samples_all.npz"))
    # sample_batch itself: a hold without a core in the batch
    with pytest.raises(ValueError, match="core_pos"):
        driver.sample_batch(_NeverSamples(), driver.pack_batch(_mols(cores=()), confs), "cpu", dict(n_steps=2), core={})


class _HeldRun:
    def __init__(self, at, G, n_steps, held):
        self.at, self.G, self.n_steps = at, G, n_steps
        self.core_dev = torch.arange(G, dtype=torch.float32) + 0.5 if held else None
        self.range_graphs = set()

    def remaining(self):
        return self.n_steps

    def advance(self, m):
        self.pos = self.at.to(torch.float32)[:, None].repeat(1, 3)

    def finish(self):
        return self.pos, []

    def nan_graphs(self):
        return torch.zeros(self.G, dtype=torch.bool)


class _HeldSampler:
    """Stands where the model does for the driver's bookkeeping: records the core keywords of every pass."""

    def __init__(self):
        self.calls = []

    def begin_sampling(self, at, pos_init, bi, bt, batch, G, extend_order, clip_local=None, save_traj=True, raise_on_nan=True,
                       noise=None, n_steps=2, **kw):
        self.calls.append({k: v for k, v in kw.items() if k.startswith("core_")})
        return _HeldRun(at, G, n_steps, "core_pos" in kw)


def test_sample_batch_hands_the_core_to_the_sampler_only_where_there_is_one():
    mols = _mols()
    confs = driver.num_confs("2")
    packed = driver.pack_batch(mols, confs)
    m = _HeldSampler()
    held = {"weight": 0.5, "start_sigma": 0.7}
    _, _, ok = driver.sample_batch(m, packed, "cpu", dict(n_steps=3), log=lambda s: None, core=held)
    assert ok.all() and len(m.calls) == 1
    kw = m.calls[0]
    assert np.array_equal(kw["core_pos"], packed["core_pos"]) and np.array_equal(kw["core_select"], packed["core_select"])
    assert kw["core_weight"] == 0.5 and kw["core_start_sigma"] == 0.7
    assert held["dev"].dtype == torch.float32 and held["dev"].tolist() == [0.5, 1.5, 2.5, 3.5, 4.5, 5.5]
    # without `core` the sampler sees none of the keywords, whatever the batch carries
    m2 = _HeldSampler()
    driver.sample_batch(m2, packed, "cpu", dict(n_steps=3), log=lambda s: None)
    assert m2.calls == [{}]
    # a pass over molecules without a core (here: the batch restricted to them) is sampled as ever
    m3 = _HeldSampler()
    held3 = {"weight": 1.0}
    sub = driver.subset_batch(packed, [0, 2])
    driver.sample_batch(m3, sub, "cpu", dict(n_steps=3), log=lambda s: None, core=held3)
    assert m3.calls == [{}] and torch.isnan(held3["dev"]).all()
