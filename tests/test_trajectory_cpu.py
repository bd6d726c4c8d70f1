"""CPU: host logic of the trajectory RMSD tracking (agdiff_amd/trajectory.py, driver --track-rmsd): the export and its
declaration, the ring's row spans, argument checks, the test set's `pos_target_<i>`, packing, and the driver's refusals.  Nothing
here computes on a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from agdiff_amd import _lib, driver, synth, trajectory


def test_export_argtypes_and_header():
    lib = _lib.load()
    assert hasattr(lib, "agdiff_traj_rmsd")
    P, I = ctypes.c_void_p, ctypes.c_int32
    assert _lib.EXPORTS["agdiff_traj_rmsd"] == [P, ctypes.c_int64, P, P, P, I, I, I, P, P, P]
    assert list(lib.agdiff_traj_rmsd.argtypes) == _lib.EXPORTS["agdiff_traj_rmsd"] and lib.agdiff_traj_rmsd.restype is ctypes.c_int
    src = open(_lib.HEADER).read()
    assert "int agdiff_traj_rmsd(const float* frames, int64_t frame_stride" in src
    # the export came without an ABI bump: library and header still agree on the version
    assert lib.agdiff_abi_version() == _lib.DEFINES["AGDIFF_ABI_VERSION"]


def test_argument_errors_of_the_entry_point_need_no_gpu():
    """Null pointers, negative sizes, a stride below 3 N and overlapping outputs are refused before any launch."""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    call = lambda *a: lib.agdiff_traj_rmsd(*a)
    assert call(null, 12, p, p, p, 1, 1, 4, p, null, null) == -1
    assert call(p, 12, null, p, p, 1, 1, 4, p, null, null) == -1
    assert call(p, 12, p, null, p, 1, 1, 4, p, null, null) == -1
    assert call(p, 12, p, p, null, 1, 1, 4, p, null, null) == -1
    assert call(p, 12, p, p, p, 1, 1, 4, null, null, null) == -1
    assert call(p, 11, p, p, p, 1, 1, 4, p, null, null) == -1          # frame_stride < 3 N
    assert call(p, 12, p, p, p, -1, 1, 4, p, null, null) == -1
    assert call(p, 12, p, p, p, 1, -1, 4, p, null, null) == -1
    assert call(p, 12, p, p, p, 1, 1, 0, p, null, null) == -1
    assert call(p, 12, p, p, p, 1, 1, 4, p, p, null) == -1             # out_mirror == out
    assert call(p, 12, p, p, p, 0, 1, 4, p, null, null) == 0           # nothing to do: no launch
    assert call(p, 12, p, p, p, 1, 0, 4, p, null, null) == 0


def test_ring_spans():
    rs = trajectory.ring_spans
    assert rs(0, 0, 8) == [] and rs(5, 5, 8) == []
    assert rs(0, 3, 8) == [(0, 3)]                      # no wrap
    assert rs(3, 7, 8) == [(3, 7)]
    assert rs(11, 13, 8) == [(3, 5)]                    # later laps
    assert rs(7, 11, 8) == [(7, 8), (0, 3)]             # wrap
    assert rs(6, 14, 8) == [(6, 8), (0, 6)]             # exact fill, wrapped
    assert rs(8, 16, 8) == [(0, 8)]                     # exact fill, aligned
    assert rs(4, 8, 8) == [(4, 8)]                      # up to the ring's end: one span
    with pytest.raises(ValueError):
        rs(3, 12, 8)                                    # nine steps in eight rows
    with pytest.raises(ValueError):
        rs(5, 4, 8)
    with pytest.raises(ValueError):
        rs(0, 0, 0)
    # every step lands in its own row, in step order
    for done, ready, rows in ((0, 5, 5), (13, 21, 8), (9, 10, 2), (0, 1, 1)):
        got = [r for lo, hi in rs(done, ready, rows) for r in range(lo, hi)]
        assert got == [k % rows for k in range(done, ready)]


def test_rmsd_to_target_argument_checks():
    N = 6
    frames = np.zeros((2, N, 3), dtype=np.float32)
    target = np.zeros((N, 3), dtype=np.float32)
    batch = np.array([0, 0, 0, 1, 1, 1])
    f = trajectory.rmsd_to_target
    with pytest.raises(ValueError):
        f(np.zeros((2, N, 2), dtype=np.float32), target, batch)
    with pytest.raises(ValueError):
        f(frames, np.zeros((N + 1, 3), dtype=np.float32), batch)
    with pytest.raises(ValueError):
        f(frames, target, batch[:-1])
    with pytest.raises(ValueError):
        f(frames, target, np.array([0, 0, 1, 0, 1, 1]))                  # unsorted
    with pytest.raises(ValueError):
        f(frames, target, batch, select=np.ones(N - 1, dtype=bool))
    with pytest.raises(ValueError, match="graph 1 has no selected atom"):
        f(frames, target, batch, select=np.array([1, 0, 0, 0, 0, 0]))
    with pytest.raises(ValueError, match="graph 0 has no selected atom"):
        f(frames, target, batch, atom_type=np.array([1, 1, 1, 6, 1, 1]))   # graph 0: hydrogens only
    with pytest.raises(ValueError, match="no selected atom"):
        f(frames, target, np.array([0, 0, 0, 2, 2, 2]))                  # graph 1 has no atom at all


def _mols(k=3, targets=True):
    rng = np.random.default_rng(11)
    out = []
    for i in range(k):
        n = int(rng.integers(6, 14))
        at, r, c, t = synth.random_molecule(rng, n)
        m = dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=t, num_refs=1 + i, name="m%d" % i, index=i)
        if targets:
            m["pos_target"] = rng.normal(size=(n, 3)).astype(np.float32)
        out.append(m)
    return out


def test_pos_target_round_trips_through_the_testset(tmp_path):
    mols = _mols()
    del mols[1]["pos_target"]
    p = str(tmp_path / "t.npz")
    driver.save_testset(p, mols)
    back = driver.load_testset(p)
    assert back[1].get("pos_target") is None
    for k in (0, 2):
        assert back[k]["pos_target"].dtype == np.float32 and np.array_equal(back[k]["pos_target"], mols[k]["pos_target"])
    bad = _mols(1)
    bad[0]["pos_target"] = bad[0]["pos_target"][:-1]
    with pytest.raises(ValueError):
        driver.save_testset(str(tmp_path / "bad.npz"), bad)


def test_pack_and_subset_carry_the_target():
    mols = _mols()
    confs = driver.num_confs("2x")
    packed = driver.pack_batch(mols, confs)
    tgt = packed["pos_target"]
    assert tgt.dtype == np.float32 and tgt.shape == (packed["atom_type"].shape[0], 3)
    for m, (off, n, g) in zip(mols, packed["spans"]):
        assert g == confs(m["num_refs"])
        for c in range(g):
            assert np.array_equal(tgt[off + c * n:off + (c + 1) * n], m["pos_target"])
    sub = driver.subset_batch(packed, [2, 0])
    ref = driver.pack_batch([mols[2], mols[0]], confs)
    assert np.array_equal(sub["pos_target"], ref["pos_target"]) and np.array_equal(sub["atom_type"], ref["atom_type"])
    # a batch in which one molecule has no target carries none (and what it carried before is unchanged)
    some = _mols()
    del some[0]["pos_target"]
    assert "pos_target" not in driver.pack_batch(some, confs)
    plain = driver.pack_batch([{k: v for k, v in m.items() if k != "pos_target"} for m in mols], confs)
    assert "pos_target" not in plain and "pos_target" not in driver.subset_batch(plain, [1])
    for k in ("atom_type", "bond_index", "bond_type", "batch", "stream_ids"):
        assert np.array_equal(plain[k], packed[k]), k


class _NeverSamples:
    """A model on which any sampling call is an error: run_job must refuse before it gets here."""

    def begin_sampling(self, *a, **k):
        raise AssertionError("sampling started")

    def langevin_dynamics_sample_diffusion(self, *a, **k):
        raise AssertionError("sampling started")


def test_run_job_refuses_before_sampling(tmp_path):
    confs = driver.num_confs("2")
    mols = _mols()
    del mols[1]["pos_target"]
    with pytest.raises(ValueError, match="m1"):
        driver.run_job(_NeverSamples(), mols, str(tmp_path / "a"), confs, 200, dict(n_steps=2), "cpu", track_rmsd=True, log=lambda s: None)
    with pytest.raises(ValueError, match="m1"):
        driver.run_job(_NeverSamples(), mols, str(tmp_path / "a"), confs, 200, dict(n_steps=2), "cpu", track_rmsd_mirror=True,
                       log=lambda s: None)
    with pytest.raises(ValueError, match="shard"):
        driver.run_job(_NeverSamples(), _mols(), str(tmp_path / "b"), confs, 200, dict(n_steps=2), "cpu", track_rmsd=True, shard=True,
                       rank=0, world=2, log=lambda s: None)
    assert not os.path.exists(str(tmp_path / "a" / "samples_all.npz")) and not os.path.exists(str(tmp_path / "b" / "samples_all.npz"))
    # sample_batch itself: curves without a target in the batch
    with pytest.raises(ValueError, match="pos_target"):
        driver.sample_batch(_NeverSamples(), driver.pack_batch(_mols(targets=False), confs), "cpu", dict(n_steps=2), curves={})


class _CurveRun:
    """Stands where epsnet.LangevinRun does for the driver's bookkeeping: the curve of graph c at step s is 1000 x (first atom type
    of the graph) + 10 x s + (the pass's clip_local or 0); graphs whose first atom type is `nan_type` fail without local clipping."""

    def __init__(self, owner, at, batch, G, clip_local, n_steps, mirror):
        self.owner, self.at, self.batch, self.G, self.clip_local, self.n_steps = owner, at, batch, G, clip_local, n_steps
        first = torch.zeros(G, dtype=torch.long).scatter_reduce(0, batch, at, "amin", include_self=False)
        self.first = first
        self.rmsd_curve = (1000.0 * first[None, :] + 10.0 * torch.arange(n_steps)[:, None] + float(clip_local or 0)).float()
        self.rmsd_curve_mirror = -self.rmsd_curve if mirror else None
        self.range_graphs = set()

    def remaining(self):
        return self.n_steps

    def advance(self, m):
        self.pos = self.at.to(torch.float32)[:, None].repeat(1, 3)

    def finish(self):
        return self.pos, []

    def nan_graphs(self):
        return (self.first == self.owner.nan_type) & torch.tensor(self.clip_local is None)


class _CurveSampler:
    def __init__(self, nan_type=-1, never=False):
        self.nan_type, self.never, self.targets = nan_type, never, []

    def begin_sampling(self, at, pos_init, bi, bt, batch, G, extend_order, clip_local=None, save_traj=True, raise_on_nan=True,
                       noise=None, n_steps=2, rmsd_target=None, rmsd_mirror=False, **kw):
        self.targets.append(np.asarray(rmsd_target))
        return _CurveRun(self, at, batch, G, None if self.never else clip_local, n_steps, rmsd_mirror)


def test_sample_batch_sorts_the_curves_of_retried_and_dropped_molecules():
    mols = _mols(4)
    for k, m in enumerate(mols):
        m["atom_type"] = np.full_like(m["atom_type"], 2 + k)
    confs = driver.num_confs("2")
    packed = driver.pack_batch(mols, confs)
    m = _CurveSampler(nan_type=4)                  # molecule 2 fails its first pass and succeeds with clip_local=20
    curves = {"mirror": True}
    _, _, ok = driver.sample_batch(m, packed, "cpu", dict(n_steps=3), log=lambda s: None, curves=curves)
    assert ok.all() and curves["rmsd"].shape == (3, 8) and curves["rmsd"].dtype == torch.float32
    step = 10.0 * torch.arange(3, dtype=torch.float32)[:, None]
    want = torch.cat([1000.0 * (2 + k) + step + (20.0 if k == 2 else 0.0) for k in range(4) for _ in range(2)], dim=1)
    assert torch.equal(curves["rmsd"], want) and torch.equal(curves["rmsd_mirror"], -want)
    off, n, g = packed["spans"][2]
    assert len(m.targets) == 2 and np.array_equal(m.targets[0], packed["pos_target"])
    assert np.array_equal(m.targets[1], packed["pos_target"][off:off + n * g])          # the retry's target: that molecule's rows
    # a molecule that fails every attempt: its columns stay NaN, the others are unchanged; no mirror curve unless asked
    m2 = _CurveSampler(nan_type=4, never=True)
    curves2 = {}
    _, _, ok = driver.sample_batch(m2, packed, "cpu", dict(n_steps=3), log=lambda s: None, curves=curves2)
    assert ok.tolist() == [True, True, False, True] and "rmsd_mirror" not in curves2
    assert torch.isnan(curves2["rmsd"][:, 4:6]).all()
    keep = [0, 1, 2, 3, 6, 7]
    assert torch.equal(curves2["rmsd"][:, keep], want[:, keep])


def test_run_job_writes_the_curves(tmp_path):
    mols = _mols(3)
    for k, m in enumerate(mols):
        m["atom_type"] = np.full_like(m["atom_type"], 2 + k)
    out = str(tmp_path / "out")
    merged = driver.run_job(_CurveSampler(), mols, out, driver.num_confs("2"), 10 ** 6, dict(n_steps=4), "cpu", track_rmsd_mirror=True,
                            log=lambda s: None)
    for k in range(3):
        c = merged["rmsd_traj_%d" % k]
        assert c.shape == (4, 2) and c.dtype == np.float32 and np.array_equal(c[:, 0], 1000.0 * (2 + k) + 10.0 * np.arange(4))
        assert np.array_equal(merged["rmsd_mirror_traj_%d" % k], -c)
    plain = driver.run_job(_CurveSampler(), mols, str(tmp_path / "plain"), driver.num_confs("2"), 10 ** 6, dict(n_steps=4), "cpu",
                           log=lambda s: None)
    assert not any(k.startswith("rmsd_") for k in plain)
