"""GPU (MI355X): every conformer's RMSD to a target along the denoising run (csrc/eval.hip: agdiff_traj_rmsd; agdiff_amd/trajectory.py;
epsnet.LangevinRun with rmsd_target; driver --track-rmsd) against oracle.covmat_oracle.kabsch_rmsd (float64 SVD) per (frame,
graph) on the selected atoms -- and on the centroid-inverted frame for the mirror output -- at the project's RMSD bar of 2e-5
Angstrom absolute (tests/test_hip_eval.py, tests/test_hip_ensemble.py: the same pair arithmetic)."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import t

pytestmark = pytest.mark.gpu

TOL = 2e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _walk(rng, n, step=1.5):
    d = rng.normal(size=(n, 3))
    d *= step / np.linalg.norm(d, axis=1, keepdims=True)
    return np.cumsum(d, axis=0)


def _oracle(frames, target, batch, select):
    """(proper, mirror) float64 [S, G]: kabsch_rmsd of the selected atoms of every (frame, graph) onto the target's, and of the frame
    inverted through the centroid of those atoms."""
    from oracle.covmat_oracle import kabsch_rmsd
    frames, target = np.asarray(frames, dtype=np.float64), np.asarray(target, dtype=np.float64)
    batch, select = np.asarray(batch), np.asarray(select).astype(bool)
    S, G = frames.shape[0], int(batch[-1]) + 1
    out, mir = np.zeros((S, G)), np.zeros((S, G))
    for g in range(G):
        idx = np.nonzero((batch == g) & select)[0]
        y = target[idx]
        for s in range(S):
            x = frames[s, idx]
            out[s, g] = kabsch_rmsd(x, y)
            mir[s, g] = kabsch_rmsd(2.0 * x.mean(axis=0) - x, y)
    return out, mir


def _case(seed=0, heavy=(1, 2, 3, 63, 64, 65, 129), S=3):
    """One packed batch: graph g has heavy[g] selected (heavy) atoms with hydrogens interleaved irregularly, so that graph offsets
    and the selected atoms' positions inside a graph are irregular.  Target = a random walk of 1.5 A steps per graph; every frame
    = another random walk of each graph, rigidly moved (random proper rotation + translation)."""
    rng = np.random.default_rng(seed)
    types, batch = [], []
    for g, h in enumerate(heavy):
        ty = []
        for _ in range(h):
            ty.extend([1] * int(rng.integers(0, 3)))
            ty.append(int(rng.choice([6, 7, 8])))
        ty.extend([1] * int(rng.integers(0, 4)))
        types.extend(ty)
        batch.extend([g] * len(ty))
    atom_type, batch = np.asarray(types, dtype=np.int64), np.asarray(batch, dtype=np.int64)
    N, G = atom_type.shape[0], len(heavy)
    target = np.zeros((N, 3))
    frames = np.zeros((S, N, 3))
    for g in range(G):
        idx = np.nonzero(batch == g)[0]
        target[idx] = _walk(rng, idx.size) + rng.normal(size=3) * 5.0
        for s in range(S):
            frames[s, idx] = _walk(rng, idx.size) @ _rotation(rng).T + rng.normal(size=3) * 10.0
    return dict(atom_type=atom_type, batch=batch, select=atom_type != 1, target=target.astype(np.float32),
                frames=frames.astype(np.float32), N=N, G=G, S=S)


_SHARED = {}


def _shared_case():
    """The oracle case and its float64 reference, computed once for the tests that use them (never modified)."""
    if not _SHARED:
        c = _case()
        c["ref"], c["ref_mirror"] = _oracle(c["frames"], c["target"], c["batch"], c["select"])
        _SHARED.update(c)
    return _SHARED


def _report(name, got, ref):
    err = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())
    print("traj_rmsd %-52s max |err| %.2e (bar %.0e)" % (name, err, TOL))
    return err


# ---------------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("strided", [False, True])
def test_against_the_oracle(strided):
    from agdiff_amd.trajectory import rmsd_to_target
    c = _shared_case()
    assert c["G"] == 7 and [int(c["select"][c["batch"] == g].sum()) for g in range(7)] == [1, 2, 3, 63, 64, 65, 129]
    assert int((~c["select"]).sum()) > 100                                  # hydrogens in between: irregular offsets
    if strided:
        pitch = 3 * c["N"] + 5
        buf = torch.full((c["S"], pitch), float("nan"), device="cuda:0")
        buf[:, :3 * c["N"]] = t(c["frames"]).cuda().reshape(c["S"], -1)
        frames = torch.as_strided(buf, (c["S"], c["N"], 3), (pitch, 3, 1))
        assert frames.stride(0) == pitch and not frames.is_contiguous()
    else:
        frames = t(c["frames"]).cuda()
    got, mir = rmsd_to_target(frames, c["target"], c["batch"], atom_type=c["atom_type"], mirror=True)
    assert got.shape == mir.shape == (c["S"], c["G"]) and got.dtype == mir.dtype == torch.float32 and got.is_cuda
    e1 = _report("proper%s" % (" strided" if strided else ""), got.cpu().numpy(), c["ref"])
    e2 = _report("mirror%s" % (" strided" if strided else ""), mir.cpu().numpy(), c["ref_mirror"])
    assert e1 < TOL and e2 < TOL
    # the proper output alone is the same launch without the second store; `select` given explicitly equals the heavy-atom default
    alone = rmsd_to_target(frames, t(c["target"]).cuda(), t(c["batch"]).cuda(), select=c["select"])
    assert torch.equal(alone, got)
    if strided:
        plain = rmsd_to_target(t(c["frames"]).cuda(), c["target"], c["batch"], atom_type=c["atom_type"], mirror=True)
        assert torch.equal(plain[0], got) and torch.equal(plain[1], mir)       # independent of frame_stride


# ---------------------------------------------------------------------------------------------------- 2. known answers
def test_known_answers_rigid_motion_and_mirror_image():
    from agdiff_amd.trajectory import rmsd_to_target
    from oracle.covmat_oracle import kabsch_rmsd
    rng = np.random.default_rng(4)
    sizes = [9, 70, 3]                                   # graph 0: a chiral 9-atom walk
    batch = np.repeat(np.arange(3), sizes)
    target = np.concatenate([_walk(rng, n) for n in sizes])
    moved, mirrored = np.zeros_like(target), np.zeros_like(target)
    for g in range(3):
        idx = np.nonzero(batch == g)[0]
        R, shift = _rotation(rng), rng.normal(size=3) * 8.0
        moved[idx] = target[idx] @ R.T + shift
        mirrored[idx] = -(target[idx] @ R.T) + shift       # the rigidly moved mirror image (inversion = a reflection x a rotation)
    frames = np.stack([moved, mirrored]).astype(np.float32)
    tgt = target.astype(np.float32)
    # on the oracle first: graph 0 is chiral -- its mirror image does not superpose
    i0 = np.nonzero(batch == 0)[0]
    assert kabsch_rmsd(frames[0, i0], tgt[i0]) < TOL and kabsch_rmsd(frames[1, i0], tgt[i0]) > 0.1
    assert kabsch_rmsd(2.0 * frames[1, i0].astype(np.float64).mean(axis=0) - frames[1, i0], tgt[i0]) < TOL
    out, mir = rmsd_to_target(frames, tgt, batch, mirror=True)          # (neither select nor atom_type: all atoms)
    out, mir = out.cpu().numpy(), mir.cpu().numpy()
    print("traj_rmsd known answers: rigid %s  mirror-of-mirror %s  chiral proper %.3f" % (out[0], mir[1], out[1, 0]))
    assert (out[0] < TOL).all() and (mir[1] < TOL).all()
    assert out[1, 0] > 0.1 and mir[0, 0] > 0.1
    assert out[1, 2] < TOL                               # three atoms are planar: the mirror image superposes properly too


# ---------------------------------------------------------------------------------------------------- 3. selection
def test_unselected_atoms_do_not_enter():
    from agdiff_amd.trajectory import rmsd_to_target
    c = _shared_case()
    base = rmsd_to_target(c["frames"], c["target"], c["batch"], atom_type=c["atom_type"], mirror=True)
    rng = np.random.default_rng(9)
    frames, target = c["frames"].copy(), c["target"].copy()
    hyd = ~c["select"]
    assert hyd.sum() > 50
    frames[:, hyd] += rng.normal(size=(c["S"], int(hyd.sum()), 3)).astype(np.float32) * 3.0
    target[hyd] -= 7.0
    frames[1, np.nonzero(hyd)[0][3]] = np.nan            # not even a NaN in an unselected atom shows
    got = rmsd_to_target(frames, target, c["batch"], atom_type=c["atom_type"], mirror=True)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])


# ---------------------------------------------------------------------------------------------------- 4. non-finite input
def test_non_finite_input_marks_exactly_its_entry():
    from agdiff_amd.trajectory import rmsd_to_target
    c = _shared_case()
    base = [x.cpu() for x in rmsd_to_target(c["frames"], c["target"], c["batch"], atom_type=c["atom_type"], mirror=True)]
    assert torch.isfinite(base[0]).all() and torch.isfinite(base[1]).all()
    sel_of = lambda g: np.nonzero((c["batch"] == g) & c["select"])[0]
    frames = c["frames"].copy()
    frames[0, sel_of(4)[60], 1] = np.nan                 # (s, g) = (0, 4)
    frames[2, sel_of(1)[1], 2] = np.inf                  # (s, g) = (2, 1)
    frames[1, sel_of(6)[100], 0] = -np.inf               # (s, g) = (1, 6): an atom past the first 64-lane stride of its graph
    got = [x.cpu() for x in rmsd_to_target(frames, c["target"], c["batch"], atom_type=c["atom_type"], mirror=True)]
    hit = torch.zeros(c["S"], c["G"], dtype=torch.bool)
    hit[0, 4] = hit[2, 1] = hit[1, 6] = True
    for b, g in zip(base, got):
        assert torch.isnan(g[hit]).all()
        assert torch.equal(g[~hit], b[~hit])
    # a non-finite TARGET coordinate: that graph's column in every frame
    target = c["target"].copy()
    target[sel_of(3)[5], 0] = np.nan
    got = [x.cpu() for x in rmsd_to_target(c["frames"], target, c["batch"], atom_type=c["atom_type"], mirror=True)]
    col = torch.zeros(c["S"], c["G"], dtype=torch.bool)
    col[:, 3] = True
    for b, g in zip(base, got):
        assert torch.isnan(g[col]).all() and torch.equal(g[~col], b[~col])


# ---------------------------------------------------------------------------------------------------- 5. consistency
def test_consistent_with_the_rmsd_matrix():
    """One graph, S frames: agdiff_rmsd_matrix with R = 1 reference (the target) and P = 1 (identity) on the same atoms -- the same
    arithmetic in another summation order, so to the bar and not bit for bit."""
    from agdiff_amd import _lib
    from agdiff_amd.trajectory import rmsd_to_target
    rng = np.random.default_rng(21)
    n, S = 37, 5
    atom_type = rng.choice([1, 6, 8], size=n, p=[0.4, 0.4, 0.2])
    atom_type[0] = 6
    idx = np.nonzero(atom_type != 1)[0].astype(np.int32)
    target = _walk(rng, n).astype(np.float32)
    frames = np.stack([_walk(rng, n) @ _rotation(rng).T + rng.normal(size=3) * 4.0 for _ in range(S)]).astype(np.float32)
    got = rmsd_to_target(frames, target, np.zeros(n, dtype=np.int64), atom_type=atom_type)
    lib = _lib.load()
    m = int(idx.shape[0])
    ref_d, gen_d, idx_d = t(target[None]).cuda().contiguous(), t(frames).cuda().contiguous(), t(idx).cuda()
    scratch = torch.empty((1 + S) * (3 * m + 1), dtype=torch.float32, device="cuda:0")
    out = torch.empty((1, S), dtype=torch.float32, device="cuda:0")
    _lib.check(lib.agdiff_rmsd_matrix(_lib.ptr(ref_d), _lib.ptr(gen_d), _lib.ptr(idx_d), ctypes.c_void_p(0), 1, S, n, m, 1,
                                      _lib.ptr(scratch), _lib.ptr(out), _lib.stream_ptr()), "agdiff_rmsd_matrix")
    err = _report("vs agdiff_rmsd_matrix", got[:, 0].cpu().numpy(), out[0].cpu().numpy().astype(np.float64))
    assert err < TOL


# ---------------------------------------------------------------------------------------------------- 6. sampler
def _sampler_setup():
    from agdiff_amd import get_model, qm9_model_config, synth
    from oracle import agdiff_oracle as O
    cfg = qm9_model_config(num_diffusion_timesteps=12)
    sd = O.synth_state_dict_for(cfg)
    m = get_model(cfg)
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    m = m.to("cuda:0").eval()
    b = synth.make_packed_batch("qm9", 3, 2, seed=7)             # three molecules, two conformers each
    at, bi, bt, ba = [t(b[k]).cuda() for k in ("atom_type", "bond_index", "bond_type", "batch")]
    gen = torch.Generator().manual_seed(3)
    N = at.shape[0]
    pos_init = torch.randn(N, 3, generator=gen)
    noise = torch.randn(10, N, 3, generator=gen)
    target = torch.randn(N, 3, generator=gen) * 1.5
    return m, b, (at, bi, bt, ba), pos_init, noise, target


def _run(m, b, graph, pos_init, noise, **extra):
    at, bi, bt, ba = graph
    run = m.begin_sampling(at, pos_init.cuda(), bi, bt, ba, b["num_graphs"], False, n_steps=10, w_global=1.0, global_start_sigma=0.5,
                           clip=1000.0, noise=noise.cuda(), nan_check_every=4, **extra)
    run.advance(run.remaining())
    pos, traj = run.finish()
    _FUSED[id(run)] = bool(run._fused_front())           # (asked while model.fused_front is what the run ran with)
    return run, pos.cpu(), traj


_RUNS = {}
_FUSED = {}             # id(run) -> which front the run took (the runs live in _RUNS for the module's lifetime)


def _sampler_runs():
    """The runs of the sampler tests, made once, all with the same pos_init and noise: `off` (no tracking), `kept` (tracking,
    save_traj=True), `ring` (tracking, save_traj=False: a ring of 8 frames for 10 steps, polled at steps 4 and 8), and with
    model.fused_front = False `loose` (as `ring`), `loose_kept` (as `kept`) and `loose_off` (as `off`).  Each = (run, pos, traj)."""
    if not _RUNS:
        m, b, graph, pos_init, noise, target = _sampler_setup()
        track = dict(rmsd_target=target, rmsd_mirror=True)
        _RUNS["setup"] = (m, b, graph, pos_init, noise, target)
        _RUNS["off"] = _run(m, b, graph, pos_init, noise)
        _RUNS["kept"] = _run(m, b, graph, pos_init, noise, **track)
        _RUNS["ring"] = _run(m, b, graph, pos_init, noise, save_traj=False, **track)
        m.fused_front = False
        try:
            _RUNS["loose"] = _run(m, b, graph, pos_init, noise, save_traj=False, **track)
            _RUNS["loose_kept"] = _run(m, b, graph, pos_init, noise, **track)
            _RUNS["loose_off"] = _run(m, b, graph, pos_init, noise)
        finally:
            m.fused_front = True
    return _RUNS


def test_sampler_tracks_the_curve_with_and_without_the_trajectory():
    from agdiff_amd.trajectory import rmsd_to_target
    R = _sampler_runs()
    m, b, graph, pos_init, noise, target = R["setup"]
    assert b["num_graphs"] == 6
    heavy = (graph[0] != 1).cpu().numpy()
    batch = np.asarray(b["batch"])
    (off_run, off_pos, off_traj), (kept_run, kept_pos, kept_traj), (ring_run, ring_pos, ring_traj) = R["off"], R["kept"], R["ring"]
    assert off_run.rmsd_curve is None and off_run.rmsd_curve_mirror is None and off_run._rmsd is None and off_run._rmsd_ring is None
    assert ring_traj == [] and ring_run.traj is None and ring_run._rmsd_ring.shape[0] == 8        # 2 x nan_check_every < 10 steps
    assert _FUSED[id(kept_run)] and _FUSED[id(ring_run)] and kept_run.graph_steps == 0 and kept_run._rmsd_ring is None
    # tracking changes nothing of the run
    assert torch.equal(kept_pos, off_pos) and torch.equal(ring_pos, off_pos)
    assert len(kept_traj) == 10 and all(torch.equal(a, b_) for a, b_ in zip(kept_traj, off_traj))
    for run in (kept_run, ring_run):
        for curve in (run.rmsd_curve, run.rmsd_curve_mirror):
            assert tuple(curve.shape) == (10, 6) and curve.dtype == torch.float32 and not curve.is_cuda
    # ring (wrapped, polled mid-run) == trajectory rows == the stand-alone call on the stacked trajectory, bit for bit
    assert torch.equal(kept_run.rmsd_curve, ring_run.rmsd_curve) and torch.equal(kept_run.rmsd_curve_mirror, ring_run.rmsd_curve_mirror)
    alone = rmsd_to_target(torch.stack(kept_traj), target, batch, atom_type=graph[0], mirror=True)
    assert torch.equal(alone[0].cpu(), kept_run.rmsd_curve) and torch.equal(alone[1].cpu(), kept_run.rmsd_curve_mirror)
    # ... and right: against the oracle on the run's trajectory
    ref, ref_mirror = _oracle(torch.stack(kept_traj).numpy(), target.numpy(), batch, heavy)
    assert _report("sampler fused, proper", kept_run.rmsd_curve.numpy(), ref) < TOL
    assert _report("sampler fused, mirror", kept_run.rmsd_curve_mirror.numpy(), ref_mirror) < TOL
    # without rmsd_mirror there is no mirror curve; an explicit selection equal to the default gives the same bits
    plain_run, _, _ = _run(m, b, graph, pos_init, noise, save_traj=False, rmsd_target=target, rmsd_select=graph[0] != 1)
    assert plain_run.rmsd_curve_mirror is None and torch.equal(plain_run.rmsd_curve, kept_run.rmsd_curve)


def test_sampler_tracks_launch_by_launch_too():
    """model.fused_front = False: update, graph build and forward launch by launch (the path a batch with a large molecule takes)."""
    R = _sampler_runs()
    m, b, graph, pos_init, noise, target = R["setup"]
    heavy = (graph[0] != 1).cpu().numpy()
    batch = np.asarray(b["batch"])
    (loose_run, loose_pos, _), (lk_run, lk_pos, lk_traj), (lo_run, lo_pos, lo_traj) = R["loose"], R["loose_kept"], R["loose_off"]
    assert not _FUSED[id(loose_run)] and not _FUSED[id(lk_run)] and not _FUSED[id(lo_run)] and loose_run._rmsd_ring.shape[0] == 8 and lo_run.rmsd_curve is None
    assert tuple(loose_run.rmsd_curve.shape) == (10, 6) and tuple(loose_run.rmsd_curve_mirror.shape) == (10, 6)
    ref, ref_mirror = _oracle(torch.stack(lk_traj).numpy(), target.numpy(), batch, heavy)
    e1 = _report("sampler launch by launch, proper", lk_run.rmsd_curve.numpy(), ref)
    e2 = _report("sampler launch by launch, mirror", lk_run.rmsd_curve_mirror.numpy(), ref_mirror)
    assert e1 < TOL and e2 < TOL
    # ring == trajectory rows, and tracking changes nothing of this run either
    assert torch.equal(loose_run.rmsd_curve, lk_run.rmsd_curve) and torch.equal(loose_run.rmsd_curve_mirror, lk_run.rmsd_curve_mirror)
    assert torch.equal(loose_pos, lo_pos) and torch.equal(lk_pos, lo_pos) and all(torch.equal(a, b_) for a, b_ in zip(lk_traj, lo_traj))


def test_final_positions_agree_across_the_two_fronts():
    """The tracked launch-by-launch run ends where the untracked fused run ends, bit for bit.  (That tracking changes nothing within
    either front is asserted above; this compares ACROSS the fronts, which tests/test_hip_poly.py::
    test_fused_front_equals_the_unfused_loop gates at 2e-6 relative because the two update kernels sum a node's terms over
    different lane partitions.  The figure this test prints has not been recorded on a GPU yet.)"""
    R = _sampler_runs()
    loose_pos, off_pos = R["loose"][1], R["off"][1]
    print("traj_rmsd final pos, launch by launch vs fused front: max |diff| %.3e" % float((loose_pos - off_pos).abs().max()))
    assert torch.equal(loose_pos, off_pos)


def test_a_quarantined_graph_has_a_nan_column():
    R = _sampler_runs()
    m, b, graph, pos_init, noise, target = R["setup"]
    kept_run = R["kept"][0]
    batch = np.asarray(b["batch"])
    bad_init = pos_init.clone()
    bad_init[int(np.nonzero(batch == 2)[0][1]), 0] = float("nan")
    nan_run, nan_pos, _ = _run(m, b, graph, bad_init, noise, save_traj=False, rmsd_target=target, rmsd_mirror=True, raise_on_nan=False)
    assert nan_run.nan_graphs().tolist() == [False, False, True, False, False, False]
    others = [0, 1, 3, 4, 5]
    for got, want in ((nan_run.rmsd_curve, kept_run.rmsd_curve), (nan_run.rmsd_curve_mirror, kept_run.rmsd_curve_mirror)):
        assert torch.isnan(got[:, 2]).all() and torch.equal(got[:, others], want[:, others])


# ---------------------------------------------------------------------------------------------------- 7. driver and command line
def test_run_job_saves_the_curves_and_the_command_line_reproduces_them(tmp_path):
    from agdiff_amd import driver, get_model, qm9_model_config, synth
    from oracle.covmat_oracle import kabsch_rmsd
    m = get_model(qm9_model_config(num_diffusion_timesteps=8))
    m.load_state_dict(synth.synth_state_dict(m.state_dict()))
    m = m.to("cuda:0").eval()
    rng = np.random.default_rng(5)
    mols = []
    for i, n in enumerate((13, 9)):
        at, r, c, ty = synth.random_molecule(rng, n)
        mols.append(dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=ty, num_refs=3 + i, name="mol%d" % i, index=i,
                         pos_target=_walk(rng, n).astype(np.float32)))
    testset = str(tmp_path / "test.npz")
    driver.save_testset(testset, mols)
    mols = driver.load_testset(testset)
    confs = lambda num_refs: num_refs
    kw = dict(n_steps=6, step_lr=1e-6, w_global=1.0, clip=1000.0)
    quiet = lambda *_: None
    res = driver.run_job(m, mols, str(tmp_path / "tracked"), confs, 10 ** 6, kw, "cuda:0", log=quiet, save_traj=True, track_rmsd=True)
    for i, mol in enumerate(mols):
        g, n = 3 + i, mol["atom_type"].shape[0]
        curve = res["rmsd_traj_%d" % i]
        assert curve.shape == (6, g) and curve.dtype == np.float32 and np.isfinite(curve).all()
        assert "rmsd_mirror_traj_%d" % i not in res and res["traj_%d" % i].shape == (6, g, n, 3)
        hv = np.nonzero(mol["atom_type"] != 1)[0]
        want = np.array([kabsch_rmsd(res["pos_gen_%d" % i][c][hv], mol["pos_target"][hv]) for c in range(g)])
        assert _report("run_job last row, molecule %d" % i, curve[-1], want) < TOL
    # with the mirror switch and without --save-traj: the same proper curves from the ring, plus the mirror's
    torch.manual_seed(0)
    both = driver.run_job(m, mols, str(tmp_path / "mirror"), confs, 10 ** 6, kw, "cuda:0", log=quiet, track_rmsd_mirror=True)
    assert {"rmsd_traj_0", "rmsd_mirror_traj_0", "rmsd_traj_1", "rmsd_mirror_traj_1"} <= set(both) and "traj_0" not in both
    assert both["rmsd_mirror_traj_1"].shape == (6, 4)
    # the command line on the saved trajectory: bit for bit what the run tracked
    out = str(tmp_path / "curves.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "agdiff_amd.trajectory", "--samples", str(tmp_path / "tracked" / "samples_all.npz"),
                        "--testset", testset, "--out", out, "--mirror"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    z = np.load(out)
    assert set(z.files) == {"rmsd_traj_0", "rmsd_mirror_traj_0", "rmsd_traj_1", "rmsd_mirror_traj_1"}
    for i in range(2):
        assert np.array_equal(z["rmsd_traj_%d" % i], res["rmsd_traj_%d" % i])
        assert z["rmsd_mirror_traj_%d" % i].shape == res["rmsd_traj_%d" % i].shape
    assert len(glob.glob(str(tmp_path / "tracked" / "samples_[0-9]*.npz"))) == 1
