"""GPU (MI355X): the rigid core hold (csrc/eval.hip: agdiff_hold_core; agdiff_amd/core.py; epsnet.LangevinRun with core_pos /
core_select; driver --hold-core) against the float64 restatement tests/core_ref.py (SVD Kabsch; anchored on the CPU in
tests/test_core_ref_cpu.py) at the project's RMSD bar of 2e-5 Angstrom absolute (tests/test_hip_trajectory.py,
tests/test_hip_eval.py).  The kernel's only fp32 step is the final rounding of a coordinate: at |x| <= 32 Angstrom that is
<= 1.9e-6 Angstrom, so the bar leaves a factor of ten."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import core_ref as C
from helpers import t

pytestmark = pytest.mark.gpu

TOL = 2e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    """int32 view of a float32 tensor / array on the host: equality of these is equality bit for bit, NaNs included."""
    x = x.detach().cpu() if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _hold(c, weight=1.0, skip=None, pos=None, core_pos=None, select=None):
    """One stand-alone launch on case c (or on the given replacements): (new pos, copy_out pre-filled with NaN, dev) on the host."""
    from agdiff_amd.core import hold_core
    p = t(c["pos"] if pos is None else pos).cuda().contiguous()
    copy = torch.full_like(p, float("nan"))
    got, dev = hold_core(p, c["core_pos"] if core_pos is None else core_pos, c["select"] if select is None else select, c["batch"],
                         weight=weight, skip=skip, copy_out=copy)
    assert got.data_ptr() == p.data_ptr() and dev.dtype == torch.float32 and tuple(dev.shape) == (c["G"],)
    return got.cpu(), copy.cpu(), dev.cpu()


_CASES = {}


def _case(family):
    """The packed case of a family and its float64 reference at weight 1 and 0.5, computed once (never modified)."""
    if family not in _CASES:
        c = C.case(family)
        c["ref"] = {w: C.hold_core(c["pos"], c["core_pos"], c["select"], c["batch"], weight=w) for w in (1.0, 0.5)}
        _CASES[family] = c
    return _CASES[family]


# ---------------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("weight", [1.0, 0.5])
@pytest.mark.parametrize("family", C.FAMILIES)
def test_against_the_restatement(family, weight):
    c = _case(family)
    batch, sel = c["batch"], c["select"]
    assert c["G"] == 7 and [int(sel[batch == g].sum()) for g in range(7)] == [1, 2, 3, 63, 64, 65, 129]
    assert int((~sel).sum()) > 100 and c["gap"] >= C.GAP_MIN
    ref, ref_dev, touched = c["ref"][weight]
    assert touched.all()
    got, copy, dev = _hold(c, weight)
    got64, worst, worst_dev = got.numpy().astype(np.float64), 0.0, 0.0
    for g in range(7):
        idx = np.nonzero((batch == g) & sel)[0]
        if idx.size >= 3:
            worst = max(worst, float(np.abs(got64[idx] - ref[idx]).max()))
            worst_dev = max(worst_dev, abs(float(dev[g]) - ref_dev[g]))
    print("hold_core %-10s weight %.1f: max |coordinate err| %.2e  max |dev err| %.2e (bar %.0e); smallest gap %.1e"
          % (family, weight, worst, worst_dev, TOL, c["gap"]))
    assert worst < TOL and worst_dev < TOL
    i0 = np.nonzero((batch == 0) & sel)[0]
    assert _same_bits(got[i0], c["pos"][i0]) and float(dev[0]) == 0.0                     # m = 1: the atom stays where it is
    i1 = np.nonzero((batch == 1) & sel)[0]
    if weight == 1.0:                                                                     # m = 2: the pair at the template's distance
        d_got = float(np.linalg.norm(got64[i1[0]] - got64[i1[1]]))
        d_tpl = float(np.linalg.norm(c["core_pos"][i1[0]].astype(np.float64) - c["core_pos"][i1[1]].astype(np.float64)))
        assert abs(d_got - d_tpl) < TOL
    assert np.isfinite(got64[i1]).all() and np.isfinite(float(dev[1]))
    hyd = np.nonzero(~sel)[0]
    assert _same_bits(got[hyd], c["pos"][hyd])                                            # unselected atoms keep their bits
    chosen = np.nonzero(sel)[0]
    assert _same_bits(copy[chosen], got[chosen]) and torch.isnan(copy[hyd]).all()         # copy_out: the new values, nothing else


# ---------------------------------------------------------------------------------------------------- 2. known answers
def test_known_answers_rigid_motion_and_mirror_image():
    from oracle.covmat_oracle import kabsch_rmsd
    rng = np.random.default_rng(4)
    sizes = [9, 70, 3]                                   # graph 0: a chiral 9-atom walk
    batch = np.repeat(np.arange(3), sizes)
    template = np.concatenate([C.walk(rng, n) for n in sizes])
    moved, mirrored = np.zeros_like(template), np.zeros_like(template)
    for g in range(3):
        idx = np.nonzero(batch == g)[0]
        R, shift = C.rotation(rng), rng.normal(size=3) * 8.0
        moved[idx] = template[idx] @ R.T + shift
        mirrored[idx] = -(template[idx] @ R.T) + shift     # the rigidly moved mirror image
    tpl = template.astype(np.float32)
    c = dict(pos=moved.astype(np.float32), core_pos=tpl, select=np.ones(batch.shape[0], dtype=bool), batch=batch, G=3)
    i0 = np.nonzero(batch == 0)[0]
    assert kabsch_rmsd(c["pos"][i0], tpl[i0]) < TOL and kabsch_rmsd(mirrored.astype(np.float32)[i0], tpl[i0]) > 0.1     # on the oracle first
    got, _, dev = _hold(c)
    err = float((got - t(c["pos"])).abs().max())
    print("hold_core known answers: rigid motion max |move| %.2e dev %s" % (err, dev.tolist()))
    assert err < TOL and (dev < TOL).all()
    got, _, dev = _hold(c, pos=mirrored.astype(np.float32))
    print("hold_core known answers: mirror image dev %s" % dev.tolist())
    assert float(dev[0]) > 0.1                            # proper rotations only: the template is held in ITS handedness
    assert float(dev[2]) < TOL                            # three atoms are planar: the mirror image superposes properly too
    assert kabsch_rmsd(got.numpy()[i0], tpl[i0]) < TOL    # what was written is the template itself, not its mirror image


# ---------------------------------------------------------------------------------------------------- 3. skip and non-finite
def test_skipped_empty_and_non_finite_graphs_are_left_alone():
    c = _case("noise 0.3")
    batch, sel = c["batch"], c["select"]
    base_pos, base_copy, base_dev = _hold(c)
    assert torch.isfinite(base_dev).all()
    sel_of = lambda g: np.nonzero((batch == g) & sel)[0]
    cases = []
    skip = np.zeros(7, dtype=np.int32)
    skip[4] = 1
    cases.append(("skip", 4, dict(skip=skip)))
    empty = sel.copy()
    empty[batch == 3] = False
    cases.append(("empty selection", 3, dict(select=empty)))
    pos = c["pos"].copy()
    pos[sel_of(6)[100], 0] = np.nan                      # an atom past the first 64-lane stride of its graph
    cases.append(("NaN in pos", 6, dict(pos=pos)))
    core_pos = c["core_pos"].copy()
    core_pos[sel_of(5)[7], 2] = np.nan
    cases.append(("NaN in core_pos", 5, dict(core_pos=core_pos)))
    pos_inf = c["pos"].copy()
    pos_inf[sel_of(3)[1], 1] = -np.inf
    cases.append(("inf in pos", 3, dict(pos=pos_inf)))
    for name, g, kw in cases:
        got, copy, dev = _hold(c, **kw)
        given = kw.get("pos", c["pos"])
        rows = np.nonzero(batch == g)[0]
        others = np.nonzero(batch != g)[0]
        assert _same_bits(got[rows], given[rows]), name                                   # the graph: bit for bit the input
        assert torch.isnan(copy[rows]).all(), name                                         # ... and nothing of it in copy_out
        assert torch.isnan(dev[g]), name
        keep = [k for k in range(7) if k != g]
        assert _same_bits(got[others], base_pos[others]) and _same_bits(dev[keep], base_dev[keep]), name
        assert _same_bits(copy[others], base_copy[others]), name
    # a NaN in an UNSELECTED atom changes nothing
    pos = c["pos"].copy()
    hyd = np.nonzero((batch == 6) & ~sel)[0][3]
    pos[hyd] = np.nan
    got, copy, dev = _hold(c, pos=pos)
    rest = np.arange(c["N"]) != hyd
    assert torch.isnan(got[hyd]).all() and _same_bits(got[rest], base_pos[rest]) and _same_bits(dev, base_dev)
    assert _same_bits(copy, base_copy)
    # skip given as all zeros is no skip
    got, copy, dev = _hold(c, skip=np.zeros(7, dtype=np.int32))
    assert _same_bits(got, base_pos) and _same_bits(dev, base_dev)


# ---------------------------------------------------------------------------------------------------- 4. sampler
_S = {}


def _sampler():
    """The set-up and the unconstrained runs of tests/test_hip_trajectory.py (`off`: fused front; `loose_off`: launch by launch),
    the core of every graph -- its first ceil(heavy / 2) heavy atoms, template = a walk per graph -- and the constrained run with
    the trajectory kept; made once."""
    if not _S:
        import test_hip_trajectory as TT
        R = TT._sampler_runs()
        m, b, graph, pos_init, noise, _ = R["setup"]
        at, batch = graph[0].cpu().numpy(), np.asarray(b["batch"])
        N, G = at.shape[0], int(b["num_graphs"])
        rng = np.random.default_rng(17)
        select, template = np.zeros(N, dtype=bool), np.zeros((N, 3), dtype=np.float32)
        for g in range(G):
            idx = np.nonzero(batch == g)[0]
            heavy = idx[at[idx] != 1]
            select[heavy[:(heavy.size + 1) // 2]] = True
            template[idx] = C.walk(rng, idx.size).astype(np.float32)
        run = lambda **kw: TT._run(m, b, graph, kw.pop("pos_init", pos_init), noise, **kw)
        fused = lambda r: TT._FUSED[id(r)]
        _S.update(TT=TT, m=m, b=b, graph=graph, pos_init=pos_init, noise=noise, batch=batch, N=N, G=G, select=select, template=template,
                  run=run, fused=fused, off=R["off"], loose_off=R["loose_off"], core=dict(core_pos=template, core_select=select))
        _S["held"] = run(**_S["core"])
    return _S


def _loose(S, **kw):
    """A run with model.fused_front = False (launch by launch), as the constrained runs go."""
    S["m"].fused_front = False
    try:
        return S["run"](**kw)
    finally:
        S["m"].fused_front = True


def _held_exactly(S, frame, graphs=None):
    """kabsch_rmsd of every graph's core in `frame` [N, 3] to the template's core: the largest over `graphs`."""
    from oracle.covmat_oracle import kabsch_rmsd
    frame = np.asarray(frame, dtype=np.float64)
    worst = 0.0
    for g in (range(S["G"]) if graphs is None else graphs):
        idx = np.nonzero((S["batch"] == g) & S["select"])[0]
        worst = max(worst, kabsch_rmsd(frame[idx], S["template"][idx]))
    return worst


def _alone(S, frame, weight=1.0):
    """The stand-alone launch on a frame of an unconstrained run."""
    c = dict(pos=frame.numpy(), core_pos=S["template"], select=S["select"], batch=S["batch"], G=S["G"])
    return _hold(c, weight)[0]


def test_sampler_holds_the_core_in_every_frame():
    S = _sampler()
    run, pos, traj = S["held"]
    sizes = [int(S["select"][S["batch"] == g].sum()) for g in range(S["G"])]
    assert S["G"] == 6 and min(sizes) >= 1 and max(sizes) >= 3 and (~S["select"]).sum() > S["select"].sum()
    assert len(traj) == 10
    worst = max(_held_exactly(S, f.numpy()) for f in traj + [pos])
    print("hold_core sampler: core sizes %s; largest core RMSD to the template over 10 frames + final %.2e (bar %.0e)" % (sizes, worst, TOL))
    assert worst < TOL
    assert torch.equal(traj[-1], pos)                                                      # copy_out reached the last row too
    dev = run.core_dev
    assert dev.dtype == torch.float32 and tuple(dev.shape) == (6,) and not dev.is_cuda and torch.isfinite(dev).all()
    # which paths: the constrained run goes launch by launch, without step graphs; a run without the keywords is what it was
    assert not S["fused"](run) and run.graph_steps == 0 and not run._use_graphs
    off_run, off_pos, off_traj = S["off"]
    again_run, again_pos, again_traj = S["run"]()
    assert S["fused"](off_run) and S["fused"](again_run) and off_run.core_dev is None and again_run.graph_steps == off_run.graph_steps
    assert _same_bits(again_pos, off_pos) and all(_same_bits(a, b_) for a, b_ in zip(again_traj, off_traj))


def test_sampler_first_step_is_the_update_then_the_hold():
    S = _sampler()
    _, _, traj = S["held"]
    lo_traj = S["loose_off"][2]
    sel, hyd = np.nonzero(S["select"])[0], np.nonzero(~S["select"])[0]
    assert _same_bits(traj[0][hyd], lo_traj[0][hyd])
    assert _same_bits(traj[0][sel], _alone(S, lo_traj[0])[sel])
    assert not _same_bits(traj[0][sel], lo_traj[0][sel])                                   # (the hold did move them)


def test_sampler_empty_selection_is_the_unconstrained_launch_by_launch_run():
    S = _sampler()
    run, pos, traj = S["run"](core_pos=S["template"], core_select=np.zeros(S["N"], dtype=bool))
    lo_run, lo_pos, lo_traj = S["loose_off"]
    assert not S["fused"](run) and run.graph_steps == 0 and torch.isnan(run.core_dev).all()
    assert _same_bits(pos, lo_pos) and len(traj) == 10 and all(_same_bits(a, b_) for a, b_ in zip(traj, lo_traj))


def test_sampler_core_start_sigma():
    S = _sampler()
    lo_run, _, lo_traj = S["loose_off"]
    sig = [s[0] for s in lo_run._sched]
    assert len(sig) == 10 and all(a > b_ for a, b_ in zip(sig, sig[1:]))
    k0 = 4
    start = 0.5 * (sig[k0 - 1] + sig[k0])                  # between two sigmas of the schedule: step k0 is the first one held
    run, pos, traj = S["run"](core_start_sigma=start, **S["core"])
    assert not S["fused"](run)
    for k in range(k0):
        assert _same_bits(traj[k], lo_traj[k]), k
    sel, hyd = np.nonzero(S["select"])[0], np.nonzero(~S["select"])[0]
    assert _same_bits(traj[k0][hyd], lo_traj[k0][hyd])
    assert _same_bits(traj[k0][sel], _alone(S, lo_traj[k0])[sel]) and not _same_bits(traj[k0][sel], lo_traj[k0][sel])
    assert _held_exactly(S, pos.numpy()) < TOL and torch.equal(traj[-1], pos)
    # a start sigma below the whole schedule: only the closing hold runs
    run, pos, traj = S["run"](core_start_sigma=0.5 * sig[-1], **S["core"])
    assert all(_same_bits(traj[k], lo_traj[k]) for k in range(9)) and _same_bits(traj[9][hyd], lo_traj[9][hyd])
    assert _held_exactly(S, pos.numpy()) < TOL and torch.isfinite(run.core_dev).all()


def test_sampler_core_weight_blends_and_the_closing_hold_is_exact():
    S = _sampler()
    lo_traj = S["loose_off"][2]
    run, pos, traj = S["run"](core_weight=0.5, **S["core"])
    frame0 = lo_traj[0].numpy()
    gap = C.assert_gaps(frame0, S["template"], S["select"], S["batch"])
    ref, _, _ = C.hold_core(frame0, S["template"], S["select"], S["batch"], weight=0.5)
    worst, seen = 0.0, 0
    for g in range(S["G"]):
        idx = np.nonzero((S["batch"] == g) & S["select"])[0]
        if idx.size >= 3:
            worst, seen = max(worst, float(np.abs(traj[0].numpy().astype(np.float64)[idx] - ref[idx]).max())), seen + 1
    print("hold_core sampler weight 0.5: frame 0 vs the restatement's blend, %d graphs: max |err| %.2e (bar %.0e; gap %.1e)" % (seen, worst, TOL, gap))
    assert seen >= 1 and worst < TOL
    hyd = np.nonzero(~S["select"])[0]
    assert _same_bits(traj[0][hyd], lo_traj[0][hyd])
    assert _held_exactly(S, traj[0].numpy()) > 100 * TOL                                   # half way is not on the template yet
    assert _held_exactly(S, pos.numpy()) < TOL and torch.equal(traj[-1], pos)              # the closing launch runs at weight 1


def test_sampler_leaves_a_quarantined_graph_alone():
    S = _sampler()
    bad_init = S["pos_init"].clone()
    bad_init[int(np.nonzero(S["batch"] == 2)[0][1]), 0] = float("nan")
    run, pos, _ = S["run"](pos_init=bad_init, raise_on_nan=False, **S["core"])
    free_run, free_pos, _ = _loose(S, pos_init=bad_init, raise_on_nan=False)
    assert run.nan_graphs().tolist() == [False, False, True, False, False, False] == free_run.nan_graphs().tolist()
    rows = np.nonzero(S["batch"] == 2)[0]
    assert _same_bits(pos[rows], free_pos[rows])                                           # the placeholder: as without a core
    assert torch.isnan(run.core_dev[2]) and torch.isfinite(run.core_dev[[0, 1, 3, 4, 5]]).all()
    assert _held_exactly(S, pos.numpy(), graphs=[0, 1, 3, 4, 5]) < TOL


def test_sampler_tracking_sees_the_held_frames():
    from agdiff_amd.trajectory import rmsd_to_target
    S = _sampler()
    _, held_pos, held_traj = S["held"]
    target = S["TT"]._sampler_runs()["setup"][5]
    ring_run, ring_pos, ring_traj = S["run"](save_traj=False, rmsd_target=target, **S["core"])
    assert ring_traj == [] and ring_run._rmsd_ring.shape[0] == 8 and _same_bits(ring_pos, held_pos)
    alone = rmsd_to_target(torch.stack(held_traj), target, S["batch"], atom_type=S["graph"][0])
    assert tuple(ring_run.rmsd_curve.shape) == (10, 6) and torch.equal(alone.cpu(), ring_run.rmsd_curve)
    # ... which differ from the unconstrained run's: the ring rows hold what the hold wrote
    assert not torch.equal(ring_run.rmsd_curve, S["TT"]._sampler_runs()["loose"][0].rmsd_curve)


def test_sampler_holds_with_counter_noise_and_without_a_trajectory():
    """noise_mode="counter" (no `noise` tensor), save_traj=False and no tracking: copy_out is null."""
    S = _sampler()
    at, bi, bt, ba = S["graph"]
    m = S["m"]
    ids = np.arange(S["G"], dtype=np.int64)
    p0 = m.counter_normals(S["b"]["batch"], ids, 5, [-1])[0]
    run = m.begin_sampling(at, p0, bi, bt, ba, S["G"], False, n_steps=4, w_global=1.0, global_start_sigma=0.5, clip=1000.0,
                           noise_mode="counter", noise_seed=5, stream_ids=ids, save_traj=False, **S["core"])
    run.advance(run.remaining())
    pos, traj = run.finish()
    assert traj == [] and _held_exactly(S, pos.cpu().numpy()) < TOL and torch.isfinite(run.core_dev).all()


# ---------------------------------------------------------------------------------------------------- 5. driver and command line
def test_run_job_holds_the_core_and_the_command_line_reproduces_it(tmp_path):
    from agdiff_amd import Config, driver, get_model, qm9_model_config, synth
    from oracle import agdiff_oracle as O
    cfg = qm9_model_config(num_diffusion_timesteps=8)
    sd = O.synth_state_dict_for(cfg)
    ckpt = str(tmp_path / "ckpt.pt")
    torch.save({"config": Config(model=cfg), "model": sd, "iteration": 0}, ckpt)
    m = get_model(cfg)
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    m = m.to("cuda:0").eval()
    rng = np.random.default_rng(5)
    mols = []
    for i, n in enumerate((13, 12, 9)):
        at, r, c, ty = synth.random_molecule(rng, n)
        mols.append(dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=ty, num_refs=2, name="mol%d" % i, index=i))
    heavy = np.nonzero(mols[1]["atom_type"] != 1)[0]
    assert heavy.size >= 4
    mask = np.zeros(12, dtype=bool)
    mask[heavy[:3]] = True
    mols[1]["core_pos"] = (C.walk(rng, 12) + 3.0).astype(np.float32)         # (off the origin: the template's frame is not the run's)
    mols[1]["core_mask"] = mask
    testset = str(tmp_path / "test.npz")
    driver.save_testset(testset, mols)
    mols = driver.load_testset(testset)
    kw = dict(n_steps=6, step_lr=1e-6, w_global=1.0, global_start_sigma=0.5, clip=1000.0)
    res = driver.run_job(m, mols, str(tmp_path / "held"), driver.num_confs("2"), 10 ** 6, kw, "cuda:0", log=lambda *_: None,
                         noise="counter", seed=2021, hold_core=True)
    got = res["pos_gen_1"]
    assert got.shape == (2, 12, 3) and got.dtype == np.float32
    err = float(np.abs(got[:, mask].astype(np.float64) - mols[1]["core_pos"][mask].astype(np.float64)[None]).max())
    print("hold_core run_job: core atoms of pos_gen_1 vs core_pos_1, max |coordinate err| %.2e (bar %.0e); core_rmsd_1 %s"
          % (err, TOL, res["core_rmsd_1"].tolist()))
    assert err < TOL                                                          # in the template's frame, coordinate by coordinate
    assert res["core_rmsd_1"].shape == (2,) and res["core_rmsd_1"].dtype == np.float32 and np.isfinite(res["core_rmsd_1"]).all()
    for i in (0, 2):
        assert "core_rmsd_%d" % i not in res and np.isfinite(res["pos_gen_%d" % i]).all()
    # the free atoms were sampled, not copied: the two conformers differ outside the core
    assert np.abs(got[0][~mask] - got[1][~mask]).max() > 1e-3
    # the same job from the command line, in a child process
    out = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "agdiff_amd.driver", "--ckpt", ckpt, "--testset", testset, "--out", out, "--num-confs", "2",
                        "--n-steps", "6", "--noise", "counter", "--seed", "2021", "--max-atoms", str(10 ** 6), "--hold-core"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    z = np.load(os.path.join(out, "samples_all.npz"))
    assert set(k for k in z.files if k.startswith("core_rmsd_")) == {"core_rmsd_1"}
    for key in ("pos_gen_0", "pos_gen_1", "pos_gen_2", "core_rmsd_1"):
        assert np.array_equal(z[key], res[key]), key
