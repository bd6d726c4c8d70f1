"""GPU (MI355X): distance restraints (csrc/eval.hip: agdiff_restrain_pairs; agdiff_amd/restraints.py; epsnet.LangevinRun with
restraint_pairs / _lo / _hi) against the float64 restatement tests/restraints_ref.py (anchored on the CPU in
tests/test_restraints_ref_cpu.py) at the project's RMSD bar of 2e-5 Angstrom absolute (tests/test_hip_core.py).  Beyond fp64
operation order the only sources of error are fp32 roundings of <= 1.9e-6 Angstrom each (|x| <= 32 Angstrom), one per sweep on
either side; the cases keep every restrained distance >= 0.1 Angstrom, so a rounding of one sweep enters the next one's direction
with a factor of order one, and three sweeps stay a factor of a few below the bar."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import restraints_ref as R
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


def _launch(pos, pairs, lo, hi, batch, **kw):
    """One stand-alone launch: (new pos, copy_out pre-filled with NaN, viol) on the host."""
    from agdiff_amd.restraints import restrain_pairs
    p = t(np.asarray(pos, dtype=np.float32)).cuda().contiguous()
    copy = torch.full_like(p, float("nan"))
    got, viol = restrain_pairs(p, pairs, lo, hi, batch, copy_out=copy, **kw)
    assert got.data_ptr() == p.data_ptr() and viol.dtype == torch.float32 and tuple(viol.shape) == (int(np.asarray(batch)[-1]) + 1,)
    return got.cpu(), copy.cpu(), viol.cpu()


_CASES, _REFS = {}, {}


def _case(family):
    if family not in _CASES:
        _CASES[family] = R.case(family)
    return _CASES[family]


def _ref(family, weight, sweeps, fixed):
    """The restatement's answer for a family and a setting, computed once (never modified)."""
    key = (family, weight, sweeps, fixed)
    if key not in _REFS:
        c = _case(family)
        _REFS[key] = R.restrain_pairs(c["pos"], c["pairs"], c["lo"], c["hi"], c["batch"], weight=weight, sweeps=sweeps,
                                      fixed=c["fixed"] if fixed else None)
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("sweeps", [1, 3])
@pytest.mark.parametrize("weight", [1.0, 0.5])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_against_the_restatement(family, weight, sweeps, fixed):
    c = _case(family)
    batch, rows = c["batch"], c["rows"]
    assert c["G"] == 7 and [int((rows[batch == g] > 0).sum()) for g in range(7)] == [0, 2, 2, 63, 64, 65, 129]
    assert rows[c["hub"]] == 70 and int((rows == 0).sum()) > 100
    kinds = set(c["kinds"])
    if family != "satisfied":
        assert {"above", "below", "inside", "inside, lower only", "inside, upper only", "below, lower only", "above, upper only"} <= kinds
    ref, ref_viol, written = _ref(family, weight, sweeps, fixed)
    got, copy, viol = _launch(c["pos"], c["pairs"], c["lo"], c["hi"], batch, weight=weight, sweeps=sweeps,
                              fixed=c["fixed"] if fixed else None)
    worst = float(np.abs(got.numpy().astype(np.float64) - ref.astype(np.float64)).max())
    worst_viol = float(np.abs(viol.numpy().astype(np.float64) - ref_viol).max())
    moved = float(np.abs(ref.astype(np.float64) - c["pos"]).max())
    print("restrain_pairs %-9s weight %.1f sweeps %d fixed %-5s: max |coordinate err| %.2e  max |viol err| %.2e (bar %.0e); largest move %.2f, "
          "largest viol %.2f" % (family, weight, sweeps, fixed, worst, worst_viol, TOL, moved, float(ref_viol.max())))
    assert worst < TOL and worst_viol < TOL
    free = np.nonzero(rows == 0)[0]
    assert _same_bits(got[free], c["pos"][free])                                          # atoms with an empty row keep their bits
    satisfied = [g for g in range(7) if ref_viol[g] == 0.0]
    assert 0 in satisfied and 1 in satisfied and (family != "satisfied" or len(satisfied) == 7)
    for g in satisfied:
        assert float(viol[g]) == 0.0 and _same_bits(got[batch == g], c["pos"][batch == g]), g    # ... as do all atoms of satisfied graphs
    if family != "satisfied":
        assert moved > 0.1 and (ref_viol[2:] > 0.01).all()
    with_row = np.nonzero(rows > 0)[0]
    assert written[with_row].all() and not written[free].any()
    assert _same_bits(copy[with_row], got[with_row]) and torch.isnan(copy[free]).all()   # copy_out: the new values, nothing else
    if fixed:
        held = np.nonzero(c["fixed"])[0]
        assert _same_bits(got[held], c["pos"][held])


# ---------------------------------------------------------------------------------------------------- 2. known answers
def test_known_answers_of_the_cpu_anchor():
    import test_restraints_ref_cpu as A
    assert A.KNOWN == ("upper bound", "fixed end", "lower bound", "inside")
    dist = lambda p: float(R.distances(p.numpy(), [[0, 1]])[0])
    pos, batch = A._two(5.0)
    got, copy, viol = _launch(pos, [[0, 1]], [0.0], [3.0], batch)                         # lands exactly on the upper bound
    mid = np.abs(got[:2].numpy().astype(np.float64).mean(0) - pos[:2].astype(np.float64).mean(0)).max()
    print("restrain_pairs known answers: d 5 -> %.7f (hi 3), centroid moved %.1e, viol %.7f" % (dist(got), mid, float(viol[0])))
    assert abs(dist(got) - 3.0) < TOL and mid < TOL and abs(float(viol[0]) - 2.0) < TOL and _same_bits(got[2], pos[2])
    assert torch.isnan(copy[2]).all() and _same_bits(copy[:2], got[:2])
    got, _, _ = _launch(pos, [[0, 1]], [0.0], [3.0], batch, fixed=[1, 0, 0])              # one end fixed: the other moves the whole 2
    assert _same_bits(got[0], pos[0]) and abs(float(np.linalg.norm(got[1].numpy().astype(np.float64) - pos[1])) - 2.0) < TOL
    assert abs(dist(got) - 3.0) < TOL
    got, _, _ = _launch(pos, [[0, 1]], [0.0], [3.0], batch, fixed=[1, 1, 0])
    assert _same_bits(got, pos)
    pos2, _ = A._two(2.0)
    got, _, viol = _launch(pos2, [[1, 0]], [3.5], [np.inf], batch)                        # a lower bound pushes apart
    assert abs(dist(got) - 3.5) < TOL and abs(float(viol[0]) - 1.5) < TOL
    pos4, _ = A._two(4.0)
    pos4[0, 0] = -0.0
    d = float(R.distances(pos4, [[0, 1]])[0])
    for lo, hi in ((0.7 * d, 1.3 * d), (0.0, np.inf), (d - 1e-3, d + 1e-3)):              # inside the window: the bytes stay
        got, copy, viol = _launch(pos4, [[0, 1]], [lo], [hi], batch, sweeps=3)
        assert _same_bits(got, pos4) and float(viol[0]) == 0.0 and _same_bits(copy[:2], pos4[:2])
    half, _, _ = _launch(pos, [[0, 1]], [0.0], [3.0], batch, weight=0.5)                  # w = 0.5: half as far
    assert abs(dist(half) - 4.0) < TOL
    twice, _, _ = _launch(pos, [[0, 1]], [0.0], [3.0], batch, weight=0.5, sweeps=2)       # two sweeps = two one-sweep calls
    again, _, _ = _launch(half.numpy(), [[0, 1]], [0.0], [3.0], batch, weight=0.5)
    assert _same_bits(twice, again) and abs(dist(twice) - 3.5) < TOL


# ---------------------------------------------------------------------------------------------------- 3. graphs that must not be written
def test_skipped_non_finite_and_coincident():
    c = _case("strong")
    batch, rows = c["batch"], c["rows"]
    args = (c["pairs"], c["lo"], c["hi"], batch)
    base_pos, base_copy, base_viol = _launch(c["pos"], *args)
    assert torch.isfinite(base_viol).all()
    restrained_of = lambda g: np.nonzero((batch == g) & (rows > 0))[0]
    cases = []
    skip = np.zeros(7, dtype=np.int32)
    skip[4] = 1
    cases.append(("skip", 4, dict(skip=skip), c["pos"]))
    pos = c["pos"].copy()
    pos[restrained_of(6)[100], 0] = np.nan               # an atom past the first 64-lane stride of its graph
    cases.append(("NaN in pos", 6, {}, pos))
    pos_inf = c["pos"].copy()
    pos_inf[restrained_of(3)[1], 1] = -np.inf
    cases.append(("inf in pos", 3, {}, pos_inf))
    for name, g, kw, given in cases:
        got, copy, viol = _launch(given, *args, **kw)
        here, others = np.nonzero(batch == g)[0], np.nonzero(batch != g)[0]
        assert _same_bits(got[here], given[here]), name                                   # the graph: bit for bit the input
        assert torch.isnan(copy[here]).all() and torch.isnan(viol[g]), name               # ... nothing of it in copy_out, viol NaN
        keep = [k for k in range(7) if k != g]
        assert _same_bits(got[others], base_pos[others]) and _same_bits(viol[keep], base_viol[keep]), name
        assert _same_bits(copy[others], base_copy[others]), name
    # a NaN in an UNRESTRAINED atom changes nothing
    pos = c["pos"].copy()
    lone = np.nonzero((batch == 6) & (rows == 0))[0][3]
    pos[lone] = np.nan
    got, copy, viol = _launch(pos, *args)
    rest = np.arange(c["N"]) != lone
    assert torch.isnan(got[lone]).all() and _same_bits(got[rest], base_pos[rest]) and _same_bits(viol, base_viol)
    # a coincident pair moves nothing (no direction), whatever its window says; its violation is still reported
    pos = c["pos"].copy()
    a, b = c["pairs"][np.nonzero(batch[c["pairs"][:, 0]] == 1)[0][0]]
    pos[b] = pos[a]
    got, _, viol = _launch(pos, [[a, b]], [1.0], [2.0], batch)
    assert _same_bits(got, pos) and float(viol[1]) == 1.0 and float(viol[0]) == 0.0
    # sweeps = 0 changes no byte and reports the same viol as a one-sweep call
    got, copy, viol = _launch(c["pos"], *args, sweeps=0)
    assert _same_bits(got, c["pos"]) and _same_bits(viol, base_viol) and torch.isnan(copy).all()
    # skip given as all zeros is no skip; no pairs at all: nothing moves, viol 0
    got, _, viol = _launch(c["pos"], *args, skip=np.zeros(7, dtype=np.int32))
    assert _same_bits(got, base_pos) and _same_bits(viol, base_viol)
    got, copy, viol = _launch(c["pos"], None, None, None, batch)
    assert _same_bits(got, c["pos"]) and (viol == 0).all() and torch.isnan(copy).all()


# ---------------------------------------------------------------------------------------------------- 4. sampler
_S = {}


def _sampler():
    """The set-up and the unconstrained runs of tests/test_hip_trajectory.py (`off`: fused front; `loose_off`: launch by launch).
    Restraints of every graph: its first and last atom pulled into [0.30, 0.35] Angstrom (no unrestrained conformer has them
    there), its second and second-to-last pushed beyond 8 Angstrom: two pairs without a common atom, so that a sweep at weight 1
    puts each pair onto its bound.  The restrained run with the trajectory kept is made once."""
    if not _S:
        import test_hip_trajectory as TT
        runs = TT._sampler_runs()
        m, b, graph, pos_init, noise, _ = runs["setup"]
        at, batch = graph[0].cpu().numpy(), np.asarray(b["batch"])
        N, G = at.shape[0], int(b["num_graphs"])
        pairs, lo, hi = [], [], []
        for g in range(G):
            idx = np.nonzero(batch == g)[0]
            assert idx.size >= 5
            pairs += [(idx[0], idx[-1]), (idx[-2], idx[1])]
            lo += [0.30, 8.0]
            hi += [0.35, np.inf]
        kw = dict(restraint_pairs=np.asarray(pairs, dtype=np.int32), restraint_lo=np.asarray(lo, dtype=np.float32),
                  restraint_hi=np.asarray(hi, dtype=np.float32))
        run = lambda **k: TT._run(m, b, graph, k.pop("pos_init", pos_init), noise, **k)
        _S.update(TT=TT, m=m, b=b, graph=graph, pos_init=pos_init, noise=noise, batch=batch, at=at, N=N, G=G, kw=kw, run=run,
                  fused=lambda r: TT._FUSED[id(r)], off=runs["off"], loose_off=runs["loose_off"],
                  table=(kw["restraint_pairs"], kw["restraint_lo"], kw["restraint_hi"], batch))
        _S["restrained"] = run(**kw)
    return _S


def _alone(S, frame, **kw):
    return _launch(frame.numpy() if torch.is_tensor(frame) else frame, *S["table"], **kw)


def test_sampler_first_step_is_the_update_then_the_launch():
    S = _sampler()
    run, pos, traj = S["restrained"]
    lo_traj = S["loose_off"][2]
    assert len(traj) == 10 and not S["fused"](run) and run.graph_steps == 0 and not run._use_graphs
    assert _same_bits(traj[0], _alone(S, lo_traj[0])[0]) and not _same_bits(traj[0], lo_traj[0])
    assert torch.equal(traj[-1], pos)                                                      # copy_out reached the last row too


def test_sampler_start_sigma_gates_and_the_closing_launch_always_runs():
    S = _sampler()
    lo_run, _, lo_traj = S["loose_off"]
    sig = [s[0] for s in lo_run._sched]
    assert len(sig) == 10 and all(a > b_ for a, b_ in zip(sig, sig[1:]))
    k0 = 4
    start = 0.5 * (sig[k0 - 1] + sig[k0])                  # between two sigmas of the schedule: step k0 is the first one restrained
    run, pos, traj = S["run"](restraint_start_sigma=start, **S["kw"])
    assert not S["fused"](run)
    for k in range(k0):
        assert _same_bits(traj[k], lo_traj[k]), k
    assert _same_bits(traj[k0], _alone(S, lo_traj[k0])[0]) and not _same_bits(traj[k0], lo_traj[k0])
    assert torch.equal(traj[-1], pos)
    # a start sigma below the whole schedule: only the closing launch runs
    run, pos, traj = S["run"](restraint_start_sigma=0.5 * sig[-1], **S["kw"])
    assert all(_same_bits(traj[k], lo_traj[k]) for k in range(9))
    assert _same_bits(traj[9], _alone(S, lo_traj[9])[0]) and _same_bits(pos, traj[9]) and not _same_bits(pos, lo_traj[9])
    assert torch.isfinite(run.restraint_viol).all()


def test_sampler_without_pairs_is_what_it_was():
    """No keywords, or an empty pair list: the run of today, fused front included, bit for bit -- and with it the launch-by-launch
    run's result, which tests/test_hip_trajectory.py::test_final_positions_agree_across_the_two_fronts ties to the fused one."""
    S = _sampler()
    off_run, off_pos, off_traj = S["off"]
    lo_pos = S["loose_off"][1]
    empty = dict(restraint_pairs=np.zeros((0, 2), dtype=np.int32), restraint_lo=np.zeros(0, dtype=np.float32),
                 restraint_hi=np.zeros(0, dtype=np.float32))
    for kw in ({}, empty, dict(restraint_pairs=[], restraint_lo=[], restraint_hi=[], restraint_weight=0.5, restraint_sweeps=3)):
        run, pos, traj = S["run"](**kw)
        assert S["fused"](run) and S["fused"](off_run) and run.graph_steps == off_run.graph_steps and run._use_graphs == off_run._use_graphs
        assert run.restraint_viol is None
        assert _same_bits(pos, off_pos) and len(traj) == 10 and all(_same_bits(a, b_) for a, b_ in zip(traj, off_traj))
        assert _same_bits(pos, lo_pos)


def test_sampler_restrained_run_differs_and_violates_less():
    """Fails on a sampler that swallows the keywords: the run would be the unrestrained one."""
    S = _sampler()
    run, pos, traj = S["restrained"]
    off_pos = S["off"][1]
    assert not _same_bits(pos, off_pos)
    viol = run.restraint_viol
    assert viol is not None and viol.dtype == torch.float32 and tuple(viol.shape) == (6,) and not viol.is_cuda
    measured = _alone(S, pos, sweeps=0)[2]
    assert _same_bits(viol, measured)                                                      # = a measuring launch on what the run returned
    free = _alone(S, off_pos, sweeps=0)[2]
    print("restrain_pairs sampler: largest violation per graph, unrestrained %s, restrained %s" % (free.tolist(), viol.tolist()))
    assert (free > 0.1).all() and (viol < free).all()
    assert (viol < 1e-4).all()               # pairs without a common atom, weight 1: the closing launch puts each onto its bound


def test_sampler_weight_and_sweeps_reach_the_launch():
    S = _sampler()
    lo_traj = S["loose_off"][2]
    run, pos, traj = S["run"](restraint_weight=0.5, restraint_sweeps=3, **S["kw"])
    assert _same_bits(traj[0], _alone(S, lo_traj[0], weight=0.5, sweeps=3)[0])
    assert not _same_bits(traj[0], S["restrained"][2][0]) and (run.restraint_viol > 1e-4).any()     # soft: not forced at the end


def _core(S):
    """test_hip_core's core of every graph: its first ceil(heavy / 2) heavy atoms, template = a walk per graph; and one restraint
    per graph between the first core atom and the last atom outside the core."""
    import core_ref as C
    rng = np.random.default_rng(17)
    select, template = np.zeros(S["N"], dtype=bool), np.zeros((S["N"], 3), dtype=np.float32)
    pairs = []
    for g in range(S["G"]):
        idx = np.nonzero(S["batch"] == g)[0]
        heavy = idx[S["at"][idx] != 1]
        select[heavy[:(heavy.size + 1) // 2]] = True
        template[idx] = C.walk(rng, idx.size).astype(np.float32)
        pairs.append((idx[select[idx]][0], idx[~select[idx]][-1]))
    return select, template, np.asarray(pairs, dtype=np.int32)


def test_sampler_with_a_core_held_as_well():
    from oracle.covmat_oracle import kabsch_rmsd
    S = _sampler()
    select, template, pairs = _core(S)
    core = dict(core_pos=template, core_select=select)
    lo, hi = np.full(S["G"], 0.30, dtype=np.float32), np.full(S["G"], 0.35, dtype=np.float32)
    only_run, only_pos, only_traj = S["run"](**core)
    run, pos, traj = S["run"](restraint_pairs=pairs, restraint_lo=lo, restraint_hi=hi, **core)
    assert not S["fused"](run) and torch.isfinite(run.core_dev).all() and torch.isfinite(run.restraint_viol).all()
    worst = max(kabsch_rmsd(pos.numpy().astype(np.float64)[(S["batch"] == g) & select], template[(S["batch"] == g) & select])
                for g in range(S["G"]))
    print("restrain_pairs sampler + core: largest core RMSD to the template %.2e (bar %.0e); viol %s" % (worst, TOL, run.restraint_viol.tolist()))
    assert worst < TOL                                                                     # the core is exact
    # first frame: the update, the restraint launch with the core fixed, then the hold
    from agdiff_amd.core import hold_core
    lo_traj = S["loose_off"][2]
    step = _launch(lo_traj[0].numpy(), pairs, lo, hi, S["batch"], fixed=select)[0]
    assert _same_bits(step[select], lo_traj[0][select])                                    # fixed: the core atoms wait for the hold
    held, _ = hold_core(step.cuda().contiguous(), template, select, S["batch"])
    assert _same_bits(traj[0], held.cpu())
    partner = pairs[:, 1]
    assert (np.abs(pos.numpy()[partner] - only_pos.numpy()[partner]).max(axis=1) > 1e-3).all()     # the free partners have moved
    before = _launch(only_pos.numpy(), pairs, lo, hi, S["batch"], sweeps=0)[2]
    assert (run.restraint_viol < before).all()


def test_sampler_leaves_a_quarantined_graph_alone():
    S = _sampler()
    bad_init = S["pos_init"].clone()
    bad_init[int(np.nonzero(S["batch"] == 2)[0][1]), 0] = float("nan")
    run, pos, _ = S["run"](pos_init=bad_init, raise_on_nan=False, **S["kw"])
    S["m"].fused_front = False
    try:
        free_run, free_pos, _ = S["run"](pos_init=bad_init, raise_on_nan=False)
    finally:
        S["m"].fused_front = True
    assert run.nan_graphs().tolist() == [False, False, True, False, False, False] == free_run.nan_graphs().tolist()
    rows = np.nonzero(S["batch"] == 2)[0]
    assert _same_bits(pos[rows], free_pos[rows])                                           # the placeholder: as without restraints
    assert torch.isnan(run.restraint_viol[2]) and (run.restraint_viol[[0, 1, 3, 4, 5]] < 1e-4).all()


def test_sampler_restrains_with_counter_noise_and_without_a_trajectory():
    """noise_mode="counter" (no `noise` tensor), save_traj=False and no tracking: copy_out is null."""
    S = _sampler()
    at, bi, bt, ba = S["graph"]
    m = S["m"]
    ids = np.arange(S["G"], dtype=np.int64)
    p0 = m.counter_normals(S["b"]["batch"], ids, 5, [-1])[0]
    run = m.begin_sampling(at, p0, bi, bt, ba, S["G"], False, n_steps=4, w_global=1.0, global_start_sigma=0.5, clip=1000.0,
                           noise_mode="counter", noise_seed=5, stream_ids=ids, save_traj=False, **S["kw"])
    run.advance(run.remaining())
    pos, traj = run.finish()
    assert traj == [] and torch.isfinite(pos).all() and (run.restraint_viol < 1e-4).all()


# ---------------------------------------------------------------------------------------------------- 5. job function and command line
def test_sample_restrained_and_the_command_line(tmp_path):
    from agdiff_amd import Config, driver, get_model, qm9_model_config, restraints, synth
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
    for i, n in enumerate((12, 9)):
        at, r, c, ty = synth.random_molecule(rng, n)
        mols.append(dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=ty, num_refs=2, name="mol%d" % i, index=i))
    plain, testset = str(tmp_path / "plain.npz"), str(tmp_path / "test.npz")
    driver.save_testset(plain, mols)
    given = {0: ([[0, 11], [10, 1]], [0.30, 8.0], [0.35, np.inf])}
    restraints.add_restraints(plain, testset, given)
    mols = driver.load_testset(testset)
    mols[0]["restr_pairs"], mols[0]["restr_lo"], mols[0]["restr_hi"] = restraints.load_restraints(testset)[0]
    kw = dict(n_steps=6, step_lr=1e-6, w_global=1.0, global_start_sigma=0.5, clip=1000.0)
    quiet = lambda *_: None
    res = [restraints.sample_restrained(m, mol, 2, kw, "cuda:0", counter_seed=2021, log=quiet) for mol in mols]
    pos0, viol0, ok0 = res[0]
    assert ok0 and res[1][2] and pos0.shape == (2, 12, 3) and pos0.dtype == np.float32 and viol0.dtype == np.float32 and viol0.shape == (2,)
    assert (viol0 < 1e-4).all() and np.array_equal(res[1][1], np.zeros(2, dtype=np.float32)) and np.isfinite(res[1][0]).all()
    # the same draws through begin_sampling
    packed = driver.pack_batch([mols[0]], lambda _: 2)
    pr, lo, hi = restraints.pack_restraints(packed, [given[0]])
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p0 = m.counter_normals(packed["batch"], packed["stream_ids"], 2021, [-1])[0]
    run = m.begin_sampling(T(packed["atom_type"]), p0, T(packed["bond_index"]), T(packed["bond_type"]), T(packed["batch"]), 2, False,
                           raise_on_nan=False, save_traj=False, noise_mode="counter", noise_seed=2021, stream_ids=packed["stream_ids"],
                           restraint_pairs=pr, restraint_lo=lo, restraint_hi=hi, **kw)
    run.advance(run.remaining())
    direct = run.finish()[0].cpu().numpy().reshape(2, 12, 3)
    assert np.array_equal(direct, pos0) and np.array_equal(run.restraint_viol.numpy(), viol0)
    # unrestrained, the same molecule comes out elsewhere, and outside its windows
    free, _, _ = restraints.sample_restrained(m, {k: v for k, v in mols[0].items() if not k.startswith("restr_")}, 2, kw, "cuda:0",
                                              counter_seed=2021, log=quiet)
    assert not np.array_equal(free, pos0) and (restraints.measure(free, given[0]) > 0.1).all()
    # the command line, in a child process: the same job bit for bit
    out = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "agdiff_amd.restraints", "--ckpt", ckpt, "--testset", testset, "--out", out, "--num-confs", "2",
                        "--n-steps", "6", "--noise", "counter", "--seed", "2021"], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    samples = os.path.join(out, "samples_all.npz")
    z = np.load(samples)
    assert set(z.files) == {"pos_gen_0", "name_0", "restr_viol_0", "pos_gen_1", "name_1", "restr_viol_1"}
    for i in range(2):
        assert np.array_equal(z["pos_gen_%d" % i], res[i][0]) and np.array_equal(z["restr_viol_%d" % i], res[i][1]), i
    # report mode measures the finished job (in this process), and the validity module accepts the file
    rep = restraints.main(["--report", "--samples", samples, "--testset", testset, "--out", str(tmp_path / "viol.npz")])
    assert np.array_equal(rep["restr_viol_0"], viol0) and np.array_equal(rep["restr_viol_1"], np.zeros(2, dtype=np.float32))
    assert set(np.load(str(tmp_path / "viol.npz")).files) == {"restr_viol_0", "restr_viol_1"}
    from agdiff_amd import validity                      # (python -m agdiff_amd.validity's main, without another process)
    verdicts = validity.main(["--samples", samples, "--testset", testset, "--out", str(tmp_path / "valid.npz")])
    assert verdicts["valid_0"].shape == (2,) and verdicts["valid_1"].shape == (2,)
