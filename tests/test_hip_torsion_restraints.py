"""GPU (MI355X): torsion restraints (csrc/eval.hip: agdiff_restrain_torsions; agdiff_amd/torsion_restraints.py; epsnet.LangevinRun
with torsion_quads / _target / _tol) against the float64 restatement tests/torsion_restraints_ref.py (anchored on the CPU in
tests/test_torsion_restraints_ref_cpu.py) at the project's bar of 2e-5 Angstrom absolute (tests/test_hip_core.py,
tests/test_hip_restraints.py).

Why the bar holds for these cases.  Kernel and restatement compute in fp64 from the same fp32 inputs, so after ONE rotation they can
differ only where the last fp64 bits decide an fp32 rounding: by at most one fp32 step u (u = 2^-23 = 1.2e-7 Angstrom, every
|coordinate| < 2).  A later rotation that reads atoms which are off by d on one side is off itself: its measured angle by at most
3 d / l (the moved quad atoms v and b, each displaced by d, over a lever arm l: the smallest distance of a or b from the axis, or
the axis length), its axis direction by d / l, its pivot by d.  An atom within D of the pivot is then displaced by at most
D (3 d / l) + 2 D (d / l) + 2 d, and rounded once more: d' <= (5 D / l + 2) d + u.  The generator asserts |x| <= 2, l >= 1.25,
D <= 2 and that no atom turns more than three times, so d1 = u, d2 = 11 u, d3 = 111 u = 1.3e-5 Angstrom < 2e-5
(torsion_restraints_ref.error_bound; asserted below).  Angles and violations of the measure pass come from identical inputs: only
libm's atan2 and the final rounding differ, one fp32 step at pi, 2.4e-7 rad."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import torsion_restraints_ref as R
from helpers import t
from test_torsion_restraints_cpu import usable_bridges

pytestmark = pytest.mark.gpu

TOL = 2e-5
ANGLE_TOL = 2.4e-7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    """int32 view of a float32 tensor / array on the host: equality of these is equality bit for bit, NaNs included."""
    x = x.detach().cpu() if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _launch(pos, quads, target, tol, batch, sides, **kw):
    """One stand-alone launch: (new pos, copy_out pre-filled with NaN, angle, viol) on the host."""
    from agdiff_amd.torsion_restraints import restrain_torsions
    p = t(np.asarray(pos, dtype=np.float32)).cuda().contiguous()
    copy = torch.full_like(p, float("nan"))
    got, angle, viol = restrain_torsions(p, quads, target, tol, batch, sides, copy_out=copy, **kw)
    assert got.data_ptr() == p.data_ptr() and viol.dtype == angle.dtype == torch.float32
    assert tuple(viol.shape) == (int(np.asarray(batch)[-1]) + 1,) and tuple(angle.shape) == (0 if quads is None else len(quads),)
    return got.cpu(), copy.cpu(), angle.cpu(), viol.cpu()


_CASES, _REFS = {}, {}


def _case(family):
    if family not in _CASES:
        _CASES[family] = R.case(family)
    return _CASES[family]


def _args(c):
    return c["quads"], c["centre"], c["half"], c["batch"], c["sides"]


def _ref(family, weight, turn=True):
    """The restatement's answer for a family and a setting, computed once (never modified)."""
    key = (family, weight, turn)
    if key not in _REFS:
        c = _case(family)
        _REFS[key] = R.restrain_torsions(c["pos"], c["quads"], c["centre"], c["half"], c["batch"], *c["sides"], weight=weight, turn=turn)
    return _REFS[key]


def _levers(pos, quads):
    """The smallest lever arm of the quads in pos (float64): distance of a and of b from the axis, and the axis length."""
    p = np.asarray(pos, dtype=np.float64)
    out = []
    for a, u, v, b in np.asarray(quads).reshape(-1, 4).tolist():
        out += [R.lever_arm(p, a, u, v), R.lever_arm(p, b, u, v), float(np.linalg.norm(p[v] - p[u]))]
    return min(out)


def _angle_bound(pos, quads, roundings=2):
    """Bound on how far a dihedral of `quads` in the fp32 positions `pos` lies from where fp64 put it: each of its four atoms
    displaced by `roundings` half-steps of fp32 at the largest coordinate, over the smallest lever arm, + the fp32 step of the angle."""
    step = float(np.spacing(np.float32(np.abs(np.asarray(pos, dtype=np.float64)).max())))
    return 4.0 * roundings * 0.5 * np.sqrt(3.0) * step / _levers(pos, quads) + ANGLE_TOL


def _left_bound(pos, quads):
    """What a closing launch at weight 1 may leave of a restraint (test_sampler_restrained_run_differs_and_violates_less): twice
    _angle_bound with one rounding."""
    return 2.0 * _angle_bound(pos, quads, roundings=1)


# ---------------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("weight", [1.0, 0.5])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_against_the_restatement(family, weight):
    c = _case(family)
    batch, quads = c["batch"], c["quads"]
    assert c["G"] == 7 and c["T"] == 14 and R.error_bound(c) < TOL
    assert (c["x_max"], c["depth"]) <= (R.X_MAX, R.DEPTH_MAX) and c["l_min"] >= R.L_MIN and c["d_max"] <= R.D_MAX
    ref, ref_angle, ref_viol, written = _ref(family, weight)
    _, ref_angle0, ref_viol0, _ = _ref(family, weight, turn=False)
    got, copy, angle, viol = _launch(c["pos"], *_args(c), weight=weight)
    same, copy0, angle0, viol0 = _launch(c["pos"], *_args(c), weight=weight, turn=False)
    worst = float(np.abs(got.numpy().astype(np.float64) - ref.astype(np.float64)).max())
    worst_viol = float(np.abs(viol.numpy().astype(np.float64) - ref_viol).max())
    worst_angle0 = float(np.abs(angle0.numpy().astype(np.float64) - ref_angle0).max())
    worst_angle = float(np.abs(R.wrap(angle.numpy().astype(np.float64) - ref_angle)).max())
    moved = float(np.abs(ref.astype(np.float64) - c["pos"]).max())
    print("restrain_torsions %-9s weight %.1f: max |coordinate err| %.2e (bar %.0e, derived bound %.2e)  max |viol err| %.2e  max |angle err| "
          "measured %.2e, at its turn %.2e (bar %.1e); largest move %.2f A, largest viol %.3f rad, %d atoms differ in a bit"
          % (family, weight, worst, TOL, R.error_bound(c), worst_viol, worst_angle0, worst_angle, ANGLE_TOL, moved, float(ref_viol.max()),
             int((_bits(got) != _bits(ref)).any(dim=1).sum())))
    assert worst < TOL
    assert worst_viol <= ANGLE_TOL and worst_angle0 <= ANGLE_TOL
    first_turn = np.array([c["turns"][q[3]] <= 1 for q in quads])           # restraints no earlier turn has touched
    assert np.abs(R.wrap(angle.numpy().astype(np.float64) - ref_angle))[first_turn].max() <= ANGLE_TOL
    assert worst_angle <= 3.0 * R.error_bound(c) / R.L_MIN + ANGLE_TOL
    # turn = 0 writes nothing and reports the same viol as a turning call
    assert _same_bits(same, c["pos"]) and torch.isnan(copy0).all() and _same_bits(viol0, viol)
    # what must keep its bits
    free = np.nonzero(~c["in_row"])[0]
    assert free.size > 80 and _same_bits(got[free], c["pos"][free])                       # atoms in no side row
    still = np.nonzero(c["turns"] == 0)[0]
    assert _same_bits(got[still], c["pos"][still])                                       # ... and the sides of satisfied restraints
    axis = np.unique(quads[:, 1:3].reshape(-1))
    axis = axis[c["turns"][axis] == 0]                                                    # u, v that no OTHER restraint turns
    assert {int(quads[0, 1]), int(quads[0, 2]), int(quads[11, 1]), int(quads[11, 2])} <= set(axis.tolist())
    assert _same_bits(got[axis], c["pos"][axis])
    satisfied = [g for g in range(7) if ref_viol[g] == 0.0]
    assert 0 in satisfied and (family != "satisfied" or len(satisfied) == 7)
    for g in satisfied:
        assert float(viol[g]) == 0.0 and _same_bits(got[batch == g], c["pos"][batch == g]), g    # whole satisfied graphs
    if family == "satisfied":
        assert _same_bits(got, c["pos"]) and torch.isnan(copy).all() and (viol == 0).all()       # no byte may change
    else:
        assert moved > 0.3 and (ref_viol[1:] > 0.3).all() and int(written.sum()) > 300
    # copy_out: exactly the stored values
    w = np.nonzero(written)[0]
    assert np.array_equal(written, c["turns"] > 0)
    assert _same_bits(copy[w], got[w]) and torch.isnan(copy[np.nonzero(~written)[0]]).all()


# ---------------------------------------------------------------------------------------------------- 2. graphs that must not be written
def test_left_alone():
    c = _case("violated")
    batch, quads, first = c["batch"], c["quads"], c["first"]
    base_pos, base_copy, base_angle, base_viol = _launch(c["pos"], *_args(c))
    assert torch.isfinite(base_viol).all() and torch.isfinite(base_angle).all()
    rows_of = lambda g: np.nonzero(batch[quads[:, 1]] == g)[0]
    cases = []
    skip = np.zeros(7, dtype=np.int32)
    skip[4] = 1
    cases.append(("skip", 4, dict(skip=skip), c["pos"]))
    pos = c["pos"].copy()
    b6 = int(quads[rows_of(6)[-1], 3])                   # b of graph 6's last quad ...
    pos[b6, 0] = np.nan
    cases.append(("NaN in a quad atom", 6, {}, pos))
    pos_inf = c["pos"].copy()
    pos_inf[int(quads[rows_of(3)[0], 1]), 1] = -np.inf
    cases.append(("inf in a quad atom", 3, {}, pos_inf))
    # ... and a graph whose quad list runs past lane 64: 70 measuring restraints on graph 5, the NaN in the last one's atom
    many = np.repeat(quads[rows_of(5)], 70, axis=0)
    q_many = np.concatenate([quads[:rows_of(5)[0]], many, quads[rows_of(5)[-1] + 1:]])
    grow = lambda x, fill=None: np.concatenate([x[:rows_of(5)[0]], np.repeat(x[rows_of(5)], 70) if fill is None else np.full(70, fill, x.dtype),
                                                x[rows_of(5)[-1] + 1:]])
    sides_many = (grow(c["side_row"], -1), c["side_ptr"], c["side_idx"])
    q_many[rows_of(5)[0] + 69] = [first[5] + 4, first[5] + 1, first[5] + 2, first[5] + 3]           # (another a: a blob atom)
    args_many = (q_many, grow(c["centre"]), grow(c["half"]), batch, sides_many)
    many_pos, _, many_angle, many_viol = _launch(c["pos"], *args_many)
    assert many_angle.shape[0] == c["T"] + 69 and torch.isfinite(many_angle).all() and _same_bits(many_pos[batch == 5], c["pos"][batch == 5])
    pos_far = c["pos"].copy()
    pos_far[first[5] + 4, 2] = np.nan
    got, copy, angle, viol = _launch(pos_far, *args_many)
    assert torch.isnan(viol[5]) and torch.isnan(angle[rows_of(5)[0]:rows_of(5)[0] + 70]).all() and _same_bits(got[batch != 5], many_pos[batch != 5])
    assert _same_bits(viol[[0, 1, 2, 3, 4, 6]], many_viol[[0, 1, 2, 3, 4, 6]])
    for name, g, kw, given in cases:
        got, copy, angle, viol = _launch(given, *_args(c), **kw)
        here, others = np.nonzero(batch == g)[0], np.nonzero(batch != g)[0]
        assert _same_bits(got[here], given[here]), name                                   # the graph: bit for bit the input
        assert torch.isnan(copy[here]).all() and torch.isnan(viol[g]) and torch.isnan(angle[rows_of(g)]).all(), name
        keep = [k for k in range(7) if k != g]
        other_rows = np.nonzero(batch[quads[:, 1]] != g)[0]
        assert _same_bits(got[others], base_pos[others]) and _same_bits(viol[keep], base_viol[keep]), name
        assert _same_bits(copy[others], base_copy[others]) and _same_bits(angle[other_rows], base_angle[other_rows]), name
    # a NaN in a SIDE atom that is in no quad: that atom stays, the rest turn as before
    pos = c["pos"].copy()
    lone = int(first[4] + 40)
    assert c["turns"][lone] == 1 and lone not in quads
    pos[lone, 1] = np.nan
    got, copy, angle, viol = _launch(pos, *_args(c))
    rest = np.arange(c["N"]) != lone
    assert _same_bits(got[lone], pos[lone]) and torch.isnan(copy[lone]).all()
    assert _same_bits(got[rest], base_pos[rest]) and _same_bits(viol, base_viol) and _same_bits(angle, base_angle)
    # a collinear quad: angle NaN, nothing moved, viol unaffected
    pos = c["pos"].copy()
    a, u, v, b = quads[rows_of(1)[0]]
    pos[a] = pos[v]                                      # b1 = -b2 exactly: n1 = 0
    got, copy, angle, viol = _launch(pos, *_args(c))
    g1 = np.nonzero(batch == 1)[0]
    assert torch.isnan(angle[rows_of(1)[0]]) and _same_bits(got[g1], pos[g1]) and float(viol[1]) == 0.0
    assert _same_bits(got[batch != 1], base_pos[batch != 1]) and _same_bits(viol[[0, 2, 3, 4, 5, 6]], base_viol[[0, 2, 3, 4, 5, 6]])
    # side_row = -1: measured, not moved -- and a quad that names an atom of another graph is degenerate and reads nothing
    row = c["side_row"].copy()
    row[rows_of(3)[0]] = -1
    got, copy, angle, viol = _launch(c["pos"], *_args(c)[:4], (row, c["side_ptr"], c["side_idx"]))
    g3 = np.nonzero(batch == 3)[0]
    assert _same_bits(got[g3], c["pos"][g3]) and _same_bits(viol, base_viol) and _same_bits(angle, base_angle) and torch.isnan(copy[g3]).all()
    assert _same_bits(got[batch != 3], base_pos[batch != 3])
    got, _, angle, viol = _launch(c["pos"], *_args(c)[:4], None)                          # no sides at all: the measuring launch
    assert _same_bits(got, c["pos"]) and _same_bits(viol, base_viol)
    got, copy, angle, viol = _launch(c["pos"], None, None, None, batch, None)
    assert _same_bits(got, c["pos"]) and (viol == 0).all() and torch.isnan(copy).all()
    got, _, _, viol = _launch(c["pos"], *_args(c), skip=np.zeros(7, dtype=np.int32))     # all zeros is no skip
    assert _same_bits(got, base_pos) and _same_bits(viol, base_viol)


# ---------------------------------------------------------------------------------------------------- 3. known answer
def test_alanine_dipeptide_turned_to_phi_psi():
    """phi = (4, 6, 8, 14) and psi = (6, 8, 14, 16) of ACE-ALA-NME from a random geometry to (-60, -45) degrees with tol 0: both
    on target when re-measured by agdiff_torsion_angles, within _angle_bound -- every quad atom has passed through at most two
    fp32 roundings (phi's turn, psi's turn), each half a step of the largest coordinate, over the smallest lever arm --, and every
    bond length kept to 2e-5 Angstrom."""
    from agdiff_amd import synth
    from agdiff_amd.torsion_restraints import batch_sides
    from agdiff_amd.torsions import torsion_angles
    d = synth.alanine_dipeptide(1)
    n = int(d["atom_type"].shape[0])
    quads = np.array([[4, 6, 8, 14], [6, 8, 14, 16]], dtype=np.int32)
    target = np.deg2rad([-60.0, -45.0]).astype(np.float32)
    pos = (np.random.default_rng(3).normal(size=(n, 3)) * 1.5).astype(np.float32)
    assert _levers(pos, quads) > 1.0
    oq, sides = batch_sides(n, d["bond_index"], d["bond_type"], d["batch"], quads)
    assert oq.tolist() == [[14, 8, 6, 4], [6, 8, 14, 16]] and sides[0].tolist() == [0, 1]            # phi is turned on its N-terminal side
    got, copy, angle, viol = _launch(pos, oq, target, np.zeros(2, dtype=np.float32), d["batch"], sides)
    before = R.dihedral(pos, quads)
    assert float(viol[0]) > 0.5 and abs(float(viol[0]) - float(np.abs(R.wrap(before - target)).max())) < 1e-6
    after = torsion_angles(got.reshape(1, n, 3).cuda().contiguous(), quads).cpu().numpy()[0].astype(np.float64)
    bound = _angle_bound(got.numpy(), quads)
    err = np.abs(R.wrap(after - target.astype(np.float64)))
    print("restrain_torsions alanine dipeptide: phi, psi %s -> %s degrees, |error| %s rad (bound %.2e)"
          % (np.rad2deg(before).round(2).tolist(), np.rad2deg(after).round(4).tolist(), err.tolist(), bound))
    assert bound < 5e-6 and (err <= bound).all()
    bi = np.asarray(d["bond_index"])[:, np.asarray(d["bond_type"]) < 22]
    length = lambda p: np.linalg.norm(np.asarray(p, dtype=np.float64)[bi[0]] - np.asarray(p, dtype=np.float64)[bi[1]], axis=1)
    assert bi.shape[1] == 42 and np.abs(length(got.numpy()) - length(pos)).max() < TOL


# ---------------------------------------------------------------------------------------------------- 4. sampler
_S = {}
TARGET, WINDOW = 1.0, 0.25


def _sampler():
    """The set-up and the unconstrained runs of tests/test_hip_trajectory.py (`off`: fused front; `loose_off`: launch by launch).
    One restraint per graph, target 1.0 +- 0.25 rad, on that usable bridge of the graph (a bridge with a neighbour on both ends:
    every graph has at least 10) whose dihedral in the unrestrained result lies furthest outside the window.  The restrained run
    with the trajectory kept is made once."""
    if not _S:
        import test_hip_trajectory as TT
        from agdiff_amd.torsion_restraints import batch_sides
        runs = TT._sampler_runs()
        m, b, graph, pos_init, noise, _ = runs["setup"]
        at, batch = graph[0].cpu().numpy(), np.asarray(b["batch"])
        bi, bt = np.asarray(b["bond_index"]), np.asarray(b["bond_type"])
        N, G = at.shape[0], int(b["num_graphs"])
        off_pos = runs["off"][1].numpy()
        quads, bridges_of = [], []
        for g in range(G):
            idx = np.nonzero(batch == g)[0]
            own = (bi[0] >= idx[0]) & (bi[0] <= idx[-1])
            qs = np.asarray(usable_bridges(dict(atom_type=at[idx], edge_index=bi[:, own] - idx[0], edge_type=bt[own]))) + idx[0]
            assert len(qs) >= 10
            out = np.abs(R.excess(R.dihedral(off_pos, qs), TARGET, WINDOW))
            quads.append(qs[int(np.argmax(out))])
            bridges_of.append(qs)
        quads = np.asarray(quads, dtype=np.int32)
        kw = dict(torsion_quads=quads, torsion_target=np.full(G, TARGET, dtype=np.float32), torsion_tol=np.full(G, WINDOW, dtype=np.float32))
        oq, sides = batch_sides(N, bi, bt, batch, quads)
        run = lambda **k: TT._run(m, b, graph, k.pop("pos_init", pos_init), noise, **k)
        _S.update(TT=TT, m=m, b=b, graph=graph, pos_init=pos_init, noise=noise, batch=batch, at=at, N=N, G=G, kw=kw, run=run, bi=bi, bt=bt,
                  fused=lambda r: TT._FUSED[id(r)], off=runs["off"], loose_off=runs["loose_off"], quads=quads, bridges_of=bridges_of,
                  table=(oq, kw["torsion_target"], kw["torsion_tol"], batch, sides))
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
    run, pos, traj = S["run"](torsion_start_sigma=start, **S["kw"])
    assert not S["fused"](run)
    for k in range(k0):
        assert _same_bits(traj[k], lo_traj[k]), k
    assert _same_bits(traj[k0], _alone(S, lo_traj[k0])[0]) and not _same_bits(traj[k0], lo_traj[k0])
    assert torch.equal(traj[-1], pos)
    # a start sigma below the whole schedule: only the closing launch runs
    run, pos, traj = S["run"](torsion_start_sigma=0.5 * sig[-1], **S["kw"])
    assert all(_same_bits(traj[k], lo_traj[k]) for k in range(9))
    assert _same_bits(traj[9], _alone(S, lo_traj[9])[0]) and _same_bits(pos, traj[9]) and not _same_bits(pos, lo_traj[9])
    assert torch.isfinite(run.torsion_viol).all() and torch.isfinite(run.torsion_angle).all()


def test_sampler_without_quads_is_what_it_was():
    """No keywords, or an empty quad list: the run of today, fused front included, bit for bit."""
    S = _sampler()
    off_run, off_pos, off_traj = S["off"]
    lo_pos = S["loose_off"][1]
    empty = dict(torsion_quads=np.zeros((0, 4), dtype=np.int32), torsion_target=np.zeros(0, dtype=np.float32),
                 torsion_tol=np.zeros(0, dtype=np.float32))
    for kw in ({}, empty, dict(torsion_quads=[], torsion_target=[], torsion_tol=[], torsion_weight=0.5, torsion_start_sigma=0.3)):
        run, pos, traj = S["run"](**kw)
        assert S["fused"](run) and S["fused"](off_run) and run.graph_steps == off_run.graph_steps and run._use_graphs == off_run._use_graphs
        assert run.torsion_viol is None and run.torsion_angle is None
        assert _same_bits(pos, off_pos) and len(traj) == 10 and all(_same_bits(a, b_) for a, b_ in zip(traj, off_traj))
        assert _same_bits(pos, lo_pos)


def test_sampler_restrained_run_differs_and_violates_less():
    """Fails on a sampler that swallows the keywords: the run would be the unrestrained one.  The bound on what is left: the closing
    launch turns at weight 1 onto the window's edge in fp64 and rounds every turned atom to fp32 once, so each of a quad's four atoms
    is off by at most half an fp32 step of the largest coordinate per axis, and the dihedral by 4 x sqrt(3)/2 steps over the smallest
    lever arm (distance of a or b from the axis, or the axis length), + the fp32 step of the angle itself: _angle_bound with one
    rounding, computed in float64 from the returned positions; the test allows twice that."""
    S = _sampler()
    run, pos, traj = S["restrained"]
    off_pos = S["off"][1]
    assert not _same_bits(pos, off_pos)
    viol, angle = run.torsion_viol, run.torsion_angle
    assert viol is not None and viol.dtype == torch.float32 and tuple(viol.shape) == (6,) and not viol.is_cuda
    assert angle.dtype == torch.float32 and tuple(angle.shape) == (6,) and not angle.is_cuda
    _, _, m_angle, m_viol = _alone(S, pos, turn=False)
    assert _same_bits(viol, m_viol) and _same_bits(angle, m_angle)                         # = a measuring launch on what the run returned
    free = _alone(S, off_pos, turn=False)[3]
    bound = _left_bound(pos.numpy(), S["quads"])
    print("restrain_torsions sampler: largest excess per graph, unrestrained %s, restrained %s (bound %.2e rad)"
          % (free.tolist(), viol.tolist(), bound))
    assert (free > 0.5).all() and (viol < free).all()
    assert (viol <= bound).all()


def test_sampler_weight_reaches_the_launch():
    S = _sampler()
    lo_traj = S["loose_off"][2]
    run, pos, traj = S["run"](torsion_weight=0.5, **S["kw"])
    assert _same_bits(traj[0], _alone(S, lo_traj[0], weight=0.5)[0])
    assert not _same_bits(traj[0], S["restrained"][2][0]) and (run.torsion_viol > 1e-3).any()       # soft: not forced at the end
    # a side table given with the quads is used as it is: the same run as with the sides from the bonds
    oq, tg, tl, _, sides = S["table"]
    run2, pos2, _ = S["run"](torsion_quads=oq, torsion_target=tg, torsion_tol=tl, torsion_sides=sides)
    assert _same_bits(pos2, S["restrained"][1]) and _same_bits(run2.torsion_viol, S["restrained"][0].torsion_viol)


def _core(S):
    """test_hip_core's core of every graph: its first ceil(heavy / 2) heavy atoms, template = a walk per graph; one distance
    restraint per graph between the first core atom and the last atom outside the core; and one torsion restraint per graph on its
    first usable bridge that has a side without a core atom."""
    import core_ref as C
    from agdiff_amd.torsion_restraints import batch_sides
    rng = np.random.default_rng(17)
    select, template = np.zeros(S["N"], dtype=bool), np.zeros((S["N"], 3), dtype=np.float32)
    pairs, quads = [], []
    for g in range(S["G"]):
        idx = np.nonzero(S["batch"] == g)[0]
        heavy = idx[S["at"][idx] != 1]
        select[heavy[:(heavy.size + 1) // 2]] = True
        template[idx] = C.walk(rng, idx.size).astype(np.float32)
        pairs.append((idx[select[idx]][0], idx[~select[idx]][-1]))
    for g in range(S["G"]):
        for q in S["bridges_of"][g]:
            oq, (row, sp, si) = batch_sides(S["N"], S["bi"], S["bt"], S["batch"], q[None, :], frozen=select)
            if row[0] >= 0:
                quads.append(q)
                break
    assert len(quads) == S["G"]
    return select, template, np.asarray(pairs, dtype=np.int32), np.asarray(quads, dtype=np.int32)


def test_sampler_with_distance_restraints_and_a_core_as_well():
    from oracle.covmat_oracle import kabsch_rmsd
    from agdiff_amd.core import hold_core
    from agdiff_amd.restraints import restrain_pairs
    from agdiff_amd.torsion_restraints import batch_sides
    S = _sampler()
    select, template, pairs, quads = _core(S)
    G = S["G"]
    lo, hi = np.full(G, 0.30, dtype=np.float32), np.full(G, 0.35, dtype=np.float32)
    tg, tl = np.full(G, -2.0, dtype=np.float32), np.full(G, 0.1, dtype=np.float32)
    run, pos, traj = S["run"](restraint_pairs=pairs, restraint_lo=lo, restraint_hi=hi, torsion_quads=quads, torsion_target=tg, torsion_tol=tl,
                              core_pos=template, core_select=select)
    assert not S["fused"](run) and torch.isfinite(run.core_dev).all() and torch.isfinite(run.restraint_viol).all()
    assert torch.isfinite(run.torsion_viol).all()
    worst = max(kabsch_rmsd(pos.numpy().astype(np.float64)[(S["batch"] == g) & select], template[(S["batch"] == g) & select]) for g in range(G))
    print("restrain_torsions sampler + pairs + core: largest core RMSD to the template %.2e (bar %.0e); torsion viol %s"
          % (worst, TOL, run.torsion_viol.tolist()))
    assert worst < TOL                                                                     # the core is exact
    # first frame: the update, the distance launch with the core fixed, the torsion launch on sides without a core atom, the hold
    lo_traj = S["loose_off"][2]
    step, _ = restrain_pairs(lo_traj[0].cuda().contiguous(), pairs, lo, hi, S["batch"], fixed=select)
    oq, sides = batch_sides(S["N"], S["bi"], S["bt"], S["batch"], quads, frozen=select)
    assert (sides[0] >= 0).all()
    turned, _, angle, viol = _launch(step.cpu().numpy(), oq, tg, tl, S["batch"], sides)
    assert _same_bits(turned[select], step.cpu()[select]) and not _same_bits(turned, step.cpu()) and (viol > 0).any()
    held, _ = hold_core(turned.cuda().contiguous(), template, select, S["batch"])
    assert _same_bits(traj[0], held.cpu())


def test_sampler_gates_each_constraint_by_its_own_start_sigma():
    """The three constraints of one run, each with a start sigma of its own: pairs from step 2, torsions from step 4, the hold from
    step 6 (A); the same with the hold's start below the whole schedule (B); and with the torsions' there as well (C).  All three
    carry the core keywords, so `fixed` and `frozen` are the same in each; a frame is compared with the public launchers applied by
    hand to the frame of the run that lacks just that constraint at that step."""
    from agdiff_amd.core import hold_core
    from agdiff_amd.restraints import restrain_pairs
    from agdiff_amd.torsion_restraints import batch_sides
    S = _sampler()
    select, template, pairs, quads = _core(S)
    G = S["G"]
    lo, hi = np.full(G, 0.30, dtype=np.float32), np.full(G, 0.35, dtype=np.float32)
    tg, tl = np.full(G, -2.0, dtype=np.float32), np.full(G, 0.1, dtype=np.float32)
    lo_run, _, lo_traj = S["loose_off"]
    sig = [s[0] for s in lo_run._sched]
    assert len(sig) == 10 and all(a > b_ for a, b_ in zip(sig, sig[1:]))
    between = lambda k: 0.5 * (sig[k - 1] + sig[k])        # between two sigmas of the schedule: step k is the first one gated in
    below = 0.5 * sig[-1]                                  # below the whole schedule: only the closing launch runs
    kw = dict(restraint_pairs=pairs, restraint_lo=lo, restraint_hi=hi, torsion_quads=quads, torsion_target=tg, torsion_tol=tl,
              core_pos=template, core_select=select, restraint_start_sigma=between(2))
    runs = {"A": S["run"](torsion_start_sigma=between(4), core_start_sigma=between(6), **kw),
            "B": S["run"](torsion_start_sigma=between(4), core_start_sigma=below, **kw),
            "C": S["run"](torsion_start_sigma=below, core_start_sigma=below, **kw)}
    (_, _, A), (_, _, B), (_, _, C) = runs["A"], runs["B"], runs["C"]
    for k in range(2):
        assert _same_bits(A[k], lo_traj[k]), k
    step, _ = restrain_pairs(lo_traj[2].cuda().contiguous(), pairs, lo, hi, S["batch"], fixed=select)
    assert _same_bits(C[2], step.cpu()) and not _same_bits(C[2], lo_traj[2])
    for k in range(4):
        assert _same_bits(B[k], C[k]), k
    oq, sides = batch_sides(S["N"], S["bi"], S["bt"], S["batch"], quads, frozen=select)
    turned = _launch(C[4].numpy(), oq, tg, tl, S["batch"], sides)[0]
    assert _same_bits(B[4], turned) and not _same_bits(B[4], C[4])
    for k in range(6):
        assert _same_bits(A[k], B[k]), k
    held, _ = hold_core(B[6].cuda().contiguous(), template, select, S["batch"])
    assert _same_bits(A[6], held.cpu()) and not _same_bits(A[6], B[6])
    for name, (run, pos, traj) in runs.items():
        assert len(traj) == 10 and not S["fused"](run) and torch.equal(traj[-1], pos), name
        assert torch.isfinite(run.core_dev).all() and torch.isfinite(run.restraint_viol).all() and torch.isfinite(run.torsion_viol).all(), name


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
    assert torch.isnan(run.torsion_viol[2]) and torch.isnan(run.torsion_angle[2])
    ok = np.nonzero(S["batch"] != 2)[0]
    bound = _left_bound(pos.numpy()[ok], np.searchsorted(ok, S["quads"][[0, 1, 3, 4, 5]]))
    assert (run.torsion_viol[[0, 1, 3, 4, 5]] <= bound).all() and torch.isfinite(run.torsion_angle[[0, 1, 3, 4, 5]]).all()


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
    assert traj == [] and torch.isfinite(pos).all() and (run.torsion_viol <= _left_bound(pos.cpu().numpy(), S["quads"])).all()


# ---------------------------------------------------------------------------------------------------- 5. job function and command line
def test_sample_restrained_and_the_command_line(tmp_path):
    from agdiff_amd import Config, driver, get_model, qm9_model_config, synth
    from agdiff_amd import torsion_restraints as TR
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
    q0, q1 = usable_bridges(mols[0]), usable_bridges(mols[1])
    assert (len(q0), len(q1)) == (5, 4)
    plain, testset = str(tmp_path / "plain.npz"), str(tmp_path / "test.npz")
    driver.save_testset(plain, mols)
    grid = np.array([[-2.0], [-0.5], [1.0]], dtype=np.float32)             # a [3, 1] scan table
    given = {0: ([q0[1]], grid, [0.0]), 1: ([q1[0], q1[2]], [1.0, -1.0], [0.0, 0.1])}
    TR.add_torsion_restraints(plain, testset, given)
    mols = driver.load_testset(testset)
    loaded = TR.load_torsion_restraints(testset)
    for i in range(2):
        mols[i]["tors_quads"], mols[i]["tors_target"], mols[i]["tors_tol"] = loaded[i]
    kw = dict(n_steps=6, step_lr=1e-6, w_global=1.0, global_start_sigma=0.5, clip=1000.0)
    quiet = lambda *_: None
    res = [TR.sample_restrained(m, mol, 4, kw, "cuda:0", counter_seed=2021, log=quiet) for mol in mols]
    pos0, viol0, angle0, ok0 = res[0]
    assert ok0 and res[1][3] and pos0.shape == (4, 12, 3) and pos0.dtype == np.float32 and viol0.dtype == np.float32 and viol0.shape == (4,)
    assert angle0.shape == (4, 1) and angle0.dtype == np.float32 and res[1][2].shape == (4, 2) and res[1][0].shape == (4, 9, 3)
    # conformer c sits on grid row c mod 3 (tol 0, weight 1: the closing launch lands there), within the bound of section 4
    for c in range(4):
        bound = _left_bound(pos0[c], [q0[1]])
        err = abs(float(R.wrap(float(angle0[c, 0]) - float(grid[c % 3, 0]))))
        print("restrain_torsions scan: conformer %d angle %.6f, grid %.1f, |error| %.2e (bound %.2e)" % (c, angle0[c, 0], grid[c % 3, 0], err, bound))
        assert err <= bound and viol0[c] <= bound
        assert res[1][1][c] <= _left_bound(res[1][0][c], given[1][0])
    # the same draws through begin_sampling
    packed = driver.pack_batch([mols[0]], lambda _: 4)
    q, tg, tl, sides = TR.pack_torsion_restraints(packed, [loaded[0]])
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p0 = m.counter_normals(packed["batch"], packed["stream_ids"], 2021, [-1])[0]
    run = m.begin_sampling(T(packed["atom_type"]), p0, T(packed["bond_index"]), T(packed["bond_type"]), T(packed["batch"]), 4, False,
                           raise_on_nan=False, save_traj=False, noise_mode="counter", noise_seed=2021, stream_ids=packed["stream_ids"],
                           torsion_quads=q, torsion_target=tg, torsion_tol=tl, torsion_sides=sides, **kw)
    run.advance(run.remaining())
    direct = run.finish()[0].cpu().numpy().reshape(4, 12, 3)
    assert np.array_equal(direct, pos0) and np.array_equal(run.torsion_viol.numpy(), viol0)
    assert np.array_equal(run.torsion_angle.numpy().reshape(4, 1), angle0)
    # unrestrained, the same molecule comes out elsewhere, and off its grid
    free, _, none, _ = TR.sample_restrained(m, {k: v for k, v in mols[0].items() if not k.startswith("tors_")}, 4, kw, "cuda:0",
                                            counter_seed=2021, log=quiet)
    assert none.shape == (4, 0) and not np.array_equal(free, pos0) and (TR.measure(mols[0], free, loaded[0])[0] > 1e-3).all()
    # the command line, in a child process: the same job bit for bit
    out = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "agdiff_amd.torsion_restraints", "--ckpt", ckpt, "--testset", testset, "--out", out,
                        "--num-confs", "4", "--n-steps", "6", "--noise", "counter", "--seed", "2021"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    samples = os.path.join(out, "samples_all.npz")
    z = np.load(samples)
    assert set(z.files) == {"%s_%d" % (k, i) for k in ("pos_gen", "name", "tors_viol", "tors_angle") for i in range(2)}
    for i in range(2):
        assert np.array_equal(z["pos_gen_%d" % i], res[i][0]) and np.array_equal(z["tors_viol_%d" % i], res[i][1]), i
        assert np.array_equal(z["tors_angle_%d" % i], res[i][2]) and z["tors_angle_%d" % i].dtype == np.float32, i
    # report mode measures the finished job (in this process), and the validity module accepts the file
    rep = TR.main(["--report", "--samples", samples, "--testset", testset, "--out", str(tmp_path / "viol.npz")])
    for i in range(2):
        assert np.array_equal(rep["tors_viol_%d" % i], res[i][1]) and np.array_equal(rep["tors_angle_%d" % i], res[i][2]), i
    assert set(np.load(str(tmp_path / "viol.npz")).files) == {"tors_viol_0", "tors_viol_1", "tors_angle_0", "tors_angle_1"}
    from agdiff_amd import validity                      # (python -m agdiff_amd.validity's main, without another process)
    verdicts = validity.main(["--samples", samples, "--testset", testset, "--out", str(tmp_path / "valid.npz")])
    assert verdicts["valid_0"].shape == (4,) and verdicts["valid_1"].shape == (4,)
