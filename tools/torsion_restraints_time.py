#!/usr/bin/env python3
"""What sampling under torsion restraints costs (agdiff_amd/torsion_restraints.py), on the first packed batch of the
default job (bench.drugs200_job, 196,608 atoms at most -- the bench's batch shape, tools/restraints_time.py's), all in this one
process:

  * the time per step of a `--n-steps`-step run (save_traj=False, nan_check_every=64), `--repeats` runs of each kind, interleaved:
    with the fused front (today's default), launch by launch (model.fused_front = False) without restraints, and launch by launch
    under `--per-graph` torsion restraints per conformer (such a run cannot take the fused front): wall clock around advance() +
    finish() with a device synchronisation on either side;
  * the agdiff_restrain_torsions launch alone on that batch at 1 and at `--per-graph` restraints per conformer, turning and only
    measuring, and -- as the floor a launch of this grid has -- the same grid with every graph skipped (each wave reads its skip flag
    and returns): device events around `--reps` launches after a warm-up of a fifth as many, medians of `--rounds` rounds, by
    tools/core_time.py's method.  The positions are restored before every figure; after the first launch of a figure every angle
    sits on the edge of its window, so the figure is that of a run's steady state (every quad measured, little turned).

A record, not a gate: nothing here was fixed in advance.    python tools/torsion_restraints_time.py [--out profiles/torsion_restraints_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
from agdiff_amd import _lib, driver, get_model, synth
from agdiff_amd import torsion_restraints as TR

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=2000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--n-steps", type=int, default=256)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--per-graph", type=int, default=4, help="torsion restraints per conformer")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
lib = _lib.load()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


mols, confs_of = bench.drugs200_job(2021)
bmols = driver.plan_batches(mols, confs_of, 196608)[0]
packed = driver.pack_batch(bmols, confs_of)
N, G = packed["atom_type"].shape[0], packed["num_graphs"]
rng = np.random.default_rng(7)


def tables(per_graph):
    """`per_graph` restraints per molecule on bridges drawn at random, windows target +- 0.3 rad with targets uniform on the circle."""
    per = []
    for m in bmols:
        q = TR.bridge_quads(m["atom_type"].shape[0], m["edge_index"], m["edge_type"])
        q = q[np.sort(np.random.default_rng(11).permutation(q.shape[0])[:per_graph])]
        per.append((q, rng.uniform(-3.0, 3.0, size=q.shape[0]).astype(np.float32), np.full(q.shape[0], 0.3, dtype=np.float32)))
    q, tg, tl, sides = TR.pack_torsion_restraints(packed, per)
    return q, tg, tl, sides, TR.restraint_arguments(N, q, tg, tl, packed["batch"], sides, num_graphs=G)


q, tg, tl, sides, full = tables(args.per_graph)
say("torsion restraints on %s; torch %s, HIP %s, ABI %d" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip,
                                                            _lib.DEFINES["AGDIFF_ABI_VERSION"]))
say("batch: %d molecules, %d conformers, %d atoms; %d restraints = %.2f per conformer; side table: %d rows, %d entries (each molecule's "
    "rows once), the largest row %d atoms" % (len(bmols), G, N, q.shape[0], q.shape[0] / G, sides[1].shape[0] - 1, sides[2].shape[0],
                                              int(np.diff(sides[1]).max())))

# ---- the runs
cfg = bench.make_cfg("drugs", "saturated")
model = get_model(cfg)
model.load_state_dict(synth.synth_state_dict(model.state_dict()))
model = model.to(dev).eval()
T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
at, bi, bt, ba = T(packed["atom_type"]), T(packed["bond_index"]), T(packed["bond_type"]), T(packed["batch"])
kw = dict(n_steps=args.n_steps, step_lr=1e-6, w_global=1.0, global_start_sigma=0.5, clip=1000.0, save_traj=False, nan_check_every=64,
          raise_on_nan=False)          # (as the driver samples: a diverging conformer is quarantined, the run goes on)
quarantined, left = {}, {}
KINDS = ("fused front, no restraints      ", "launch by launch, no restraints ", "launch by launch, restrained    ")


def one_run(kind):
    torch.manual_seed(5)
    p0 = torch.randn(N, 3, device=dev)
    extra = dict(torsion_quads=q, torsion_target=tg, torsion_tol=tl, torsion_sides=sides) if kind == 2 else {}
    model.fused_front = kind == 0
    try:
        run = model.begin_sampling(at, p0, bi, bt, ba, G, False, **kw, **extra)
        assert bool(run._fused_front()) == (kind == 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run.advance(run.remaining())
        run.finish()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.n_steps
    finally:
        model.fused_front = True
    quarantined[kind] = int(run.nan_graphs().sum())
    if kind == 2:
        v = run.torsion_viol[~run.nan_graphs()]
        assert torch.isfinite(v).all()
        left[kind] = float(v.max()) if v.numel() else float("nan")
    return ms


for kind in range(3):                  # warm-up: code objects, the topology cache
    one_run(kind)
res = {kind: [] for kind in range(3)}
for _ in range(args.repeats):
    for kind in range(3):
        res[kind].append(one_run(kind))
med = {kind: float(np.median(res[kind])) for kind in range(3)}
for kind in range(3):
    say("%d-step run, save_traj=False, %s: ms per step %s  (median %.4f; %d of %d conformers quarantined)"
        % (args.n_steps, KINDS[kind], " ".join("%.4f" % x for x in res[kind]), med[kind], quarantined[kind], G))
say("largest excess left in the restrained run's conformers: %.2e rad (synthetic weights: this says the launches ran, nothing about "
    "chemistry)" % left[2])
say("leaving the fused front costs %+.4f ms per step (%+.2f %%); the torsion launch itself %+.4f ms per step (%+.2f %% of the "
    "launch-by-launch step); a restrained run pays %+.4f ms per step (%+.2f %%) over today's default, by the medians"
    % (med[1] - med[0], 100.0 * (med[1] / med[0] - 1.0), med[2] - med[1], 100.0 * (med[2] / med[1] - 1.0), med[2] - med[0],
       100.0 * (med[2] / med[0] - 1.0)))

# ---- the launch alone
pos0 = torch.randn(N, 3, device=dev) * 3.0
pos = pos0.clone()
gp = T(np.searchsorted(packed["batch"], np.arange(G + 1)).astype(np.int32))
out = torch.empty(G, dtype=torch.float32, device=dev)
skip_all = torch.ones(G, dtype=torch.int32, device=dev)
st = _lib.stream_ptr()


def launch(table, skip, turn):
    tr_ptr, oq, centre, half, (row, sp, si), _, _ = table
    d = [T(x) for x in (tr_ptr, oq, centre, half, row, sp, si)]
    angle = torch.empty(oq.shape[0], dtype=torch.float32, device=dev)
    return lambda: _lib.check(lib.agdiff_restrain_torsions(_lib.ptr(pos), _lib.ptr(gp), *(_lib.ptr(x) for x in d), _lib.ptr(skip), G, N,
                                                           int(oq.shape[0]), int(sp.shape[0]) - 1, 1.0, turn, None, _lib.ptr(angle),
                                                           _lib.ptr(out), st), "agdiff_restrain_torsions")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


one = tables(1)[4]
for name, fn in (("agdiff_restrain_torsions, 1 per conformer         ", launch(one, None, 1)),
                 ("agdiff_restrain_torsions, %d per conformer         " % args.per_graph, launch(full, None, 1)),
                 ("%d per conformer, only measuring (turn = 0)        " % args.per_graph, launch(full, None, 0)),
                 ("1 per conformer, every graph skipped              ", launch(one, skip_all, 1)),
                 ("%d per conformer, every graph skipped              " % args.per_graph, launch(full, skip_all, 1))):
    pos.copy_(pos0)
    timed(fn, max(1, args.reps // 5))
    us = 1e3 * np.array([timed(fn, args.reps) for _ in range(args.rounds)])
    say("%s %d waves: median %8.2f us  min %8.2f  max %8.2f   (%d launches per figure, %d rounds)"
        % (name, G, np.median(us), us.min(), us.max(), args.reps, args.rounds))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
