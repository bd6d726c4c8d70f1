#!/usr/bin/env python3
"""What sampling around a fixed core costs (agdiff_amd/core.py), on the first packed batch of the default job
(bench.drugs200_job, 196,608 atoms at most -- the bench's batch shape), all in this one process:

  * the time per step of a `--n-steps`-step run (save_traj=False, nan_check_every=64), `--repeats` runs of each kind, interleaved:
    with the fused front (today's default), launch by launch (model.fused_front = False) without a core, and launch by launch
    holding a core of about 40 % of every molecule's heavy atoms (a constrained run cannot take the fused front): wall clock
    around advance() + finish() with a device synchronisation on either side;
  * the agdiff_hold_core launch alone on that batch, and -- as the floor a launch of this grid has -- the same launch with every
    graph skipped (each wave reads its skip flag and returns): device events around `--reps` launches after a warm-up of a fifth
    as many, medians of `--rounds` rounds, by tools/planarity_time.py's method.

A record, not a gate: nothing here was fixed in advance.    python tools/core_time.py [--out profiles/core_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
from agdiff_amd import _lib, driver, get_model, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=2000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--n-steps", type=int, default=256)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--fraction", type=float, default=0.4, help="of every molecule's heavy atoms that form its core")
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
rng = np.random.default_rng(7)
for m in bmols:            # a template per molecule: a random walk of 1.5 A steps; its core: the first 40 % of the heavy atoms
    n = m["atom_type"].shape[0]
    d = rng.normal(size=(n, 3))
    m["core_pos"] = np.cumsum(1.5 * d / np.linalg.norm(d, axis=1, keepdims=True), axis=0).astype(np.float32)
    heavy = np.nonzero(np.asarray(m["atom_type"]) != 1)[0]
    m["core_mask"] = np.zeros(n, dtype=np.uint8)
    m["core_mask"][heavy[:max(1, int(round(args.fraction * heavy.size)))]] = 1
packed = driver.pack_batch(bmols, confs_of)
N, G = packed["atom_type"].shape[0], packed["num_graphs"]
heavy, held = int((packed["atom_type"] != 1).sum()), int(packed["core_select"].sum())
say("core hold on %s; torch %s, HIP %s, ABI %d" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip,
                                                   _lib.DEFINES["AGDIFF_ABI_VERSION"]))
say("batch: %d molecules, %d conformers, %d atoms (%d heavy); core: %d atoms = %.1f %% of the heavy atoms, %.1f per conformer"
    % (len(bmols), G, N, heavy, held, 100.0 * held / heavy, held / G))

# ---- the runs
cfg = bench.make_cfg("drugs", "saturated")
model = get_model(cfg)
model.load_state_dict(synth.synth_state_dict(model.state_dict()))
model = model.to(dev).eval()
T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
at, bi, bt, ba = T(packed["atom_type"]), T(packed["bond_index"]), T(packed["bond_type"]), T(packed["batch"])
kw = dict(n_steps=args.n_steps, step_lr=1e-6, w_global=1.0, global_start_sigma=0.5, clip=1000.0, save_traj=False, nan_check_every=64,
          raise_on_nan=False)          # (as the driver samples: a diverging conformer is quarantined, the run goes on)
quarantined = {}
KINDS = ("fused front, no core        ", "launch by launch, no core   ", "launch by launch, core held ")


def one_run(kind):
    torch.manual_seed(5)
    p0 = torch.randn(N, 3, device=dev)
    extra = dict(core_pos=packed["core_pos"], core_select=packed["core_select"]) if kind == 2 else {}
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
        assert torch.isfinite(run.core_dev[~run.nan_graphs()]).all()
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
say("leaving the fused front costs %+.4f ms per step (%+.2f %%); the hold itself %+.4f ms per step (%+.2f %% of the launch-by-launch step); "
    "a constrained run pays %+.4f ms per step (%+.2f %%) over today's default, by the medians"
    % (med[1] - med[0], 100.0 * (med[1] / med[0] - 1.0), med[2] - med[1], 100.0 * (med[2] / med[1] - 1.0), med[2] - med[0],
       100.0 * (med[2] / med[0] - 1.0)))

# ---- the launch alone
pos0 = torch.randn(N, 3, device=dev) * 3.0
pos = pos0.clone()
tpl, sel = T(packed["core_pos"]), T(packed["core_select"])
gp = T(np.searchsorted(packed["batch"], np.arange(G + 1)).astype(np.int32))
out = torch.empty(G, dtype=torch.float32, device=dev)
skip_all = torch.ones(G, dtype=torch.int32, device=dev)
st = _lib.stream_ptr()


def launch(skip, weight):
    return lambda: _lib.check(lib.agdiff_hold_core(_lib.ptr(pos), _lib.ptr(tpl), _lib.ptr(sel), _lib.ptr(gp), _lib.ptr(skip), G, N, weight,
                                                   None, _lib.ptr(out), st), "agdiff_hold_core")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for name, fn in (("agdiff_hold_core, weight 1            ", launch(None, 1.0)), ("agdiff_hold_core, weight 0.5          ", launch(None, 0.5)),
                 ("the same grid, every graph skipped    ", launch(skip_all, 1.0))):
    pos.copy_(pos0)
    timed(fn, max(1, args.reps // 5))
    us = 1e3 * np.array([timed(fn, args.reps) for _ in range(args.rounds)])
    say("%s %d waves: median %8.2f us  min %8.2f  max %8.2f   (%d launches per figure, %d rounds)"
        % (name, G, np.median(us), us.min(), us.max(), args.reps, args.rounds))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
