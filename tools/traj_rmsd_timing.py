#!/usr/bin/env python3
"""What tracking every conformer's RMSD to a target costs (agdiff_amd/trajectory.py), on the first packed batch of
the default job (bench.drugs200_job, 196,608 atoms at most -- the bench's batch shape):

  * one agdiff_traj_rmsd launch over 64 frames of that batch (a NaN poll's worth), heavy atoms, with and without the mirror
    output: device events around `--reps` launches after a warm-up, medians of `--rounds` rounds;
  * the time per step of a `--n-steps`-step run (save_traj=False, nan_check_every=64) without and with tracking, interleaved,
    `--repeats` runs each: wall clock around advance() + finish() with a device synchronisation on either side.

A record, not a gate.    python tools/traj_rmsd_timing.py [--out profiles/traj_rmsd_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
from agdiff_amd import driver, get_model, synth
from agdiff_amd.trajectory import RmsdTracker

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--n-steps", type=int, default=256)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


mols, confs_of = bench.drugs200_job(2021)
bmols = driver.plan_batches(mols, confs_of, 196608)[0]
rng = np.random.default_rng(7)
for m in bmols:            # a target per molecule: a random walk of 1.5 A steps (the arithmetic does not depend on what it is)
    d = rng.normal(size=(m["atom_type"].shape[0], 3))
    m["pos_target"] = np.cumsum(1.5 * d / np.linalg.norm(d, axis=1, keepdims=True), axis=0).astype(np.float32)
packed = driver.pack_batch(bmols, confs_of)
N, G = packed["atom_type"].shape[0], packed["num_graphs"]
heavy = int((packed["atom_type"] != 1).sum())
say("batch: %d molecules, %d conformers, %d atoms (%d heavy)" % (len(bmols), G, N, heavy))

# ---- the launch alone
S = args.frames
gp = np.searchsorted(packed["batch"], np.arange(G + 1)).astype(np.int32)
frames = torch.randn((S, N, 3), device=dev) * 3.0
for mirror in (False, True):
    tr = RmsdTracker(packed["pos_target"], None, gp, S, dev, mirror=mirror, atom_type=packed["atom_type"])
    tr.evaluate(frames, 3 * N, S, 0)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            tr.evaluate(frames, 3 * N, S, 0)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / args.reps)
    v = np.array(ms)
    say("agdiff_traj_rmsd, %d frames x %d graphs%s: median %.4f ms  min %.4f  max %.4f  (%.1f MB of frames read per launch: %.0f GB/s)"
        % (S, G, ", with the mirror output" if mirror else "", np.median(v), v.min(), v.max(), S * N * 12 / 1e6,
           S * N * 12 / np.median(v) / 1e6))
    assert torch.isfinite(tr.rows).all()
del frames, tr

# ---- the run with and without
cfg = bench.make_cfg("drugs", "saturated")
model = get_model(cfg)
model.load_state_dict(synth.synth_state_dict(model.state_dict()))
model = model.to(dev).eval()
T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
at, bi, bt, ba = T(packed["atom_type"]), T(packed["bond_index"]), T(packed["bond_type"]), T(packed["batch"])
kw = dict(n_steps=args.n_steps, step_lr=1e-6, w_global=1.0, global_start_sigma=0.5, clip=1000.0, save_traj=False, nan_check_every=64)


def one_run(track):
    torch.manual_seed(5)
    p0 = torch.randn(N, 3, device=dev)
    extra = dict(rmsd_target=packed["pos_target"]) if track else {}
    run = model.begin_sampling(at, p0, bi, bt, ba, G, False, **kw, **extra)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run.advance(run.remaining())
    run.finish()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.n_steps
    if track:
        assert tuple(run.rmsd_curve.shape) == (args.n_steps, G) and torch.isfinite(run.rmsd_curve).all()
    return ms


one_run(False), one_run(True)            # warm-up: code objects, the topology cache
res = {False: [], True: []}
for _ in range(args.repeats):
    for track in (False, True):
        res[track].append(one_run(track))
for track in (False, True):
    say("%d-step run, save_traj=False, %s: ms per step %s  (median %.4f)"
        % (args.n_steps, "tracking   " if track else "no tracking", " ".join("%.4f" % x for x in res[track]), np.median(res[track])))
say("tracking costs %+.4f ms per step (%+.2f %%) by the medians; the ring holds %d frames = %.0f MB"
    % (np.median(res[True]) - np.median(res[False]), 100.0 * (np.median(res[True]) / np.median(res[False]) - 1.0), 2 * 64, 2 * 64 * N * 12 / 1e6))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
