#!/usr/bin/env python3
"""Times of the distance-distribution MMD kernels, by tools/validity_timing.py's method: device events around `--reps` launches after
a warm-up, `--rounds` rounds, the two calls alternating round by round in this one process, medians.

agdiff_mmd_single and agdiff_mmd_all at R = 500 references, G = 1000 generated conformers and K = 300 atom pairs (a Drugs molecule of
25 heavy atoms), on random tables of two visibly different distributions; and, for scale, the wall time on the CPU of the float64
numpy restatement (tests/mmd_ref.py) at R = 50, G = 100, K = 300 -- a tenth of the conformers, a hundredth of the pairs.  A record,
not a gate.

    python tools/mmd_timing.py [--out profiles/mmd_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import mmd_ref as MR
from agdiff_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lib = _lib.load()
dev = torch.device("cuda", 0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(R, G, K):
    x_np, y_np = MR.tables(R, G, K, seed=2021)
    x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    M, T = R + G, (R + G + 15) // 16
    tiles = T * (T + 1) // 2
    scratch_all = torch.empty(K + 1 + 3 * tiles, dtype=torch.float64, device=dev)
    scratch_single = torch.empty(2 * K + (K * M + 1) // 2, dtype=torch.float64, device=dev)
    m_all, b_all = (torch.empty(1, dtype=torch.float32, device=dev) for _ in range(2))
    m_single, b_single = (torch.empty(K, dtype=torch.float32, device=dev) for _ in range(2))
    st = _lib.stream_ptr()

    def run_single():
        _lib.check(lib.agdiff_mmd_single(_lib.ptr(x), _lib.ptr(y), R, G, K, _lib.ptr(scratch_single), _lib.ptr(m_single), _lib.ptr(b_single),
                                         st), "agdiff_mmd_single")

    def run_all():
        _lib.check(lib.agdiff_mmd_all(_lib.ptr(x), _lib.ptr(y), R, G, K, _lib.ptr(scratch_all), _lib.ptr(m_all), _lib.ptr(b_all), st),
                   "agdiff_mmd_all")

    calls = [("agdiff_mmd_single", run_single), ("agdiff_mmd_all", run_all)]
    for _, fn in calls:                         # warm-up: code objects
        fn(); fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in calls}
    for _ in range(args.rounds):
        for name, fn in calls:
            ms[name].append(timed(fn, args.reps))
    pairs = M * (M + 1) // 2
    say("R = %d, G = %d, K = %d: M = %d rows, %d row pairs a <= b, %d tiles" % (R, G, K, M, pairs, tiles))
    evals = {"agdiff_mmd_single": K * pairs, "agdiff_mmd_all": pairs}
    for name, _ in calls:
        v = np.array(ms[name])
        say("  %-20s median %9.4f ms  min %9.4f  max %9.4f   (%.3g kernel-matrix entries, %.1f G / s)"
            % (name, np.median(v), v.min(), v.max(), evals[name], evals[name] / np.median(v) * 1e-6))
    say("  all = %.6f (bandwidth %.4f), single mean = %.6f, median = %.6f"
        % (float(m_all.item()), float(b_all.item()), float(m_single.double().mean()), float(m_single.double().median())))


def measure_cpu(R, G, K):
    x, y = MR.tables(R, G, K, seed=2021)
    t0 = time.perf_counter()
    MR.mmd_single(x, y)
    t1 = time.perf_counter()
    MR.mmd_all(x, y)
    t2 = time.perf_counter()
    say("numpy float64 reference on the CPU, R = %d, G = %d, K = %d (one run each): single %.1f ms, all %.1f ms"
        % (R, G, K, 1e3 * (t1 - t0), 1e3 * (t2 - t1)))


say("distance-distribution MMD kernels; %d launches per figure, medians of %d alternating rounds" % (args.reps, args.rounds))
measure(500, 1000, 300)
measure_cpu(50, 100, 300)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
