#!/usr/bin/env python3
"""Times of agdiff_maxmin_pick on random metric matrices (the pairwise distances of random points) at G = 1000 and G = 4096 with
K = 10, 100 and G, against three things: agdiff_butina_cluster ON THE SAME MATRIX thresholded at its 2 % quantile (the other walk
over a conformer matrix, one workgroup too), the agdiff_rmsd_self launch that makes the float matrix of a molecule of 25 heavy
atoms with P = 1, and the numpy restatement of the rule on the CPU (tests/maxmin_ref.py).  Every launch is also compared with the
restatement.  Device events around a window of launches after a warm-up -- as many launches as fill `--window-ms` -- medians over
`--rounds` rounds.  Not a test, and no figure is a gate.

    python tools/pick_timing.py [--out profiles/pick_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import butina_ref as BR
import maxmin_ref as MR
from agdiff_amd import _lib, ensemble

ap = argparse.ArgumentParser()
ap.add_argument("--window-ms", type=float, default=100.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lib = _lib.load()
dev = torch.device("cuda", 0)
st = _lib.stream_ptr()
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


def median_ms(fn):
    """(median, min, max, launches per window): warm-up, then windows of at least --window-ms of device time"""
    fn(); fn()
    torch.cuda.synchronize()
    once = max(timed(fn, 3), 1e-3)
    reps = int(min(max(args.window_ms / once, 5), 20000))
    v = np.array([timed(fn, reps) for _ in range(args.rounds)])
    return float(np.median(v)), float(v.min()), float(v.max()), reps


say("agdiff_maxmin_pick on random metric matrices; windows of >= %.0f ms of launches per figure, median of %d rounds" % (args.window_ms, args.rounds))
pick_ms = {}
for G in (1000, 4096):
    d = MR.random_metric(G, seed=G)
    dd = torch.from_numpy(d).to(dev)
    owner = torch.empty(G, dtype=torch.int32, device=dev)
    near = torch.empty(G, dtype=torch.float32, device=dev)
    n, cover = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
    for K in (10, 100, G):
        picks, radius = torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.float32, device=dev)
        fn = lambda: _lib.check(lib.agdiff_maxmin_pick(_lib.ptr(dd), G, K, 0, -1.0, _lib.ptr(picks), _lib.ptr(radius), _lib.ptr(owner),
                                                       _lib.ptr(near), _lib.ptr(n), _lib.ptr(cover), st), "agdiff_maxmin_pick")
        med, lo, hi, reps = median_ms(fn)
        got = (picks.cpu().numpy(), radius.cpu().numpy(), owner.cpu().numpy(), near.cpu().numpy(), int(n.item()), cover.cpu().numpy()[0])
        t0 = time.perf_counter()
        want = MR.maxmin(d, K)
        cpu = (time.perf_counter() - t0) * 1e3
        say("G = %4d, K = %4d: agdiff_maxmin_pick (%4d picks, %4d row reads) median %8.4f ms  min %8.4f  max %8.4f  (%5d launches a window; "
            "%.2f us a step; numpy on the CPU %.1f ms; equal to it: %s)"
            % (G, K, got[4], K, med, lo, hi, reps, 1e3 * med / K, cpu, MR.same(got, want)))
        pick_ms[(G, K)] = med
    # the other one-workgroup walk, on the same matrix under a threshold that gives every conformer 2 % of the others as neighbours
    thr = float(np.quantile(d[np.triu_indices(G, 1)], 0.02))
    adj = d <= thr
    b = torch.from_numpy(BR.pack(adj)).to(dev)
    leader, count, rank = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(3))
    fn = lambda: _lib.check(lib.agdiff_butina_cluster(_lib.ptr(b), G, 1, _lib.ptr(leader), _lib.ptr(count), _lib.ptr(rank), _lib.ptr(n), st),
                            "agdiff_butina_cluster")
    med, lo, hi, reps = median_ms(fn)
    say("G = %4d: agdiff_butina_cluster reorder = 1 on the same matrix <= %.3f (density %.3f, %4d clusters) median %8.4f ms  min %8.4f  "
        "max %8.4f  (%d launches a window); agdiff_maxmin_pick K = 10 / 100 / G: %.2f x / %.2f x / %.2f x that"
        % (G, thr, float(adj.mean()), int(n.item()), med, lo, hi, reps, pick_ms[(G, 10)] / med, pick_ms[(G, 100)] / med, pick_ms[(G, G)] / med))

# the launch that produces the float matrix: one molecule, 25 heavy atoms of 44, identity mapping only (P = 1)
natoms, m = 44, 25
rng = np.random.default_rng(2021)
for G in (1000, 4096):
    pos = torch.from_numpy((rng.normal(size=(natoms, 3))[None] * 1.5 + 0.25 * rng.normal(size=(G, natoms, 3))).astype(np.float32)).to(dev)
    idx = torch.arange(m, dtype=torch.int32, device=dev)
    scratch = torch.empty(G * (3 * m + 1), dtype=torch.float32, device=dev)
    out = torch.empty((G, G), dtype=torch.float32, device=dev)
    fn = lambda: _lib.check(lib.agdiff_rmsd_self(_lib.ptr(pos), _lib.ptr(idx), _lib.ptr(None), G, natoms, m, 0, 0.0, _lib.ptr(scratch),
                                                 _lib.ptr(out), _lib.ptr(None), st), "agdiff_rmsd_self")
    med, lo, hi, reps = median_ms(fn)
    say("G = %4d: agdiff_rmsd_self (out only; n = %d, m = %d, P = 1) median %8.4f ms  min %8.4f  max %8.4f  (%d launches a window)"
        % (G, natoms, m, med, lo, hi, reps))
    for K in (10, 100, G):
        ms = pick_ms[(G, K)]
        say("    agdiff_maxmin_pick K = %4d: %.3f x that launch%s" % (K, ms / med, " -- the picking is the slow step" if ms > med else ""))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
