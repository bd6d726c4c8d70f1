#!/usr/bin/env python3
"""Times of agdiff_kmedoids on random metric matrices (the pairwise distances of random points) at G = 1000 and G = 4096 with
K = 1, 10 and 100 from the first K conformers as seeds.  Per (G, K): the call with max_iter set to the number of updates the walk
needs (so that every enqueued launch works: the time per iteration), then with max_iter = 32 and 128 (the same walk followed by
launches that read the done flag and return: what those cost per call).  Set against: the agdiff_rmsd_self launch that makes the
float matrix of a molecule of 25 heavy atoms with P = 1, agdiff_butina_cluster on the same matrix thresholded at its 2 % quantile,
agdiff_maxmin_pick with the same K on the same matrix, and the numpy restatement of the rule on the CPU (tests/kmedoids_ref.py).
Every timed launch is also compared with the restatement, and the restatement's final cost from the first K, the last K and the
MaxMin picks as seeds is recorded: the local optimum depends on them.  Device events around a window of launches after a warm-up -- as many
launches as fill `--window-ms` -- medians over `--rounds` rounds.  Not a test, and no figure is a gate.

    python tools/medoid_timing.py [--out profiles/medoid_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import butina_ref as BR
import kmedoids_ref as KR
from agdiff_amd import _lib

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


say("agdiff_kmedoids on random metric matrices, the first K conformers as seeds; windows of >= %.0f ms of calls per figure, median of %d rounds"
    % (args.window_ms, args.rounds))
call_ms = {}
for G in (1000, 4096):
    d = KR.random_metric(G, seed=G)
    q = KR.Q(d)
    dd = torch.from_numpy(d).to(dev)
    labels, near = torch.empty(G, dtype=torch.int32, device=dev), torch.empty(G, dtype=torch.float32, device=dev)
    cost = torch.empty(1, dtype=torch.float64, device=dev)
    n_iter, status = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    work = torch.empty(_lib.DEFINES["AGDIFF_KMEDOIDS_WORK_BYTES"] // 8, dtype=torch.int64, device=dev)
    for K in (1, 10, 100):
        init = torch.arange(K, dtype=torch.int32, device=dev)
        medoids, size = torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.int32, device=dev)
        within = torch.empty(K, dtype=torch.float64, device=dev)
        t0 = time.perf_counter()
        want = KR.kmedoids(d, list(range(K)), max_iter=32, q=q)
        cpu = (time.perf_counter() - t0) * 1e3
        updates = want[6]
        assert want[7] == 0
        ms = {}
        for max_iter in (updates, 32, 128):
            fn = lambda: _lib.check(lib.agdiff_kmedoids(_lib.ptr(dd), G, K, _lib.ptr(init), max_iter, _lib.ptr(medoids), _lib.ptr(labels),
                                                        _lib.ptr(near), _lib.ptr(size), _lib.ptr(within), _lib.ptr(cost), _lib.ptr(n_iter),
                                                        _lib.ptr(status), _lib.ptr(work), st), "agdiff_kmedoids")
            med, lo, hi, reps = median_ms(fn)
            got = (medoids.cpu().numpy(), labels.cpu().numpy(), near.cpu().numpy(), size.cpu().numpy(), within.cpu().numpy(),
                   cost.cpu().numpy()[0], int(n_iter.item()), int(status.item()))
            ms[max_iter] = med
            say("G = %4d, K = %3d, max_iter = %3d: agdiff_kmedoids (%2d updates, %3d launches enqueued) median %8.4f ms  min %8.4f  max %8.4f  "
                "(%5d calls a window; equal to the restatement: %s)"
                % (G, K, max_iter, got[6], 3 * max_iter + 3, med, lo, hi, reps, KR.same(got, want)))
        idle32, idle128 = 3 * (32 - updates), 3 * (128 - updates)
        say("    %.4f ms an iteration (assign + member costs + choose); the launches that return at once: max_iter = 32, %3d of them, "
            "+%.4f ms a call (%.2f us each); max_iter = 128, %3d of them, +%.4f ms a call (%.2f us each); numpy on the CPU %.1f ms"
            % (ms[updates] / updates, idle32, ms[32] - ms[updates], 1e3 * (ms[32] - ms[updates]) / max(idle32, 1), idle128,
               ms[128] - ms[updates], 1e3 * (ms[128] - ms[updates]) / max(idle128, 1), cpu))
        call_ms[(G, K)] = ms[32]
        last, far = KR.kmedoids(d, list(range(G - K, G)), q=q), KR.kmedoids(d, KR.maxmin(d, K)[0].tolist(), q=q)
        say("    the local optimum depends on the seeds (the restatement on the CPU): final cost %.1f from the first K (%d updates), %.1f "
            "from the last K (%d), %.1f from the MaxMin picks (%d)" % (want[5], want[6], last[5], last[6], far[5], far[6]))
    # the two one-workgroup walks on the same matrix: Butina under a threshold that gives every conformer 2 % of the others as
    # neighbours, MaxMin with the same K
    n = torch.empty(1, dtype=torch.int32, device=dev)
    thr = float(np.quantile(d[np.triu_indices(G, 1)], 0.02))
    adj = d <= thr
    b = torch.from_numpy(BR.pack(adj)).to(dev)
    leader, count, rank = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(3))
    fn = lambda: _lib.check(lib.agdiff_butina_cluster(_lib.ptr(b), G, 1, _lib.ptr(leader), _lib.ptr(count), _lib.ptr(rank), _lib.ptr(n), st),
                            "agdiff_butina_cluster")
    med, lo, hi, reps = median_ms(fn)
    say("G = %4d: agdiff_butina_cluster reorder = 1 on the same matrix <= %.3f (density %.3f, %4d clusters) median %8.4f ms  min %8.4f  "
        "max %8.4f  (%d launches a window); agdiff_kmedoids (max_iter = 32) K = 1 / 10 / 100: %.2f x / %.2f x / %.2f x that"
        % (G, thr, float(adj.mean()), int(n.item()), med, lo, hi, reps, call_ms[(G, 1)] / med, call_ms[(G, 10)] / med, call_ms[(G, 100)] / med))
    cover = torch.empty(1, dtype=torch.float32, device=dev)
    for K in (1, 10, 100):
        picks, radius = torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.float32, device=dev)
        fn = lambda: _lib.check(lib.agdiff_maxmin_pick(_lib.ptr(dd), G, K, 0, -1.0, _lib.ptr(picks), _lib.ptr(radius), _lib.ptr(labels),
                                                       _lib.ptr(near), _lib.ptr(n), _lib.ptr(cover), st), "agdiff_maxmin_pick")
        med, lo, hi, reps = median_ms(fn)
        say("G = %4d, K = %3d: agdiff_maxmin_pick on the same matrix median %8.4f ms  min %8.4f  max %8.4f  (%d launches a window); "
            "agdiff_kmedoids (max_iter = 32): %.2f x that" % (G, K, med, lo, hi, reps, call_ms[(G, K)] / med))

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
    for K in (1, 10, 100):
        ms = call_ms[(G, K)]
        say("    agdiff_kmedoids K = %3d, max_iter = 32: %.3f x that launch%s" % (K, ms / med, " -- the clustering is the slow step" if ms > med else ""))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
