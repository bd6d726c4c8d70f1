#!/usr/bin/env python3
"""Times of agdiff_pam_build and agdiff_pam_swap on random metric matrices (the pairwise distances of random points, the
matrices of tools/medoid_timing.py) at G = 1000 and G = 4096 with K = 1, 10 and 100.  Per (G, K): agdiff_pam_build (the time per
BUILD pass: the call over K); the whole walk as pam_conformers runs it after its matrix (BUILD, then chunks of 64 swaps with a
read of the status after each; host clock around it, synchronised) and the swaps it makes; agdiff_pam_swap from BUILD's medoids
and from the first K conformers with max_swaps set to the swaps that walk needs, at most 256 (so that every enqueued launch
works: the time per swap iteration).  Set against, on the same matrix in the same run: one agdiff_silhouette call on the final
clustering and one iteration of agdiff_kmedoids from the first K.  BUILD and the first 8 swaps are also compared with the numpy
restatement of the rule (tests/pam_ref.py).  Then the final costs: PAM against agdiff_kmedoids (max_iter = 128) from the first K,
the last K and the MaxMin picks.  Device events around a window of launches after a warm-up -- as many launches as fill
`--window-ms` -- medians over `--rounds` rounds.  The calls go through the Python wrappers (agdiff_amd.pam, .medoids, .silhouette),
which allocate the outputs and the scratch.  Not a test, and no figure is a gate.

    python tools/pam_time.py [--out profiles/pam_timing.txt]"""
import argparse, os, sys, time, types
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import pam_ref as PR
from agdiff_amd import _lib, pam
from agdiff_amd.medoids import kmedoids
from agdiff_amd.picks import maxmin_pick
from agdiff_amd.silhouette import silhouette

ap = argparse.ArgumentParser()
ap.add_argument("--window-ms", type=float, default=100.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
_lib.load()
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


def median_ms(fn):
    """(median, min, max, calls per window): warm-up, then windows of at least --window-ms of device time"""
    fn(); fn()
    torch.cuda.synchronize()
    once = max(timed(fn, 3), 1e-3)
    reps = int(min(max(args.window_ms / once, 3), 20000))
    v = np.array([timed(fn, reps) for _ in range(args.rounds)])
    return float(np.median(v)), float(v.min()), float(v.max()), reps


def host(t):
    return [x.cpu().numpy() for x in t[:6]] + [int(t[6]), int(t[7])]


say("agdiff_pam_build / agdiff_pam_swap on random metric matrices; windows of >= %.0f ms of calls per figure, median of %d rounds"
    % (args.window_ms, args.rounds))
for G in (1000, 4096):
    d = PR.random_metric(G, seed=G)
    q = PR.Q(d)
    dd = torch.from_numpy(d).to(dev)
    m = types.SimpleNamespace(total=G, G=G, mask=None, sel=None, gen=torch.zeros((G, 1, 3), device=dev), idx=None, out=dd, bits=None,
                              hand=None, ez_state=None)
    for K in (1, 10, 100):
        first = torch.arange(K, dtype=torch.int32, device=dev)
        # BUILD
        want = PR.build(d, K, q=q)
        med, lo, hi, reps = median_ms(lambda: pam.pam_build(dd, G, K))
        built = pam.pam_build(dd, G, K)
        say("G = %4d, K = %3d: agdiff_pam_build (%3d launches) median %8.4f ms  min %8.4f  max %8.4f  (%4d calls a window; equal to the "
            "restatement: %s): %.4f ms a BUILD pass (candidates + pick); cost %.3f"
            % (G, K, 2 * K + 3, med, lo, hi, reps, PR.same(host(built), want), med / K, float(built[5])))
        # the whole walk, as pam_conformers runs it after its matrix
        walk = lambda: pam._walk(m, K, "build", None, 4096, 64, False)
        res = walk()
        torch.cuda.synchronize()
        t = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            res = walk()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        say("    pam_conformers after its matrix (BUILD + chunks of 64 swaps, a status read after each): %d swaps, converged %s, host "
            "clock median %8.3f ms  min %8.3f  max %8.3f; cost %.3f (BUILD alone %.3f)"
            % (res["swaps"], res["converged"], float(np.median(t)), min(t), max(t), res["cost"], res["build_cost"]))
        # a swap iteration: every enqueued iteration works
        iter_ms = None
        for name, seeds in (("BUILD's medoids", built[0]), ("the first K", first)):
            whole, n, s = seeds, 0, 1
            while s == 1:                                    # the swaps the walk needs from these seeds
                r = pam.pam_swap(dd, G, whole, 0, 256)
                whole, n, s = r[0], n + int(r[6]), int(r[7])
            short = PR.swap(d, seeds.cpu().numpy(), 0, max_swaps=8, q=q)
            same = PR.same(host(pam.pam_swap(dd, G, seeds, 0, 8)), short)
            work = min(n, 256)
            if work == 0:
                med, lo, hi, reps = median_ms(lambda: pam.pam_swap(dd, G, seeds, 0, 1))
                say("    agdiff_pam_swap from %s: 0 swaps needed; max_swaps = 1 (one iteration that finds nothing, %d launches) median "
                    "%8.4f ms  min %8.4f  max %8.4f  (%4d calls a window; the first 8 swaps equal the restatement: %s)"
                    % (name, 6, med, lo, hi, reps, same))
                one = med
            else:
                med, lo, hi, reps = median_ms(lambda: pam.pam_swap(dd, G, seeds, 0, work))
                one = med / work
                say("    agdiff_pam_swap from %s: %d swaps needed; max_swaps = %d (%d launches) median %8.4f ms  min %8.4f  max %8.4f  "
                    "(%4d calls a window; the first 8 swaps equal the restatement: %s): %.4f ms a swap iteration (state + candidates + "
                    "choose); final cost %.3f" % (name, n, work, 3 * work + 3, med, lo, hi, reps, same, one, float(r[5])))
            iter_ms = one if iter_ms is None else iter_ms
        # one silhouette call on the final clustering, one k-medoids iteration from the first K: same matrix, same run
        labels = res["labels"]
        sil, lo, hi, reps = median_ms(lambda: silhouette(dd, G, labels, K))
        alt = kmedoids(dd, G, first, max_iter=128)
        updates = int(alt[6])
        kmed, klo, khi, kreps = median_ms(lambda: kmedoids(dd, G, first, max_iter=updates))
        say("    agdiff_silhouette on PAM's clustering median %8.4f ms  min %8.4f  max %8.4f  (%4d calls a window); agdiff_kmedoids from the "
            "first K (%d updates, max_iter = %d) median %8.4f ms: %.4f ms an iteration; a swap iteration (from BUILD's medoids) is %.2f x "
            "a silhouette call, %.2f x (a silhouette call + a k-medoids iteration)"
            % (sil, lo, hi, reps, updates, updates, kmed, kmed / updates, iter_ms / sil, iter_ms / (sil + kmed / updates)))
        # the final costs against the alternating walk's
        last = kmedoids(dd, G, torch.arange(G - K, G, dtype=torch.int32, device=dev), max_iter=128)
        picks = maxmin_pick(dd, G, K)[0]
        far = kmedoids(dd, G, picks, max_iter=128)
        say("    final cost: PAM (BUILD + SWAP) %.3f; agdiff_kmedoids %.3f from the first K (%d updates), %.3f from the last K (%d), %.3f "
            "from the MaxMin picks (%d)" % (res["cost"], float(alt[5]), updates, float(last[5]), int(last[6]), float(far[5]), int(far[6])))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
