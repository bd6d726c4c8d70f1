#!/usr/bin/env python3
"""Times of agdiff_silhouette on random metric matrices (the pairwise distances of random points) at G = 1000 and G = 4096 with
K = 2, 10, 100 and G clusters of uniformly random labels (K = 2 .. 100 take the one-row-per-wave shape of k_sil_rows, K = G above
1024 the one-row-per-workgroup shape), and of a 2 .. 12 sweep as agdiff_amd.silhouette.sweep_medoids enqueues it: one
agdiff_maxmin_pick, then agdiff_kmedoids (max_iter = 32) and agdiff_silhouette for every K.  Set against: the agdiff_rmsd_self
launch that makes the float matrix of a molecule of 25 heavy atoms with P = 1, agdiff_kmedoids alone with the same K (and its time
per iteration: k_kmed_costs streams the matrix once, like k_sil_rows), and the numpy restatement of the rule on the CPU
(tests/silhouette_ref.py).  Every timed launch is also compared with the restatement.  Device events around a window of launches
after a warm-up -- as many launches as fill `--window-ms` -- medians over `--rounds` rounds.  Not a test, and no figure is a gate.

    python tools/silhouette_timing.py [--out profiles/silhouette_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import kmedoids_ref as KR
import silhouette_ref as SR
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


say("agdiff_silhouette on random metric matrices, uniformly random labels; windows of >= %.0f ms of calls per figure, median of %d rounds"
    % (args.window_ms, args.rounds))
sil_ms, kmed_iter_ms = {}, {}
for G in (1000, 4096):
    d = KR.random_metric(G, seed=G)
    q = KR.Q(d)
    dd = torch.from_numpy(d).to(dev)
    a, b, s = (torch.empty(G, dtype=torch.float64, device=dev) for _ in range(3))
    other, labels_out = torch.empty(G, dtype=torch.int32, device=dev), torch.empty(G, dtype=torch.int32, device=dev)
    near = torch.empty(G, dtype=torch.float32, device=dev)
    mean, cost = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    status, n_iter = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    work = torch.empty(_lib.DEFINES["AGDIFF_SILHOUETTE_WORK_BYTES"] // 8, dtype=torch.int64, device=dev)
    kwork = torch.empty(_lib.DEFINES["AGDIFF_KMEDOIDS_WORK_BYTES"] // 8, dtype=torch.int64, device=dev)

    def sil_call(lab, K, size, cmean):
        return lambda: _lib.check(lib.agdiff_silhouette(_lib.ptr(dd), G, K, _lib.ptr(lab), _lib.ptr(a), _lib.ptr(b), _lib.ptr(s), _lib.ptr(other),
                                                        _lib.ptr(size), _lib.ptr(cmean), _lib.ptr(mean), _lib.ptr(status), _lib.ptr(work), st),
                                  "agdiff_silhouette")

    def kmed_call(init, K, max_iter, medoids, size, within):
        return lambda: _lib.check(lib.agdiff_kmedoids(_lib.ptr(dd), G, K, _lib.ptr(init), max_iter, _lib.ptr(medoids), _lib.ptr(labels_out),
                                                      _lib.ptr(near), _lib.ptr(size), _lib.ptr(within), _lib.ptr(cost), _lib.ptr(n_iter),
                                                      _lib.ptr(status), _lib.ptr(kwork), st), "agdiff_kmedoids")
    for K in (2, 10, 100, G):
        labels = np.random.default_rng(G + K).integers(0, K, size=G).astype(np.int32)
        lab = torch.from_numpy(labels).to(dev)
        size, cmean = torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.float64, device=dev)
        t0 = time.perf_counter()
        want = SR.silhouette(d, labels, K, q=q)
        cpu = (time.perf_counter() - t0) * 1e3
        med, lo, hi, reps = median_ms(sil_call(lab, K, size, cmean))
        got = (a.cpu().numpy(), b.cpu().numpy(), s.cpu().numpy(), other.cpu().numpy(), size.cpu().numpy(), cmean.cpu().numpy(),
               mean.cpu().numpy()[0], int(status.item()))
        sil_ms[(G, K)] = med
        say("G = %4d, K = %4d: agdiff_silhouette (3 launches, one row per %s) median %8.4f ms  min %8.4f  max %8.4f  (%5d calls a window; "
            "equal to the restatement: %s; mean silhouette %+.4f); numpy on the CPU %.1f ms"
            % (G, K, "wave" if K <= 1024 else "workgroup", med, lo, hi, reps, SR.same(got, want), got[6], cpu))
    # agdiff_kmedoids from the first K conformers, max_iter = the updates the walk needs: the time per iteration, whose member-costs
    # launch streams the matrix once as k_sil_rows does
    for K in (2, 10, 100):
        init = torch.arange(K, dtype=torch.int32, device=dev)
        medoids, size = torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.int32, device=dev)
        within = torch.empty(K, dtype=torch.float64, device=dev)
        updates = KR.kmedoids(d, list(range(K)), max_iter=64, q=q)[6]
        med, lo, hi, reps = median_ms(kmed_call(init, K, updates, medoids, size, within))
        kmed_iter_ms[(G, K)] = med / updates
        say("G = %4d, K = %4d: agdiff_kmedoids (%2d updates, max_iter = %2d) median %8.4f ms  min %8.4f  max %8.4f  (%5d calls a window): %.4f ms "
            "an iteration (assign + member costs + choose); agdiff_silhouette is %.2f x one iteration"
            % (G, K, updates, updates, med, lo, hi, reps, med / updates, sil_ms[(G, K)] / (med / updates)))
    # the sweep as sweep_medoids enqueues it, 2 .. 12 from MaxMin seeds: nothing synchronises between the launches
    lo_k, hi_k = 2, 12
    picks, radius = torch.empty(hi_k, dtype=torch.int32, device=dev), torch.empty(hi_k, dtype=torch.float32, device=dev)
    n, cover = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
    outs = {K: (torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.int32, device=dev),
                torch.empty(K, dtype=torch.float64, device=dev), torch.empty(K, dtype=torch.float64, device=dev)) for K in range(lo_k, hi_k + 1)}
    means = torch.empty(hi_k + 1, dtype=torch.float64, device=dev)

    def sweep():
        _lib.check(lib.agdiff_maxmin_pick(_lib.ptr(dd), G, hi_k, 0, -1.0, _lib.ptr(picks), _lib.ptr(radius), _lib.ptr(labels_out), _lib.ptr(near),
                                          _lib.ptr(n), _lib.ptr(cover), st), "agdiff_maxmin_pick")
        for K in range(lo_k, hi_k + 1):
            medoids, size, within, cmean = outs[K]
            kmed_call(picks, K, 32, medoids, size, within)()
            _lib.check(lib.agdiff_silhouette(_lib.ptr(dd), G, K, _lib.ptr(labels_out), _lib.ptr(a), _lib.ptr(b), _lib.ptr(s), _lib.ptr(other),
                                             _lib.ptr(size), _lib.ptr(cmean), _lib.ptr(means[K:K + 1]), _lib.ptr(status), _lib.ptr(work), st),
                       "agdiff_silhouette")
    med, lo, hi, reps = median_ms(sweep)
    seeds = KR.maxmin(d, hi_k)[0]
    t0 = time.perf_counter()
    want = [SR.silhouette(d, KR.kmedoids(d, seeds[:K].tolist(), q=q)[1], K, q=q)[6] for K in range(lo_k, hi_k + 1)]
    cpu = (time.perf_counter() - t0) * 1e3
    got = means.cpu().numpy()[lo_k:]
    say("G = %4d: the sweep K = %d .. %d (1 MaxMin launch, then per K agdiff_kmedoids with max_iter = 32 and agdiff_silhouette: %d launches "
        "enqueued) median %8.4f ms  min %8.4f  max %8.4f  (%d sweeps a window; the curve equal to the restatement: %s; best K = %d, mean "
        "silhouette %.4f); the restatements on the CPU %.1f ms"
        % (G, lo_k, hi_k, 1 + (hi_k - lo_k + 1) * (3 * 32 + 3 + 3), med, lo, hi, reps, SR.same((got,), (np.array(want),)),
           lo_k + int(np.argmax(got)), float(got.max()), cpu))

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
    for K in (2, 10, 100, G):
        say("    agdiff_silhouette K = %4d: %.3f x that launch%s" % (K, sil_ms[(G, K)] / med, " -- the scoring is the slow step" if sil_ms[(G, K)] > med else ""))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
