#!/usr/bin/env python3
"""Times of agdiff_linkage and agdiff_linkage_cut on random metric matrices (the pairwise distances of random points, the matrices
of tools/medoid_timing.py) at G = 1000 and G = 4096, per method: the tree (2 (G - 1) + 3 dependent launches), one cut (count = 5:
four launches) and a 2 .. 12 sweep over the finished tree as agdiff_amd.linkage.sweep_linkage enqueues it (a cut and an
agdiff_silhouette for every K).  Set against, on the same matrix in the same run: the agdiff_rmsd_self launch that makes the float
matrix of a molecule of 25 heavy atoms with P = 1, a 2 .. 12 sweep as agdiff_amd.silhouette.sweep_medoids enqueues it (one
agdiff_maxmin_pick, then agdiff_kmedoids with max_iter = 32 and agdiff_silhouette for every K), and scipy.cluster.hierarchy.linkage
on this host's CPU (the numpy restatement, tests/linkage_ref.py, where scipy is absent).  Every tree is compared with the
restatement at G = 1000 and with scipy's heights at both sizes.  Device events around a window of calls after a warm-up -- as many
calls as fill `--window-ms` -- medians over `--rounds` rounds.  The calls go through the Python wrappers, which allocate the outputs
and the scratch (8 G G bytes for a tree).  Not a test, and no figure is a gate.

    python tools/linkage_time.py [--out profiles/linkage_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import linkage_ref as LR
from agdiff_amd import _lib
from agdiff_amd.linkage import METHODS, cut_tree, linkage
from agdiff_amd.medoids import kmedoids
from agdiff_amd.picks import maxmin_pick
from agdiff_amd.silhouette import silhouette
try:
    from scipy.cluster import hierarchy
    from scipy.spatial.distance import squareform
except ImportError:
    hierarchy = None

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
    """(median, min, max, calls per window): warm-up, then windows of at least --window-ms of device time"""
    fn(); fn()
    torch.cuda.synchronize()
    once = max(timed(fn, 3), 1e-3)
    reps = int(min(max(args.window_ms / once, 3), 20000))
    v = np.array([timed(fn, reps) for _ in range(args.rounds)])
    return float(np.median(v)), float(v.min()), float(v.max()), reps


def host_tree(t):
    return [x.cpu().numpy() for x in t[:5]] + [int(t[5])]


say("agdiff_linkage / agdiff_linkage_cut on random metric matrices; windows of >= %.0f ms of calls per figure, median of %d rounds"
    % (args.window_ms, args.rounds))
LO, HI = 2, 12
natoms, m = 44, 25
rng = np.random.default_rng(2021)
for G in (1000, 4096):
    d = LR.random_metric(G, seed=G)
    dd = torch.from_numpy(d).to(dev)
    # the launch that produces such a matrix: one molecule, 25 heavy atoms of 44, identity mapping only (P = 1)
    pos = torch.from_numpy((rng.normal(size=(natoms, 3))[None] * 1.5 + 0.25 * rng.normal(size=(G, natoms, 3))).astype(np.float32)).to(dev)
    idx = torch.arange(m, dtype=torch.int32, device=dev)
    scratch = torch.empty(G * (3 * m + 1), dtype=torch.float32, device=dev)
    out = torch.empty((G, G), dtype=torch.float32, device=dev)
    fn = lambda: _lib.check(lib.agdiff_rmsd_self(_lib.ptr(pos), _lib.ptr(idx), _lib.ptr(None), G, natoms, m, 0, 0.0, _lib.ptr(scratch),
                                                 _lib.ptr(out), _lib.ptr(None), st), "agdiff_rmsd_self")
    matrix_ms, lo, hi, reps = median_ms(fn)
    say("G = %4d: agdiff_rmsd_self (out only; n = %d, m = %d, P = 1) median %8.4f ms  min %8.4f  max %8.4f  (%d launches a window)"
        % (G, natoms, m, matrix_ms, lo, hi, reps))

    # the k-medoids sweep on the same matrix, as sweep_medoids enqueues it: nothing synchronises between the launches
    def medoid_sweep():
        picks = maxmin_pick(dd, G, HI)[0]
        return [silhouette(dd, G, kmedoids(dd, G, picks[:K].contiguous(), max_iter=32)[1], K)[6] for K in range(LO, HI + 1)]
    kmed_ms, lo, hi, reps = median_ms(medoid_sweep)
    curve = torch.cat(medoid_sweep()).cpu().numpy()
    say("G = %4d: the k-medoids sweep K = %d .. %d (1 MaxMin launch, then per K agdiff_kmedoids with max_iter = 32 and agdiff_silhouette) "
        "median %8.4f ms  min %8.4f  max %8.4f  (%d sweeps a window; best K = %d, mean silhouette %.4f)"
        % (G, LO, HI, kmed_ms, lo, hi, reps, LO + int(np.argmax(curve)), float(curve.max())))
    for method in METHODS:
        tree_ms, lo, hi, reps = median_ms(lambda: linkage(dd, G, method))
        tree = linkage(dd, G, method)
        got = host_tree(tree)
        same = "not compared"
        if G <= 1000:
            t0 = time.perf_counter()
            want = LR.linkage(d, method)
            same = "%s (the restatement on the CPU: %.0f ms)" % (LR.same_tree(got, want), (time.perf_counter() - t0) * 1e3)
        say("G = %4d, %-8s: agdiff_linkage (%4d launches) median %9.4f ms  min %9.4f  max %9.4f  (%3d calls a window): %.4f ms a merge "
            "(choose + update); %.2f x the agdiff_rmsd_self launch%s; equal to the restatement: %s"
            % (G, method, 2 * (G - 1) + 3, tree_ms, lo, hi, reps, tree_ms / (G - 1), tree_ms / matrix_ms,
               " -- the tree is the slow step" if tree_ms > matrix_ms else "", same))
        if hierarchy is not None:
            t0 = time.perf_counter()
            Z = hierarchy.linkage(squareform(d.astype(np.float64), checks=False), method=method)
            cpu = (time.perf_counter() - t0) * 1e3
            say("    scipy.cluster.hierarchy.linkage on this host's CPU (float64, the condensed matrix made before the clock): %.1f ms; max "
                "|height - scipy's| over the sorted heights = %.3e (2^-28 = %.3e)"
                % (cpu, float(np.abs(np.sort(got[2][:G - 1]) - np.sort(Z[:, 2])).max()), 2.0 ** -28))
        cut_ms, lo, hi, reps = median_ms(lambda: cut_tree(dd, G, tree, count=5))
        say("    agdiff_linkage_cut (count = 5; 4 launches) median %8.4f ms  min %8.4f  max %8.4f  (%d calls a window)" % (cut_ms, lo, hi, reps))

        def tree_sweep():
            return [silhouette(dd, G, cut_tree(dd, G, tree, count=K)[1], K)[6] for K in range(LO, HI + 1)]
        sweep_ms, lo, hi, reps = median_ms(tree_sweep)
        curve = torch.cat(tree_sweep()).cpu().numpy()
        say("    the sweep K = %d .. %d over the finished tree (per K agdiff_linkage_cut and agdiff_silhouette) median %8.4f ms  min %8.4f  "
            "max %8.4f  (%d sweeps a window; best K = %d, mean silhouette %.4f); tree + sweep %.3f ms = %.2f x the k-medoids sweep"
            % (LO, HI, sweep_ms, lo, hi, reps, LO + int(np.argmax(curve)), float(curve.max()), tree_ms + sweep_ms,
               (tree_ms + sweep_ms) / kmed_ms))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
