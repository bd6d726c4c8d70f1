#!/usr/bin/env python3
"""Times of the geometry-validity kernels, by tools/stereo_timing.py's method: device events around `--reps` launches after a warm-up,
`--rounds` rounds, the calls alternating round by round in this one process, medians.

agdiff_pair_bounds and agdiff_clash_scan on G = 1000 conformers of n = 44 atoms (a Drugs-sized molecule), and the scan on G = 8
conformers of n = 4096 and n = 16,384 atoms; beside each, as context, agdiff_rmsd_self on the same conformers (m heavy atoms, capped
at AGDIFF_RMSD_MAX_ATOMS; identity mapping): the matrix a prune pays for.  The molecules are random trees with their order-3 exclusions
and a random-walk geometry (tests build them the same way); a record, not a gate.

    python tools/validity_timing.py [--out profiles/validity_timing.txt]"""
import argparse, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from agdiff_amd import _lib
from agdiff_amd.ensemble import bits_pitch
from agdiff_amd.validity import CLASH_SLICE, exclusions

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


def molecule(rng, n, G):
    """a random tree (parent among the previous three atoms), its bonds, its order-3 exclusions by breadth-first search (the dense
    adjacency powers of synth.extend_graph_order_np do not fit 16,384 atoms), and G random-walk geometries with 1.5 A steps"""
    parent = np.array([0] + [int(rng.integers(max(0, a - 3), a)) for a in range(1, n)])
    adj = [[] for _ in range(n)]
    for a in range(1, n):
        adj[a].append(parent[a]); adj[parent[a]].append(a)
    src, dst = [], []
    for i in range(n):
        seen, frontier = {i}, [i]
        for _ in range(3):
            frontier = [j for f in frontier for j in adj[f] if j not in seen and not seen.add(j)]
            src += [i] * len(frontier); dst += frontier
    ex_ptr, ex_idx = exclusions(n, np.array([src, dst]), np.ones(len(src), dtype=np.int64))
    pos = np.zeros((G, n, 3))
    for a in range(1, n):
        d = rng.normal(size=(G, 3))
        pos[:, a] = pos[:, parent[a]] + 1.5 * d / np.linalg.norm(d, axis=1, keepdims=True)
    bonds = np.array([[parent[a], a] for a in range(1, n)], dtype=np.int32)
    return pos.astype(np.float32), bonds, ex_ptr, ex_idx


def measure(G, n, with_bounds):
    rng = np.random.default_rng(2021 + n)
    pos_np, bonds, ex_ptr_np, ex_idx_np = molecule(rng, n, G)
    m = min(int(0.55 * n), _lib.DEFINES["AGDIFF_RMSD_MAX_ATOMS"])
    K, S = bonds.shape[0], (n + CLASH_SLICE - 1) // CLASH_SLICE
    say("G = %d conformers, n = %d atoms, K = %d bonded pairs, %d excluded pairs of %d, S = %d slices; agdiff_rmsd_self over m = %d atoms"
        % (G, n, K, ex_idx_np.shape[0] // 2, n * (n - 1) // 2, S, m))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pos, pairs, ex_ptr, ex_idx = T(pos_np), T(bonds), T(ex_ptr_np), T(ex_idx_np)
    lo, hi = T(np.full(K, 1.1, np.float32)), T(np.full(K, 1.8, np.float32))
    radius = T(np.full(n, 1.7, np.float32))
    worst, min_ratio = (torch.empty(G, dtype=torch.float32, device=dev) for _ in range(2))
    worst_pair, n_bad, n_clash = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(3))
    min_pair = torch.empty((G, 2), dtype=torch.int32, device=dev)
    scratch = torch.empty((G, S, 4), dtype=torch.int32, device=dev)
    idx = torch.arange(m, dtype=torch.int32, device=dev)
    out_r = torch.empty((G, G), dtype=torch.float32, device=dev)
    bits_r = torch.empty((G, bits_pitch(G) // 8), dtype=torch.int64, device=dev)
    scratch_r = torch.empty(G * (3 * m + 1), dtype=torch.float32, device=dev)
    st = _lib.stream_ptr()

    def run_bounds():
        _lib.check(lib.agdiff_pair_bounds(_lib.ptr(pos), _lib.ptr(pairs), _lib.ptr(lo), _lib.ptr(hi), G, n, K, _lib.ptr(None), _lib.ptr(worst),
                                          _lib.ptr(worst_pair), _lib.ptr(n_bad), st), "agdiff_pair_bounds")

    def run_clash():
        _lib.check(lib.agdiff_clash_scan(_lib.ptr(pos), _lib.ptr(radius), _lib.ptr(ex_ptr), _lib.ptr(ex_idx), G, n, 0.6, _lib.ptr(scratch),
                                         _lib.ptr(min_ratio), _lib.ptr(min_pair), _lib.ptr(n_clash), st), "agdiff_clash_scan")

    def run_rmsd():
        _lib.check(lib.agdiff_rmsd_self(_lib.ptr(pos), _lib.ptr(idx), _lib.ptr(None), G, n, m, 0, 0.5, _lib.ptr(scratch_r), _lib.ptr(out_r),
                                        _lib.ptr(bits_r), st), "agdiff_rmsd_self")

    calls = ([("agdiff_pair_bounds", run_bounds)] if with_bounds else []) + [("agdiff_clash_scan", run_clash), ("agdiff_rmsd_self (out + bits)", run_rmsd)]
    for _, fn in calls:                         # warm-up: code objects
        fn(); fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in calls}
    for _ in range(args.rounds):
        for name, fn in calls:
            ms[name].append(timed(fn, args.reps))
    ref = np.median(ms["agdiff_rmsd_self (out + bits)"])
    for name, _ in calls:
        v = np.array(ms[name])
        say("  %-32s median %9.4f ms  min %9.4f  max %9.4f   (%.4f x agdiff_rmsd_self)" % (name, np.median(v), v.min(), v.max(), np.median(v) / ref))
    pairs_scanned = G * (n * (n - 1) // 2 - ex_idx_np.shape[0] // 2)
    say("  clash scan: %.3g pairs per launch, %.1f G pairs / s; %d conformers with a clash, smallest ratio %.3f"
        % (pairs_scanned, pairs_scanned / np.median(ms["agdiff_clash_scan"]) * 1e-6, int((n_clash > 0).sum()), float(min_ratio.min())))


say("geometry validity kernels; %d launches per figure, medians of %d alternating rounds" % (args.reps, args.rounds))
measure(1000, 44, True)
measure(8, 4096, False)
measure(8, 16384, False)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
