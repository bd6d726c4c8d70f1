#!/usr/bin/env python3
"""Times of agdiff_butina_cluster on random symmetric adjacencies, in both modes, against agdiff_leader_prune ON THE SAME BITS (the
kernel that was there before, the yardstick) and against the numpy restatement of the rule on the CPU (tests/butina_ref.py, its
running-count form); then, at G = 4096, against the agdiff_rmsd_self launch that produces such bits for a molecule of 25 heavy
atoms with P = 1.  Device events around `--reps` launches after a warm-up, medians over `--rounds` rounds.  Not a test.

    python tools/cluster_timing.py [--out profiles/cluster_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import butina_ref as BR
from agdiff_amd import _lib, ensemble

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
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
    fn(); fn()
    torch.cuda.synchronize()
    v = np.array([timed(fn, args.reps) for _ in range(args.rounds)])
    return float(np.median(v)), float(v.min()), float(v.max())


say("agdiff_butina_cluster against agdiff_leader_prune on the same bits; %d launches per figure, median of %d rounds" % (args.reps, args.rounds))
butina_4096 = {}
PAIRS = -1.0        # in the density's place: 2048 disjoint pairs, the longest loop there is (a conformer without a neighbour is not iterated over)
for G, density in ((1000, 0.02), (4096, 0.0), (4096, 0.02), (4096, 0.5), (4096, PAIRS)):
    if density == PAIRS:
        adj = BR.graph(G, [(i, i + G // 2) for i in range(G // 2)])
        density = 2.0 / G
    else:
        adj = BR.random_graph(G, density, seed=G + int(100 * density))
    b = torch.from_numpy(BR.pack(adj)).to(dev)
    keep, leader, count, rank = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(4))
    n = torch.empty(1, dtype=torch.int32, device=dev)
    prune = lambda: _lib.check(lib.agdiff_leader_prune(_lib.ptr(b), G, _lib.ptr(keep), _lib.ptr(leader), _lib.ptr(count), _lib.ptr(n), st),
                               "agdiff_leader_prune")
    p_med, p_min, p_max = median_ms(prune)
    say("G = %4d, density %.4f: agdiff_leader_prune              (%4d kept)     median %8.4f ms  min %8.4f  max %8.4f"
        % (G, density, int(n[0].item()), p_med, p_min, p_max))
    for reorder in (1, 0):
        fn = lambda: _lib.check(lib.agdiff_butina_cluster(_lib.ptr(b), G, reorder, _lib.ptr(leader), _lib.ptr(count), _lib.ptr(rank),
                                                          _lib.ptr(n), st), "agdiff_butina_cluster")
        med, lo, hi = median_ms(fn)
        got = (leader.cpu().numpy(), count.cpu().numpy(), rank.cpu().numpy())
        t0 = time.perf_counter()
        want = BR.butina(adj, bool(reorder), running=True)
        cpu = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(x, y) for x, y in zip(got, want))
        say("G = %4d, density %.4f: agdiff_butina_cluster reorder = %d (%4d clusters) median %8.4f ms  min %8.4f  max %8.4f   "
            "(%.2f x agdiff_leader_prune; numpy on the CPU %.1f ms; equal to it: %s)"
            % (G, density, reorder, int(n[0].item()), med, lo, hi, med / p_med, cpu, same))
        if G == 4096 and reorder == 1 and density not in butina_4096:
            butina_4096[density] = med

# the launch that produces the bits: one molecule, 25 heavy atoms of 44, identity mapping only (P = 1)
G, natoms, m = 4096, 44, 25
rng = np.random.default_rng(2021)
pos = torch.from_numpy((rng.normal(size=(natoms, 3))[None] * 1.5 + 0.25 * rng.normal(size=(G, natoms, 3))).astype(np.float32)).to(dev)
idx = torch.arange(m, dtype=torch.int32, device=dev)
bits = torch.empty((G, ensemble.bits_pitch(G) // 8), dtype=torch.int64, device=dev)
scratch = torch.empty(G * (3 * m + 1), dtype=torch.float32, device=dev)
for what, out in (("bits only", None), ("out + bits", torch.empty((G, G), dtype=torch.float32, device=dev))):
    fn = lambda: _lib.check(lib.agdiff_rmsd_self(_lib.ptr(pos), _lib.ptr(idx), _lib.ptr(None), G, natoms, m, 0, 0.5, _lib.ptr(scratch),
                                                 _lib.ptr(out), _lib.ptr(bits), st), "agdiff_rmsd_self")
    med, lo, hi = median_ms(fn)
    say("G = %4d: agdiff_rmsd_self (%s; n = %d, m = %d, P = 1) median %8.4f ms  min %8.4f  max %8.4f" % (G, what, natoms, m, med, lo, hi))
    for density, ms in sorted(butina_4096.items()):
        say("    agdiff_butina_cluster reorder = 1 at density %.4f: %.2f x that launch%s"
            % (density, ms / med, " -- the clustering is the slow step" if ms > med else ""))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
