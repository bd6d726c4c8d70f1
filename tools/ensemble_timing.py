#!/usr/bin/env python3
"""Times of the conformer-ensemble kernels on one molecule (G conformers, n atoms, m heavy atoms, P atom mappings):
agdiff_rmsd_self (matrix + threshold bits; upper-triangular tiles) against agdiff_rmsd_matrix(pos, pos) (every pair twice) on
the same inputs, agdiff_leader_prune, and the wall times of ensemble.prune_conformers and clusters.cluster_conformers.  Device events around `--reps` launches
after a warm-up, the two matrix calls alternating round by round in this one process.

--parent-lib PATH: the full-matrix call is ALSO taken from that build of libagdiff_hip.so (an older commit's, as AGDIFF_LIB
would load it) and timed in the same rounds -- "no slower than what was there before" measured on one device in one process.

    python tools/ensemble_timing.py [--parent-lib _ab/parent/libagdiff_hip.so] [--out profiles/ensemble_timing.txt]"""
import argparse, ctypes, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from agdiff_amd import _lib, clusters, ensemble

ap = argparse.ArgumentParser()
ap.add_argument("--G", type=int, default=1000)
ap.add_argument("--n", type=int, default=44)
ap.add_argument("--m", type=int, default=25)
ap.add_argument("--perms", type=int, nargs="+", default=[4, 64])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lib = _lib.load()
libs = [("this build", lib)]
if args.parent_lib:
    old = ctypes.CDLL(os.path.abspath(args.parent_lib))
    old.agdiff_rmsd_matrix.restype = ctypes.c_int
    old.agdiff_rmsd_matrix.argtypes = _lib.EXPORTS["agdiff_rmsd_matrix"]
    libs.append(("parent build", old))
dev = torch.device("cuda", 0)
rng = np.random.default_rng(2021)
G, n, m = args.G, args.n, args.m
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


def group_of(P, m):
    """P mappings closed under inversion: products of the disjoint swaps (0 1), (2 3), ... (a group of 2^k elements)"""
    k = int(np.log2(P))
    assert 1 << k == P and 2 * k <= m
    out = []
    for mask in range(P):
        p = np.arange(m)
        for b in range(k):
            if mask >> b & 1:
                p[[2 * b, 2 * b + 1]] = p[[2 * b + 1, 2 * b]]
        out.append(p)
    return np.stack(out).astype(np.int32)


say("conformer-ensemble kernels: G = %d conformers, n = %d atoms, m = %d heavy atoms; %d launches per figure, %d alternating rounds"
    % (G, n, m, args.reps, args.rounds))
at = np.r_[np.full(m, 6), np.full(n - m, 1)]
base = rng.normal(size=(n, 3)) * 1.5
pos_np = (base[None] + 0.25 * rng.normal(size=(G, n, 3))).astype(np.float32)
pos = torch.from_numpy(pos_np).to(dev)
idx = torch.arange(m, dtype=torch.int32, device=dev)
st = _lib.stream_ptr()
for P in args.perms:
    perms = torch.from_numpy(group_of(P, m)).to(dev)
    out_self = torch.empty((G, G), dtype=torch.float32, device=dev)
    bits = torch.empty((G, ensemble.bits_pitch(G) // 8), dtype=torch.int64, device=dev)
    scr_self = torch.empty(G * (3 * m + 1), dtype=torch.float32, device=dev)
    scr_full = torch.empty(2 * G * (3 * m + 1), dtype=torch.float32, device=dev)
    outs_full = [torch.empty((G, G), dtype=torch.float32, device=dev) for _ in libs]

    def run_self():
        _lib.check(lib.agdiff_rmsd_self(_lib.ptr(pos), _lib.ptr(idx), _lib.ptr(perms), G, n, m, P, 0.5, _lib.ptr(scr_self),
                                        _lib.ptr(out_self), _lib.ptr(bits), st), "agdiff_rmsd_self")

    def run_full(k):
        _lib.check(libs[k][1].agdiff_rmsd_matrix(_lib.ptr(pos), _lib.ptr(pos), _lib.ptr(idx), _lib.ptr(perms), G, G, n, m, P,
                                                 _lib.ptr(scr_full), _lib.ptr(outs_full[k]), st), "agdiff_rmsd_matrix")
    calls = [("agdiff_rmsd_self (out + bits)", run_self)] + [("agdiff_rmsd_matrix(pos, pos), %s" % name, (lambda k=k: run_full(k)))
                                                             for k, (name, _) in enumerate(libs)]
    for _, fn in calls:                     # warm-up: code objects, the LDS attribute
        fn(); fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in calls}
    for _ in range(args.rounds):
        for name, fn in calls:
            ms[name].append(timed(fn, args.reps))
    for k in range(len(libs)):              # same inputs, same answers
        d = float((out_self - outs_full[k]).abs().max())
        say("P = %d: max |self - full (%s)| = %.3e Angstrom; self symmetric: %s" % (P, libs[k][0], d, bool(torch.equal(out_self, out_self.T))))
    ref = "agdiff_rmsd_matrix(pos, pos), %s" % libs[-1][0]
    for name, _ in calls:
        v = np.array(ms[name])
        say("P = %d: %-48s median %8.3f ms  min %8.3f  max %8.3f   (%.2f x %s)"
            % (P, name, np.median(v), v.min(), v.max(), np.median(v) / np.median(ms[ref]), libs[-1][0]))

# the leader kernel alone, on random symmetric adjacencies: sparse (2 %: many kept) and dense (50 %: few kept)
for Gp in (1000, 4096):
    for density in (0.02, 0.5):
        adj = np.triu(rng.random((Gp, Gp)) < density, 1)
        adj = adj | adj.T | np.eye(Gp, dtype=bool)
        wide = np.zeros((Gp, 8 * ensemble.bits_pitch(Gp)), dtype=np.uint8)
        wide[:, :Gp] = adj
        b = torch.from_numpy(np.packbits(wide, axis=1, bitorder="little").view(np.int64).copy()).to(dev)
        ensemble.leader_prune(b, Gp)
        torch.cuda.synchronize()
        keep, leader, count, nk = (torch.empty(Gp, dtype=torch.int32, device=dev) for _ in range(4))
        fn = lambda: _lib.check(lib.agdiff_leader_prune(_lib.ptr(b), Gp, _lib.ptr(keep), _lib.ptr(leader), _lib.ptr(count), _lib.ptr(nk), st),
                                "agdiff_leader_prune")
        v = np.array([timed(fn, args.reps) for _ in range(args.rounds)])
        say("agdiff_leader_prune G = %4d, density %.2f (%4d kept): median %.4f ms  min %.4f  max %.4f"
            % (Gp, density, int(nk[0].item()), np.median(v), v.min(), v.max()))

# prune_conformers end to end (host: selection, uploads, three launches + the alignment, one synchronising nonzero)
for P in args.perms:
    item = {"atom_type": at, "pos_gen": pos_np, "perms": group_of(P, m)}
    for align in (False, True):
        ensemble.prune_conformers(item, 0.5, align=align, device=dev)
        torch.cuda.synchronize()
        walls = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            res = ensemble.prune_conformers(item, 0.5, align=align, device=dev)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        say("prune_conformers G = %d, P = %d, align=%s: wall median %.2f ms  min %.2f  max %.2f  (%d kept)"
            % (G, P, align, np.median(walls), min(walls), max(walls), int(res["kept"].shape[0])))
        # clusters.cluster_conformers on the same item: the same prelude and matrix launch (plus the float matrix), Butina's walk
        clusters.cluster_conformers(item, 0.5, align=align, device=dev)
        torch.cuda.synchronize()
        walls = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            res = clusters.cluster_conformers(item, 0.5, align=align, device=dev)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        say("cluster_conformers G = %d, P = %d, align=%s: wall median %.2f ms  min %.2f  max %.2f  (%d clusters)"
            % (G, P, align, np.median(walls), min(walls), max(walls), int(res["centroids"].shape[0])))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
