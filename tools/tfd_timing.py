#!/usr/bin/env python3
"""Times of the torsion kernels on one molecule, by tools/stereo_timing.py's method: device events around `--reps` launches after a
warm-up, `--rounds` rounds, the calls alternating round by round in this one process, medians.

agdiff_torsion_angles (G conformers, n atoms, Q columns) and agdiff_tfd_matrix (self matrix with bits; T torsions, P mappings) against
agdiff_rmsd_self on the same conformers (m heavy atoms, P atom mappings): the matrix a prune by RMSD pays for.

    python tools/tfd_timing.py [--out profiles/tfd_timing.txt]"""
import argparse, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from agdiff_amd import _lib
from agdiff_amd.ensemble import bits_pitch

ap = argparse.ArgumentParser()
ap.add_argument("--G", type=int, default=1000)
ap.add_argument("--n", type=int, default=44)
ap.add_argument("--m", type=int, default=25)
ap.add_argument("--T", type=int, default=8)
ap.add_argument("--P", type=int, default=4)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lib = _lib.load()
dev = torch.device("cuda", 0)
rng = np.random.default_rng(2021)
G, n, m, T, P = args.G, args.n, args.m, args.T, args.P
Q = 2 * T                                           # two columns per torsion: the canonical one and one a symmetry leads to
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


say("torsion kernels: G = %d conformers, n = %d atoms, m = %d heavy atoms, T = %d torsions in Q = %d columns, P = %d mappings; "
    "%d launches per figure, %d alternating rounds" % (G, n, m, T, Q, P, args.reps, args.rounds))
base = rng.normal(size=(n, 3)) * 1.5
pos = torch.from_numpy((base[None] + 0.25 * rng.normal(size=(G, n, 3))).astype(np.float32)).to(dev)
quads = torch.from_numpy(np.stack([rng.permutation(m)[:4] for _ in range(Q)]).astype(np.int32)).to(dev)
# P column mappings: row 0 the even columns, row p swaps the two columns of the torsions in p's bit pattern
tmap_np = np.stack([2 * np.arange(T) + ((p >> (np.arange(T) % 2)) & 1) for p in range(P)]).astype(np.int32)
tmap = torch.from_numpy(tmap_np).to(dev)
# P atom mappings closed under inversion, as tools/stereo_timing.py builds them
k = int(np.log2(P))
assert 1 << k == P and 2 * k <= m
perms_np = []
for mask in range(P):
    p = np.arange(m)
    for b in range(k):
        if mask >> b & 1:
            p[[2 * b, 2 * b + 1]] = p[[2 * b + 1, 2 * b]]
    perms_np.append(p)
perms = torch.from_numpy(np.stack(perms_np).astype(np.int32)).to(dev)
idx = torch.arange(m, dtype=torch.int32, device=dev)
ang = torch.empty((G, Q), dtype=torch.float32, device=dev)
out_t, out_r = (torch.empty((G, G), dtype=torch.float32, device=dev) for _ in range(2))
bits_t, bits_r = (torch.empty((G, bits_pitch(G) // 8), dtype=torch.int64, device=dev) for _ in range(2))
scratch = torch.empty(G * (3 * m + 1), dtype=torch.float32, device=dev)
st = _lib.stream_ptr()


def run_angles():
    _lib.check(lib.agdiff_torsion_angles(_lib.ptr(pos), _lib.ptr(quads), G, n, Q, _lib.ptr(ang), st), "agdiff_torsion_angles")


def run_tfd():
    _lib.check(lib.agdiff_tfd_matrix(_lib.ptr(ang), _lib.ptr(ang), _lib.ptr(tmap), _lib.ptr(None), G, G, Q, T, P, 0.2, _lib.ptr(out_t),
                                     _lib.ptr(None), _lib.ptr(bits_t), st), "agdiff_tfd_matrix")


def run_rmsd():
    _lib.check(lib.agdiff_rmsd_self(_lib.ptr(pos), _lib.ptr(idx), _lib.ptr(perms), G, n, m, P, 0.5, _lib.ptr(scratch), _lib.ptr(out_r),
                                    _lib.ptr(bits_r), st), "agdiff_rmsd_self")


calls = [("agdiff_torsion_angles", run_angles), ("agdiff_tfd_matrix (out + bits)", run_tfd), ("agdiff_rmsd_self (out + bits)", run_rmsd)]
for _, fn in calls:                         # warm-up: code objects
    fn(); fn()
torch.cuda.synchronize()
ms = {name: [] for name, _ in calls}
for _ in range(args.rounds):
    for name, fn in calls:
        ms[name].append(timed(fn, args.reps))
say("TFD matrix symmetric: %s; %.1f %% of the pairs within TFD 0.2, %.1f %% within RMSD 0.5"
    % (bool(torch.equal(out_t, out_t.T)), 100.0 * float((out_t <= 0.2).float().mean()), 100.0 * float((out_r <= 0.5).float().mean())))
ref = np.median(ms["agdiff_rmsd_self (out + bits)"])
for name, _ in calls:
    v = np.array(ms[name])
    say("%-34s median %8.4f ms  min %8.4f  max %8.4f   (%.4f x agdiff_rmsd_self)" % (name, np.median(v), v.min(), v.max(), np.median(v) / ref))
both = np.median(ms["agdiff_torsion_angles"]) + np.median(ms["agdiff_tfd_matrix (out + bits)"])
say("angles + TFD matrix: %.4f ms = %.4f x agdiff_rmsd_self" % (both, both / ref))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
