#!/usr/bin/env python3
"""Times of the handedness kernels on one molecule, by tools/ensemble_timing.py's method: device events around `--reps` launches
after a warm-up, `--rounds` rounds, the calls alternating round by round in this one process, medians.

agdiff_rmsd_matrix_hands (two matrices) against agdiff_rmsd_matrix (one) of this build and -- with --parent-lib PATH -- of an older
commit's build of libagdiff_hip.so, on the same inputs: R = G conformers, m heavy atoms, P atom mappings.  Then
agdiff_chiral_verdict and agdiff_mirror_conformers at G conformers, n atoms, C centres.

    python tools/stereo_timing.py [--parent-lib _ab/parent/libagdiff_hip.so] [--out profiles/stereo_timing.txt]"""
import argparse, ctypes, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from agdiff_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--G", type=int, default=1000)
ap.add_argument("--n", type=int, default=44)
ap.add_argument("--m", type=int, default=25)
ap.add_argument("--C", type=int, default=4)
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
G, n, m, C = args.G, args.n, args.m, args.C
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


say("handedness kernels: R = G = %d conformers, n = %d atoms, m = %d heavy atoms, C = %d centres; %d launches per figure, %d "
    "alternating rounds" % (G, n, m, C, args.reps, args.rounds))
base = rng.normal(size=(n, 3)) * 1.5
gen_np = (base[None] + 0.25 * rng.normal(size=(G, n, 3))).astype(np.float32)
gen_np[1::2] = -gen_np[1::2]                     # every other conformer the mirror image, as the sampler leaves them
ref = torch.from_numpy((base[None] + 0.25 * rng.normal(size=(G, n, 3))).astype(np.float32)).to(dev)
gen = torch.from_numpy(gen_np).to(dev)
idx = torch.arange(m, dtype=torch.int32, device=dev)
st = _lib.stream_ptr()
for P in args.perms:
    perms = torch.from_numpy(group_of(P, m)).to(dev)
    scratch = torch.empty(2 * G * (3 * m + 1), dtype=torch.float32, device=dev)
    proper, mirror = (torch.empty((G, G), dtype=torch.float32, device=dev) for _ in range(2))
    outs = [torch.empty((G, G), dtype=torch.float32, device=dev) for _ in libs]

    def run_hands():
        _lib.check(lib.agdiff_rmsd_matrix_hands(_lib.ptr(ref), _lib.ptr(gen), _lib.ptr(idx), _lib.ptr(perms), G, G, n, m, P,
                                                _lib.ptr(scratch), _lib.ptr(proper), _lib.ptr(mirror), st), "agdiff_rmsd_matrix_hands")

    def run_one(k):
        _lib.check(libs[k][1].agdiff_rmsd_matrix(_lib.ptr(ref), _lib.ptr(gen), _lib.ptr(idx), _lib.ptr(perms), G, G, n, m, P,
                                                 _lib.ptr(scratch), _lib.ptr(outs[k]), st), "agdiff_rmsd_matrix")
    calls = [("agdiff_rmsd_matrix_hands (proper + mirror)", run_hands)] + [("agdiff_rmsd_matrix, %s" % name, (lambda k=k: run_one(k)))
                                                                            for k, (name, _) in enumerate(libs)]
    for _, fn in calls:                     # warm-up: code objects
        fn(); fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in calls}
    for _ in range(args.rounds):
        for name, fn in calls:
            ms[name].append(timed(fn, args.reps))
    for k in range(len(libs)):              # same inputs, same answers
        say("P = %d: proper bit-identical to agdiff_rmsd_matrix (%s): %s; mirror < proper for %.1f %% of the pairs"
            % (P, libs[k][0], bool(torch.equal(proper, outs[k])), 100.0 * float((mirror < proper).float().mean())))
    ref_name = "agdiff_rmsd_matrix, %s" % libs[-1][0]
    for name, _ in calls:
        v = np.array(ms[name])
        say("P = %d: %-46s median %8.3f ms  min %8.3f  max %8.3f   (%.3f x %s)"
            % (P, name, np.median(v), v.min(), v.max(), np.median(v) / np.median(ms[ref_name]), libs[-1][0]))

# verdict and mirror: C quads over random atoms (the kernels read the quads only)
quads = torch.from_numpy(np.sort(rng.permutation(n)[:4 * C].reshape(C, 4), axis=1).astype(np.int32)).to(dev)
target = torch.ones(C, dtype=torch.int8, device=dev)
vol = torch.empty((G, C), dtype=torch.float32, device=dev)
verdict = torch.empty(G, dtype=torch.int32, device=dev)
work = gen.clone()


def run_verdict():
    _lib.check(lib.agdiff_chiral_verdict(_lib.ptr(work), _lib.ptr(quads), _lib.ptr(target), G, n, C, _lib.ptr(vol), _lib.ptr(verdict), st),
               "agdiff_chiral_verdict")


run_verdict()
flags = (torch.arange(G, device=dev) % 2).to(torch.int32).contiguous()       # every other conformer, as above


def run_mirror():
    _lib.check(lib.agdiff_mirror_conformers(_lib.ptr(work), _lib.ptr(flags), G, n, st), "agdiff_mirror_conformers")


for name, fn in (("agdiff_chiral_verdict (vol + verdict)", run_verdict), ("agdiff_mirror_conformers (%d of %d flagged)" % (int(flags.sum()), G), run_mirror)):
    fn(); fn()
    torch.cuda.synchronize()
    v = np.array([timed(fn, args.reps) for _ in range(args.rounds)])
    say("%-52s G = %d, n = %d, C = %d: median %.4f ms  min %.4f  max %.4f" % (name, G, n, C, np.median(v), v.min(), v.max()))
# the fix end to end as stereo.fix_handedness runs it (host: uploads of quads / targets, two launches, no synchronising read)
import time
from agdiff_amd import stereo
q_np, t_np = quads.cpu().numpy(), target.cpu().numpy()
walls = []
for k in range(args.rounds + 1):
    work.copy_(gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v_, _ = stereo.chiral_verdict(work, q_np, t_np, want_vol=False)
    stereo.mirror_conformers(work, v_ < 0)
    torch.cuda.synchronize()
    if k:                                   # (the first pass warms up)
        walls.append((time.perf_counter() - t0) * 1e3)
say("verdict + mirror through agdiff_amd.stereo, G = %d: wall median %.3f ms  min %.3f  max %.3f" % (G, np.median(walls), min(walls), max(walls)))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
