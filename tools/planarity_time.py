#!/usr/bin/env python3
"""Time of the planarity kernel (agdiff_planar_groups), by tools/relax_time.py's method: device events around `--reps` launches after
a warm-up of a fifth as many, `--rounds` rounds in this one process, the median (a launch takes microseconds, so a figure needs thousands
of them to be a window of a tenth of a second); beside it the wall time of the numpy restatement of the definition
(tests/planarity_ref.py, float64, numpy.linalg.eigh per conformer and group) on the same conformers, and -- as the floor a launch of
this shape has -- agdiff_pair_bounds over as many pairs as there are groups (one wave per conformer too, a square root per lane).

G = 1000 conformers of a 44-atom synthetic molecule with 5 planar groups and of a 180-atom one with 20 (tests/planarity_ref.py's
random groups of 3 .. 8 atoms: a third random, a third nearly planar, a third planar; about one group per nine atoms, as an aromatic
ring or a double bond with its neighbours takes).  A record, not a gate: nothing here was fixed in advance.  GPU only.

    python tools/planarity_time.py [--shapes 44:5,180:20] [--out profiles/planarity_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import planarity_ref as PR
from agdiff_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5000)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--confs", type=int, default=1000)
ap.add_argument("--shapes", default="44:5,180:20", help="atoms:groups of the synthetic molecules")
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


def measure(n, G, P):
    pos_np, ptr, idx, _ = PR.random_case(n, G, P, 2021 + n)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pos, t_ptr, t_idx = T(pos_np), T(ptr), T(idx)
    table = torch.empty((G, P), dtype=torch.float32, device=dev)
    worst = torch.empty(G, dtype=torch.float32, device=dev)
    group, bent = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(2))
    pairs = T(np.stack([idx[ptr[:-1]], idx[ptr[:-1] + 1]], axis=1).astype(np.int32))
    lo, hi = torch.zeros(P, device=dev), torch.full((P,), 100.0, device=dev)
    st = _lib.stream_ptr()

    def planar(want_dev):
        return lambda: _lib.check(lib.agdiff_planar_groups(_lib.ptr(pos), _lib.ptr(t_ptr), _lib.ptr(t_idx), G, n, P, PR.THRESH,
                                                           _lib.ptr(table if want_dev else None), _lib.ptr(worst), _lib.ptr(group),
                                                           _lib.ptr(bent), st), "agdiff_planar_groups")

    def floor():
        _lib.check(lib.agdiff_pair_bounds(_lib.ptr(pos), _lib.ptr(pairs), _lib.ptr(lo), _lib.ptr(hi), G, n, P, None, _lib.ptr(worst),
                                          _lib.ptr(group), _lib.ptr(bent), st), "agdiff_pair_bounds")
    say("G = %d conformers, n = %d atoms, P = %d groups of %s atoms (%d members in all)"
        % (G, n, P, "/".join(map(str, sorted(set(np.diff(ptr).tolist())))), idx.shape[0]))
    for name, fn in (("agdiff_planar_groups, with dev ", planar(True)), ("agdiff_planar_groups, no dev   ", planar(False)),
                     ("agdiff_pair_bounds, K = P pairs", floor)):
        timed(fn, args.reps // 5)                      # warm-up: code objects, clocks
        us = 1e3 * np.array([timed(fn, args.reps) for _ in range(args.rounds)])
        say("  %s  median %8.2f us  min %8.2f  max %8.2f   (%d launches per figure, %d rounds)"
            % (name, np.median(us), us.min(), us.max(), args.reps, args.rounds))
    planar(True)()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = PR.planar(pos_np, ptr, idx, PR.THRESH)
    wall = time.perf_counter() - t0
    keep = ~PR.left_out(ref)
    same = PR.close(np.where(keep, table.cpu().numpy(), 0.0), np.where(keep, ref["dev"], 0.0))
    say("  numpy restatement (float64, CPU) %9.1f ms wall, once; dev within the tests' gate of the kernel's: %s; %d of %d conformers bent"
        % (1e3 * wall, same, int((ref["n_bent"] > 0).sum()), G))


say("planarity kernel on %s; torch %s, HIP %s, ABI %d" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip,
                                                           _lib.DEFINES["AGDIFF_ABI_VERSION"]))
for shape in args.shapes.split(","):
    n, P = map(int, shape.split(":"))
    measure(n, args.confs, P)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
