#!/usr/bin/env python3
"""Times of agdiff_flip_double_bonds, by tools/stereo_timing.py's method: device events around `--reps` launches after a warm-up,
`--rounds` rounds, medians.  Two molecules, chains laid out as tests/ez_cases.py lays them out: 44 atoms with 2 tagged double bonds
and 180 atoms with 6, `--G` conformers each, half of the conformers with one bond turned over.  A flip changes its input, so every
timed launch follows a device copy of the pristine conformers into the work buffer; the copy alone is timed too and subtracted.
The same grid with `target` all zero is the floor (every bond judged, none flipped), and the float64 numpy restatement
(tests/ez_ref.py) of the same call on the CPU is the yardstick.

    python tools/ezbonds_timing.py [--out profiles/ezbonds_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import ez_cases as EC
import ez_ref as ER
from agdiff_amd import _lib, ezbonds

ap = argparse.ArgumentParser()
ap.add_argument("--G", type=int, default=1000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--cpu-confs", type=int, default=100, help="conformers the numpy restatement is timed on (scaled to --G)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
lib = _lib.load()
dev = torch.device("cuda", 0)
G = args.G
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


say("agdiff_flip_double_bonds: G = %d conformers, every other one with one tagged bond turned over; %d launches per figure, %d rounds, "
    "medians; each launch after a device copy of the input, whose own time is subtracted" % (G, args.reps, args.rounds))
st = _lib.stream_ptr()
for n, doubles in ((44, (10, 30)), (180, (20, 50, 78, 106, 134, 162))):
    mol, skeleton = EC.chain(n, set(doubles))
    quads, in_ring = ezbonds.stereo_double_bonds(*mol)
    D = quads.shape[0]
    assert D == len(doubles) and not in_ring.any()
    target = ER.states(skeleton[None], quads, np.ones(D, dtype=np.int8))[0]
    side_ptr, side_idx = ezbonds.flip_sides(n, mol[1], mol[2], quads)
    rng = np.random.default_rng(2021 + n)
    pos = np.empty((G, n, 3), dtype=np.float32)
    for g in range(G):
        p = skeleton.copy()
        if g % 2:
            c = int(rng.integers(D))
            ER.rotate_side(p, int(quads[c, 1]), int(quads[c, 2]), side_idx[side_ptr[c]:side_ptr[c + 1]])
        pos[g] = (p + rng.uniform(-0.1, 0.1, size=p.shape)) @ EC.random_rotation(rng).T
    gen = torch.from_numpy(pos).to(dev)
    work = gen.clone()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    q_d, sp_d, si_d = up(quads), up(side_ptr), up(side_idx)
    t_d, zero_d = up(target), torch.zeros(D, dtype=torch.int8, device=dev)
    state = torch.empty((G, D), dtype=torch.int8, device=dev)
    flipped = torch.empty(G, dtype=torch.int32, device=dev)

    def launch(tgt):
        work.copy_(gen)
        _lib.check(lib.agdiff_flip_double_bonds(_lib.ptr(work), _lib.ptr(q_d), _lib.ptr(tgt), _lib.ptr(sp_d), _lib.ptr(si_d), G, n, D,
                                                _lib.ptr(state), _lib.ptr(flipped), st), "agdiff_flip_double_bonds")
    calls = [("copy alone", lambda: work.copy_(gen)), ("copy + flip, half of the conformers wrong", lambda: launch(t_d)),
             ("copy + flip, target all zero (the floor)", lambda: launch(zero_d))]
    for _, fn in calls:
        fn(); fn()
    torch.cuda.synchronize()
    launch(t_d)
    torch.cuda.synchronize()
    want = ER.states(pos[:8], quads, target)
    assert np.array_equal(state[:8].cpu().numpy(), want) and int(flipped.sum()) == G // 2
    ms = {name: [] for name, _ in calls}
    for _ in range(args.rounds):
        for name, fn in calls:
            ms[name].append(timed(fn, args.reps))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    for name, _ in calls:
        v = np.array(ms[name])
        say("n = %3d, D = %d: %-44s median %.4f ms  min %.4f  max %.4f" % (n, D, name, np.median(v), v.min(), v.max()))
    say("n = %3d, D = %d: the launch alone: %.4f ms with half of the conformers wrong, %.4f ms at the floor"
        % (n, D, med[calls[1][0]] - med[calls[0][0]], med[calls[2][0]] - med[calls[0][0]]))
    k = min(args.cpu_confs, G)
    t0 = time.perf_counter()
    ER.flip(pos[:k], quads, target, side_ptr, side_idx)
    cpu = (time.perf_counter() - t0) * 1e3
    say("n = %3d, D = %d: the float64 numpy restatement on the CPU: %.1f ms for %d conformers, %.0f ms scaled to %d" % (n, D, cpu, k, cpu * G / k, G))
    walls = []
    for r in range(args.rounds + 1):
        work.copy_(gen)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ezbonds.flip_double_bonds(work, quads, target, side_ptr, side_idx)
        torch.cuda.synchronize()
        if r:
            walls.append((time.perf_counter() - t0) * 1e3)
    say("n = %3d, D = %d: through agdiff_amd.ezbonds.flip_double_bonds (host checks, five uploads, one launch): wall median %.3f ms  min %.3f  max %.3f"
        % (n, D, np.median(walls), min(walls), max(walls)))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
