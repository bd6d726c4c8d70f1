#!/usr/bin/env python3
"""Times of the ring kernels (agdiff_ring_coords, agdiff_tfd_matrix_terms) beside the two calls they stand next to
(agdiff_torsion_angles, agdiff_tfd_matrix) on the same conformers, by DESIGN.md 4.7's method: device events around `--reps` launches
of one entry point, the entry points taken in turn within a round (so that clock and cache state are shared), `--rounds` rounds after
one warm-up round, the median; and one call alone between two events on an idle stream, where the launch latency is not hidden
behind the call before.  agdiff_ring_coords reads the ring sizes back before it launches (one stream synchronisation per call), so
both of its figures are a call's time as a caller sees it, the read-back included, not the kernel's alone.  Beside them the wall
time of the numpy restatement (tests/rings_ref.py, float64) on a CPU, once.

G = 1000 conformers of a 44-atom synthetic molecule with 3 rings (6, 6, 5 atoms; 12 dihedral columns) and of a 180-atom one with 8
(6, 6, 6, 6, 5, 5, 6, 7; 50 columns).  The TFD matrices are the G x G self matrices over T = Q / 2 bonds (+ the rings for the terms
kernel, and the plain kernel at the same term count), 2 symmetry mappings.  A record, not a gate.  GPU only.

    python tools/rings_time.py [--out profiles/rings_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import rings_ref as RR
from agdiff_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--confs", type=int, default=1000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lib = _lib.load()
dev = torch.device("cuda", 0)
lines = []
SHAPES = [(44, [6, 6, 5], 12), (180, [6, 6, 6, 6, 5, 5, 6, 7], 50)]


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def measure(n, sizes, Q):
    rng = np.random.default_rng(2021 + n)
    G, Rg, T = args.confs, len(sizes), Q // 2
    pos_np = (rng.normal(size=(G, n, 3)) * 1.5).astype(np.float32)
    ptr = np.cumsum([0] + sizes).astype(np.int32)
    idx = np.concatenate([rng.permutation(n)[:N] for N in sizes]).astype(np.int32)
    quads_np = np.stack([rng.permutation(n)[:4] for _ in range(Q)]).astype(np.int32)
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pos, t_ptr, t_idx, quads = D(pos_np), D(ptr), D(idx), D(quads_np)
    tau, amp = (torch.empty((G, Rg), dtype=torch.float32, device=dev) for _ in range(2))
    pucker = torch.empty((G, int(ptr[-1]) - 3 * Rg), dtype=torch.float32, device=dev)
    ang = torch.empty((G, Q), dtype=torch.float32, device=dev)
    val = torch.empty((G, Q + Rg), dtype=torch.float32, device=dev)
    tmap_t = np.stack([np.arange(0, 2 * T, 2), np.arange(1, 2 * T, 2)]).astype(np.int32)                   # the plain kernel at T terms
    ring_cols = Q + np.arange(Rg)
    tmap_r = np.concatenate([tmap_t, np.stack([ring_cols, ring_cols[::-1]])], axis=1).astype(np.int32)      # T bonds + Rg rings
    scale = np.concatenate([np.full(T, np.pi), [RR.ring_scale(N) for N in sizes]]).astype(np.float32)
    even = np.concatenate([np.zeros(T), np.ones(Rg)]).astype(np.int32)
    d_tt, d_tr, d_sc, d_ev = D(tmap_t), D(tmap_r), D(scale), D(even)
    d_tt_wide = D(np.concatenate([tmap_t, tmap_t[:, :Rg]], axis=1).astype(np.int32))                        # the plain kernel at T + Rg terms
    out = torch.empty((G, G), dtype=torch.float32, device=dev)
    st = _lib.stream_ptr()
    P = _lib.ptr
    calls = {
        "agdiff_ring_coords, tau + amp + pucker": lambda: lib.agdiff_ring_coords(P(pos), P(t_ptr), P(t_idx), G, n, Rg, P(tau), P(amp), P(pucker), st),
        "agdiff_ring_coords, tau alone         ": lambda: lib.agdiff_ring_coords(P(pos), P(t_ptr), P(t_idx), G, n, Rg, P(tau), P(None), P(None), st),
        "agdiff_torsion_angles, Q columns      ": lambda: lib.agdiff_torsion_angles(P(pos), P(quads), G, n, Q, P(ang), st),
        "agdiff_tfd_matrix, T terms            ": lambda: lib.agdiff_tfd_matrix(P(ang), P(ang), P(d_tt), P(None), G, G, Q, T, 2, 0.0, P(out), P(None), P(None), st),
        "agdiff_tfd_matrix, T + Rg terms       ": lambda: lib.agdiff_tfd_matrix(P(val), P(val), P(d_tt_wide), P(None), G, G, Q + Rg, T + Rg, 2, 0.0, P(out), P(None),
                                                                                P(None), st),
        "agdiff_tfd_matrix_terms, T + Rg terms ": lambda: lib.agdiff_tfd_matrix_terms(P(val), P(val), P(d_tr), P(None), P(d_sc), P(d_ev), G, G, Q + Rg, T + Rg, 2,
                                                                                      0.0, P(out), P(None), P(None), st),
    }
    say("G = %d conformers, n = %d atoms, Rg = %d rings of %s atoms, Q = %d dihedral columns, T = %d bonds"
        % (G, n, Rg, "/".join(map(str, sizes)), Q, T))
    for fn in calls.values():
        assert fn() == 0
    val[:, :Q], val[:, Q:] = ang, tau
    figures = {name: [] for name in calls}
    single = {name: [] for name in calls}
    for rnd in range(args.rounds + 1):
        for name, fn in calls.items():                 # in turn within a round
            us, one = timed(fn, args.reps), timed(fn, 1)
            if rnd:                                    # (round 0 warms up: code objects, clocks)
                figures[name].append(us)
                single[name].append(one)
    for name in calls:
        us, one = np.array(figures[name]), np.array(single[name])
        say("  %s  median %8.2f us per call over %d back to back  (min %8.2f, max %8.2f);  one call alone %8.2f us   (%d rounds)"
            % (name, np.median(us), args.reps, us.min(), us.max(), np.median(one), args.rounds))
    t0 = time.perf_counter()
    want = RR.ring_coords(pos_np, ptr, idx)
    wall = time.perf_counter() - t0
    ok = np.abs(tau.cpu().numpy() - want[0]).max() <= 1e-6 and np.abs(amp.cpu().numpy() - want[1]).max() <= 1e-6
    say("  numpy restatement of agdiff_ring_coords (float64, CPU) %9.1f ms wall, once; tau and amplitudes within 1e-6 of the kernel's: %s" % (1e3 * wall, ok))
    sub = slice(0, 200)
    t0 = time.perf_counter()
    v = val.cpu().numpy()
    RR.tfd_terms(v[sub], v[sub], tmap_r, scale, even)
    wall = time.perf_counter() - t0
    say("  numpy restatement of agdiff_tfd_matrix_terms (float64, CPU), 200 x 200 of the %d x %d pairs %9.1f ms wall, once" % (G, G, 1e3 * wall))


say("ring kernels on %s; torch %s, HIP %s, ABI %d" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip,
                                                      _lib.DEFINES["AGDIFF_ABI_VERSION"]))
for n, sizes, Q in SHAPES:
    measure(n, sizes, Q)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
