#!/usr/bin/env python3
"""Time of the geometry repair (agdiff_relax_bounds), by tools/validity_timing.py's method: device events around `--reps` launches
after a warm-up, `--rounds` rounds in this one process, the median; beside it the wall time of the numpy restatement of the rule
(tests/relax_ref.py, float64, one conformer at a time) on the same conformers.

G = 1000 conformers of a 44-atom and of a 180-atom synthetic molecule (a random tree of carbons with its order-3 exclusions and the
covalent-radius bounds, as the tests build them).  The valid conformers are one random-walk geometry, repaired once by the kernel
itself until it passes, plus 0.002 A of noise per coordinate; every tenth conformer is then broken by hand -- the far half of the
atoms shifted by (1.0, 0.3, 0) A, or one atom pulled halfway to its parent, in turn.  A record, not a gate: nothing here was fixed in
advance.  GPU only.

    python tools/relax_time.py [--out profiles/relax_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import relax_ref as RR
import validity_ref as VR
from agdiff_amd import _lib
from agdiff_amd.validity import relax_bounds, relax_tables

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--confs", type=int, default=1000)
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


def conformers(n, G):
    """(the six tables, pos float32 [G, n, 3], which conformers were broken)"""
    rng = np.random.default_rng(2021 + n)
    mol, bonds = VR.random_chain(rng, n)
    tab = RR.tables(mol)
    base = None
    for _ in range(20):                                # a geometry the kernel itself brings inside the bounds
        walk = torch.from_numpy(RR.walk(rng, 1, bonds, n, 1.3, 1.7)).to(dev)
        out, status, _, _, _ = relax_bounds(walk, *tab, omega=1.5, max_iter=5000)
        if status.item() == 1:
            base = out.cpu().numpy()[0].astype(np.float64)
            break
    if base is None:
        raise SystemExit("no valid %d-atom geometry found" % n)
    pos = base[None] + 0.002 * rng.normal(size=(G, n, 3))
    broken = np.arange(G) % 10 == 9
    parent = {a: p for p, a, _ in bonds}
    for k, g in enumerate(np.nonzero(broken)[0]):
        if k % 2 == 0:
            pos[g, n // 2:] += (1.0, 0.3, 0.0)
        else:
            a = 1 + int(rng.integers(n - 1))
            pos[g, a] = 0.5 * (pos[g, a] + pos[g, parent[a]])
    return tab, RR.centred(pos), broken


def measure(n, G, omega, max_iter):
    tab, pos_np, broken = conformers(n, G)
    bd_ptr, bd_idx, bd_lo, bd_hi, rad, ex_ptr, ex_idx, K = relax_tables(n, *tab)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pos, t_ptr, t_idx, t_lo, t_hi, t_rad, t_exp, t_exi = (T(a) for a in (pos_np, bd_ptr, bd_idx, bd_lo, bd_hi, rad, ex_ptr, ex_idx))
    out = torch.empty_like(pos)
    status, iters = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(2))
    resid, moved = (torch.empty(G, dtype=torch.float32, device=dev) for _ in range(2))
    st = _lib.stream_ptr()

    def run():
        _lib.check(lib.agdiff_relax_bounds(_lib.ptr(pos), _lib.ptr(t_ptr), _lib.ptr(t_idx), _lib.ptr(t_lo), _lib.ptr(t_hi), _lib.ptr(t_rad),
                                           _lib.ptr(t_exp), _lib.ptr(t_exi), G, n, K, 0.6, 0.02, omega, max_iter, _lib.ptr(out),
                                           _lib.ptr(status), _lib.ptr(iters), _lib.ptr(resid), _lib.ptr(moved), st), "agdiff_relax_bounds")
    run(); run()                                       # warm-up: code objects
    torch.cuda.synchronize()
    ms = np.array([timed(run, args.reps) for _ in range(args.rounds)])
    s, it = status.cpu().numpy(), iters.cpu().numpy()
    say("G = %d conformers, n = %d atoms, K = %d bounded pairs, %d excluded pairs of %d; omega %.1f, at most %d updates"
        % (G, n, K, ex_idx.shape[0] // 2, n * (n - 1) // 2, omega, max_iter))
    say("  %d conformers broken by hand; status 0 / 1 / 2 / 3: %s; updates of the repaired: median %d, most %d; moved at most %.3f A"
        % (int(broken.sum()), np.bincount(s, minlength=4).tolist(), int(np.median(it[s == 1])) if (s == 1).any() else 0, int(it.max()),
           float(moved.max())))
    say("  agdiff_relax_bounds              median %9.4f ms  min %9.4f  max %9.4f   (%d launches per figure, %d rounds)"
        % (np.median(ms), ms.min(), ms.max(), args.reps, args.rounds))
    t0 = time.perf_counter()
    ref = RR.relax(pos_np, *tab, omega=omega, max_iter=max_iter, margins=False)
    wall = time.perf_counter() - t0
    say("  numpy restatement (float64, CPU) %9.1f ms wall, once; status and updates equal to the kernel's for %d of %d conformers"
        % (1e3 * wall, int(((ref["status"] == s) & (ref["iters"] == it)).sum()), G))


say("geometry repair kernel on %s; torch %s, HIP %s, ABI %d" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip,
                                                               _lib.DEFINES["AGDIFF_ABI_VERSION"]))
measure(44, args.confs, 1.0, 200)
measure(180, args.confs, 1.0, 200)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
