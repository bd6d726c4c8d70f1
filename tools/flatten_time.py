#!/usr/bin/env python3
"""Time of the flattening repair (agdiff_relax_planar), by tools/relax_time.py's method: device events around `--reps` launches after
a warm-up, `--rounds` rounds in this one process, the median; beside it, in the same run and on the same conformers, the distance
repair alone (agdiff_relax_bounds: what the planes cost per update is the comparison) and the wall time of the numpy restatement of
the rule (tests/flatten_ref.py, float64, one conformer at a time).

G = 1000 conformers of tools/relax_time.py's 44-atom and 180-atom synthetic molecules (a random tree of carbons with its order-3
exclusions and the covalent-radius bounds).  The tree has no double bonds, so the planar groups are the caller's own: every branching
atom with its parent and children, about one group per nine atoms.  The valid and flat conformers are one random-walk geometry,
repaired once by the kernel itself until it passes, plus 0.002 A of noise per coordinate; every tenth conformer is then broken by
hand as in relax_time.py (the far half of the atoms shifted by (1.0, 0.3, 0) A, or one atom pulled halfway to its parent, in turn),
and another tenth bent: the centre of one group lifted 0.6 A out of the group's plane.  A record, not a gate: nothing here was fixed
in advance.  GPU only.

    python tools/flatten_time.py [--out profiles/flatten_timing.txt]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import flatten_ref as FR
import relax_ref as RR
import validity_ref as VR
from agdiff_amd import _lib
from agdiff_amd.planarity import membership_csr, relax_planar
from agdiff_amd.validity import relax_tables

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


def branch_groups(n, bonds):
    """(grp_ptr, grp_idx): every atom with a parent and at least two children, with them (4 .. 8 atoms), the first n // 9 of them"""
    parent = {a: p for p, a, _ in bonds}
    children = {}
    for p, a, _ in bonds:
        children.setdefault(p, []).append(a)
    groups = [sorted([a, parent[a]] + children[a])[:8] for a in range(1, n) if len(children.get(a, [])) >= 2][:max(1, n // 9)]
    ptr = np.zeros(len(groups) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(g) for g in groups])
    return ptr, np.array([a for g in groups for a in g], dtype=np.int32)


def conformers(n, G):
    """(the eight tables, pos float32 [G, n, 3], which conformers were broken, which bent)"""
    rng = np.random.default_rng(2021 + n)
    mol, bonds = VR.random_chain(rng, n)
    tab = branch_groups(n, bonds) + RR.tables(mol)
    base = None
    for _ in range(20):                                # a geometry the kernel itself brings inside the bounds and onto the planes
        walk = torch.from_numpy(RR.walk(rng, 1, bonds, n, 1.3, 1.7)).to(dev)
        out, status, _, _, _ = relax_planar(walk, *tab, omega=1.5, max_iter=5000)
        if status.item() == 1:
            base = out.cpu().numpy()[0].astype(np.float64)
            break
    if base is None:
        raise SystemExit("no valid and flat %d-atom geometry found" % n)
    pos = base[None] + 0.002 * rng.normal(size=(G, n, 3))
    broken, bent = np.arange(G) % 10 == 9, np.arange(G) % 10 == 4
    parent = {a: p for p, a, _ in bonds}
    for k, g in enumerate(np.nonzero(broken)[0]):
        if k % 2 == 0:
            pos[g, n // 2:] += (1.0, 0.3, 0.0)
        else:
            a = 1 + int(rng.integers(n - 1))
            pos[g, a] = 0.5 * (pos[g, a] + pos[g, parent[a]])
    ptr, idx = tab[0], tab[1]
    for k, g in enumerate(np.nonzero(bent)[0]):
        mem = idx[ptr[k % (len(ptr) - 1)]:ptr[k % (len(ptr) - 1) + 1]]
        y = pos[g, mem] - pos[g, mem].mean(0)
        centre = mem[np.argmin((y * y).sum(1))]
        pos[g, centre] += 0.6 * np.linalg.svd(y)[2][2]
    return tab, RR.centred(pos), broken, bent


def measure(n, G, omega, max_iter):
    tab, pos_np, broken, bent = conformers(n, G)
    bd_ptr, bd_idx, bd_lo, bd_hi, rad, ex_ptr, ex_idx, K = relax_tables(n, *tab[2:])
    mb_ptr, mb_grp = membership_csr(n, tab[0], tab[1])
    P = tab[0].shape[0] - 1
    keep = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pos_np, bd_ptr, bd_idx, bd_lo, bd_hi, rad, ex_ptr, ex_idx, tab[0], tab[1],
                                                                        mb_ptr, mb_grp)]
    pos = keep[0]
    dist, groups = [_lib.ptr(t) for t in keep[:8]], [_lib.ptr(t) for t in keep[8:]]
    out = torch.empty_like(pos)
    status, iters = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(2))
    resid, moved = (torch.empty(G, dtype=torch.float32, device=dev) for _ in range(2))
    res = [_lib.ptr(t) for t in (out, status, iters, resid, moved)]
    st = _lib.stream_ptr()

    def planar():
        _lib.check(lib.agdiff_relax_planar(*dist, *groups, G, n, K, P, 0.6, 0.02, omega, max_iter, 0.25, 0.10, *res, st), "agdiff_relax_planar")

    def bounds():
        _lib.check(lib.agdiff_relax_bounds(*dist, G, n, K, 0.6, 0.02, omega, max_iter, *res, st), "agdiff_relax_bounds")
    say("G = %d conformers, n = %d atoms, K = %d bounded pairs, P = %d planar groups of %d .. %d atoms; omega %.1f, at most %d updates"
        % (G, n, K, P, np.diff(tab[0]).min(), np.diff(tab[0]).max(), omega, max_iter))
    figures = {}
    for name, run in (("agdiff_relax_bounds", bounds), ("agdiff_relax_planar", planar)):      # (planar last: its results are kept)
        run(); run()                                   # warm-up: code objects
        torch.cuda.synchronize()
        ms = np.array([timed(run, args.reps) for _ in range(args.rounds)])
        s, it = status.cpu().numpy(), iters.cpu().numpy()
        figures[name] = (np.median(ms), int(it.max()))
        say("  %-20s status 0 / 1 / 2 / 3: %s; updates of the repaired: median %d, most %d; moved at most %.3f A"
            % (name, np.bincount(s, minlength=4).tolist(), int(np.median(it[s == 1])) if (s == 1).any() else 0, int(it.max()),
               float(moved.max())))
        say("  %-20s median %9.4f ms  min %9.4f  max %9.4f   (%d launches per figure, %d rounds)"
            % (name, np.median(ms), ms.min(), ms.max(), args.reps, args.rounds))
    (tb, ib), (tp, ip) = figures["agdiff_relax_bounds"], figures["agdiff_relax_planar"]
    say("  %d conformers broken by hand, %d bent by hand; per update of the slowest conformer: %.2f us without planes, %.2f us with"
        % (int(broken.sum()), int(bent.sum()), 1e3 * tb / max(ib, 1), 1e3 * tp / max(ip, 1)))
    t0 = time.perf_counter()
    ref = FR.relax(pos_np, *tab, omega=omega, max_iter=max_iter, margins=False)
    wall = time.perf_counter() - t0
    say("  numpy restatement (float64, CPU) %9.1f ms wall, once; status and updates equal to the kernel's for %d of %d conformers"
        % (1e3 * wall, int(((ref["status"] == s) & (ref["iters"] == it)).sum()), G))


say("flattening repair kernel on %s; torch %s, HIP %s, ABI %d" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip,
                                                                 _lib.DEFINES["AGDIFF_ABI_VERSION"]))
measure(44, args.confs, 1.0, 200)
measure(180, args.confs, 1.0, 200)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
