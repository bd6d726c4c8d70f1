"""A float64 numpy restatement of the distance-restraint sweep (csrc/eval.hip: agdiff_restrain_pairs; the rule of
include/agdiff_hip.h and DESIGN.md 4.18), and the cases the tests of it share.  It works from the PAIR LIST, not from the by-atom
table the kernel gathers: another route to the same sums.  It includes the fp32 rounding between sweeps and the d < 1e-12 rule.
Anchored by known answers in tests/test_restraints_ref_cpu.py.

The cases keep every restrained distance >= D_MIN, so that no direction (x_a - x_b) / d is ill-conditioned, and every coordinate
within X_MAX, where one fp32 rounding is <= 1.9e-6 Angstrom (assertions, not filters: no case is skipped)."""
import numpy as np

D_MIN = 0.1
X_MAX = 32.0
RESTRAINED = (0, 2, 2, 63, 64, 65, 129)      # restrained atoms per graph: none, the smallest legal case (one pair) twice -- the second
#                                              with its pair listed twice --, then across the 64-lane stride
EXTRA = (9, 11, 13, 17, 19, 23, 29)          # unrestrained atoms per graph
HUB_ENTRIES = 70
FAMILIES = ("mild", "strong", "satisfied")


def restrain_pairs(pos, pairs, lo, hi, batch, weight=1.0, sweeps=1, fixed=None, skip=None):
    """agdiff_restrain_pairs restated: (new pos float32 [N, 3], viol float64 [G], written bool [N]).  `pos` is taken as the fp32
    values the kernel reads; every sweep reads the positions as they were before it (Jacobi), computes in float64 and rounds to fp32
    once.  viol: the largest |e| of each graph before the first sweep, 0 without restraints, NaN for a graph with skip != 0 or with
    a restrained coordinate that is not finite -- such a graph is not written.  written: the atoms that have a row in a graph that
    was not left alone (what copy_out receives when sweeps >= 1)."""
    x = np.asarray(pos, dtype=np.float32).copy()
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    lo = np.asarray(lo, dtype=np.float32).astype(np.float64).reshape(-1)
    hi = np.asarray(hi, dtype=np.float32).astype(np.float64).reshape(-1)
    batch = np.asarray(batch).reshape(-1)
    N, G = x.shape[0], int(batch[-1]) + 1
    w = float(np.float32(weight))
    assert 0.0 < w <= 1.0 and 0 <= int(sweeps) <= 16 and pr.shape[0] == lo.shape[0] == hi.shape[0]
    fx = np.zeros(N, dtype=bool) if fixed is None else np.asarray(fixed).reshape(-1) != 0
    a, b = pr[:, 0], pr[:, 1]
    count = np.bincount(np.concatenate([a, b]), minlength=N).astype(np.float64)      # c_a: the static row length
    pair_graph = batch[a]
    assert (batch[b] == pair_graph).all() and (a != b).all()

    def errors(x64):
        diff = x64[a] - x64[b]
        d = np.sqrt((diff * diff).sum(axis=1))
        with np.errstate(invalid="ignore"):
            e = np.where(d > hi, d - hi, np.where(d < lo, d - lo, 0.0))
        return diff, d, e

    x64 = x.astype(np.float64)
    _, d, e = errors(x64)
    viol, alive = np.zeros(G), np.ones(G, dtype=bool)
    for g in range(G):
        rows = pair_graph == g
        atoms = np.unique(pr[rows].reshape(-1))
        if skip is not None and np.asarray(skip)[g] != 0:
            viol[g], alive[g] = np.nan, False
        elif not np.isfinite(x64[atoms]).all() or not np.isfinite(d[rows]).all():
            viol[g], alive[g] = np.nan, False
        elif rows.any():
            viol[g] = np.abs(e[rows]).max()
    written = (count > 0) & alive[batch]
    live = alive[pair_graph]
    for _ in range(int(sweeps)):
        x64 = x.astype(np.float64)
        diff, d, e = errors(x64)
        act = live & np.isfinite(d) & (d >= 1e-12) & (e != 0.0)
        share_a = np.where(fx[a], 0.0, np.where(fx[b], 1.0, 0.5))
        share_b = np.where(fx[b], 0.0, np.where(fx[a], 1.0, 0.5))
        total, touched = np.zeros((N, 3)), np.zeros(N, dtype=bool)
        for k in np.nonzero(act)[0]:                    # in the order of the pair list: the order of each atom's row
            u = diff[k] / d[k]
            if share_a[k] != 0.0:
                total[a[k]] += share_a[k] * (-e[k]) * u
                touched[a[k]] = True
            if share_b[k] != 0.0:
                total[b[k]] -= share_b[k] * (-e[k]) * u
                touched[b[k]] = True
        idx = np.nonzero(touched)[0]
        x[idx] = (x64[idx] + (w / count[idx])[:, None] * total[idx]).astype(np.float32)
    return x, viol, written


def distances(pos, pairs):
    p = np.asarray(pos, dtype=np.float64)
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return np.linalg.norm(p[pr[:, 0]] - p[pr[:, 1]], axis=1)


def violations(pos, pairs, lo, hi):
    """|e| of every pair of the list, float64."""
    d = distances(pos, pairs)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return np.where(d > hi, d - hi, np.where(d < lo, lo - d, 0.0))


# window kinds, as factors of the pair's present distance: (lo, hi), and whether the pair is violated
_KINDS = {
    "inside": lambda s: (1.0 - 0.4 * s, 1.0 + 0.4 * s),
    "inside, lower only": lambda s: (1.0 - 0.5 * s, np.inf),
    "inside, upper only": lambda s: (0.0, 1.0 + 0.5 * s),
    "above": lambda s: (1.0 - 1.4 * s, 1.0 - 0.8 * s),                # d > hi
    "above, upper only": lambda s: (0.0, 1.0 - 0.6 * s),
    "below": lambda s: (1.0 + 0.8 * s, 1.0 + 1.4 * s),                # d < lo
    "below, lower only": lambda s: (1.0 + 0.6 * s, np.inf),
}
_VIOLATED = ("above", "above, upper only", "below", "below, lower only")
_SATISFIED = ("inside", "inside, lower only", "inside, upper only")


def case(family, seed=0):
    """One packed batch of 7 graphs with RESTRAINED[g] restrained and EXTRA[g] unrestrained atoms at irregular places: uniform
    positions in a 16 Angstrom box per graph; every restrained atom in a chain of pairs; in the last graph a hub with HUB_ENTRIES row
    entries; in graph 2 the one pair listed twice.  Windows are set from each pair's present distance and cycle through the kinds
    above ("satisfied": the satisfied kinds only; "mild" / "strong": strength 0.25 / 0.5, with graph 1 kept satisfied).  `fixed`: a
    mask over about a third of the atoms for the runs with fixed ends.  fp32 arrays; asserts D_MIN and X_MAX."""
    strength = {"mild": 0.25, "strong": 0.5, "satisfied": 0.5}[family]
    rng = np.random.default_rng(500 + seed)
    batch, pos, pairs, kinds, hub = [], [], [], [], None
    off = 0
    for g, (m, extra) in enumerate(zip(RESTRAINED, EXTRA)):
        n = m + extra
        batch.extend([g] * n)
        pos.append(rng.uniform(-8.0, 8.0, size=(n, 3)) + rng.uniform(-4.0, 4.0, size=3))
        chosen = off + rng.permutation(n)[:m]                         # the restrained atoms, in no order
        if m == 2:
            reps = 2 if g == 2 else 1
            pairs.extend([(int(chosen[0]), int(chosen[1]))] * reps)
        elif m > 2:
            first = 0
            if m > HUB_ENTRIES + 1:                                   # the hub: chosen[0] with the next HUB_ENTRIES atoms
                hub = int(chosen[0])
                pairs.extend((hub, int(c)) if k % 2 else (int(c), hub) for k, c in enumerate(chosen[1:HUB_ENTRIES + 1]))
                first = 1
            pairs.extend((int(chosen[k]), int(chosen[k + 1])) for k in range(first, m - 1))
        off += n
    batch, pos = np.asarray(batch, dtype=np.int64), np.concatenate(pos).astype(np.float32)
    pairs = np.asarray(pairs, dtype=np.int32)
    d0 = distances(pos, pairs)
    lo, hi = np.zeros(len(pairs), dtype=np.float32), np.zeros(len(pairs), dtype=np.float32)
    cycle = _SATISFIED if family == "satisfied" else (_VIOLATED[0], _SATISFIED[0], _VIOLATED[2], _SATISFIED[1], _VIOLATED[1], _SATISFIED[2],
                                                      _VIOLATED[3])
    for k in range(len(pairs)):
        g = batch[pairs[k, 0]]
        kind = _SATISFIED[k % 3] if g == 1 else ("below" if g == 2 and family != "satisfied" else cycle[k % len(cycle)])
        f_lo, f_hi = _KINDS[kind](strength)
        lo[k], hi[k] = np.float32(max(f_lo, 0.0) * d0[k]), np.float32(f_hi * d0[k])
        kinds.append(kind)
    N = pos.shape[0]
    fixed = rng.random(N) < 0.33
    fixed[hub] = False                                                # (the hub moves in every family)
    c = dict(family=family, pos=pos, batch=batch, pairs=pairs, lo=lo, hi=hi, kinds=kinds, fixed=fixed, hub=hub, N=N, G=len(RESTRAINED))
    rows = np.bincount(pairs.reshape(-1), minlength=N)
    c["rows"] = rows
    assert [int((rows[batch == g] > 0).sum()) for g in range(c["G"])] == list(RESTRAINED)
    assert rows[hub] == HUB_ENTRIES and int((rows == 0).sum()) > 100
    assert d0.min() >= D_MIN and np.abs(pos).max() <= X_MAX and (lo <= hi).all() and (lo >= 0).all()
    return c
