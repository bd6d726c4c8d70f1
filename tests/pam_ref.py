"""The rule of agdiff_pam_build and agdiff_pam_swap (include/agdiff_hip.h) restated in numpy on the uint64 / int64 fixed-point image
of the SAME float32 matrix, so that every comparison with the kernels is exact.  Q, valid, the assignment and `same` are
kmedoids_ref's, the matrices maxmin_ref's.  Shared by tests/test_pam_ref_cpu.py (which anchors it on hand-worked cases, on brute
force and on the invariants of the rule) and tests/test_hip_pam.py (which holds the kernels to it).  Not a test module."""
import numpy as np

import kmedoids_ref as KR
from kmedoids_ref import F32, NAN, Q, SCALE, U64, lattice, same, valid  # noqa: F401
from maxmin_ref import line, maxmin, random_metric, small_values, with_inf  # noqa: F401

I64 = np.int64
INF = U64(0xFFFFFFFFFFFFFFFF)                                # ds with K = 1: min(ds, x) = x
ROWS = 512                                                   # candidates per block of the vectorised passes


def eligible_of(d, anchor):
    """bool [G]: j == anchor or valid(dist[anchor][j])"""
    e = valid(d[anchor])
    e[anchor] = True
    return e


def _bad(G, K):
    return (np.full(K, -1, np.int32), np.full(G, -1, np.int32), np.full(G, NAN, F32), np.zeros(K, np.int32), np.zeros(K, np.float64),
            np.float64(0), 0, 2)


def _finish(d, q, med, eligible, n_swaps, status):
    """kmedoids' outputs for the medoids `med`"""
    K = len(med)
    labels, near = KR._assign(d, q, med, eligible)
    qn = np.where(eligible, Q(near), U64(0))
    size = np.bincount(labels[eligible], minlength=K).astype(np.int32)
    sums = np.array([qn[labels == r].sum(dtype=U64) for r in range(K)], dtype=U64)
    return (med.astype(np.int32), labels, near, size, sums.astype(np.float64) / SCALE, np.float64(int(sums.sum(dtype=U64))) / SCALE,
            n_swaps, status)


def total_cost(q, med, eligible):
    """the total cost (an int, in units of 2^-28) of the medoid set `med`: every eligible o at the smallest Q(dist[m][o]) over the
    medoids m, a medoid at 0"""
    med = np.asarray(med, dtype=np.int64)
    rows = q[med].copy()
    rows[np.arange(len(med)), med] = 0
    return int(rows.min(0)[eligible].sum(dtype=U64))


def state(q, med, eligible):
    """(n int64 [G], dn uint64 [G], ds uint64 [G]) of the medoid set, meaningful at the eligible o: the nearest medoid's rank (ties
    to the lowest; a medoid its own), its Q, and the smallest Q over the other ranks (INF with K = 1)"""
    K, G = len(med), q.shape[0]
    rows = q[med]                                            # [K, G]
    keys = rows + U64(1)                                     # a medoid's own column sorts before any Q, a zero included
    keys[np.arange(K), med] = 0
    n = np.argmin(keys, axis=0)                              # (the first, i.e. lowest, rank of the minimum)
    dn = rows[n, np.arange(G)]
    dn[med] = 0
    if K == 1:
        return n, dn, np.full(G, INF, dtype=U64)
    rest = rows.copy()
    rest[n, np.arange(G)] = INF
    return n, dn, rest.min(0)


def build(dist, K, anchor=0, q=None, picks=None, order=None):
    """agdiff_pam_build: kmedoids' tuple with n_swaps = 0 in n_iter's place, status 0 or 2.
      - rank 0: the eligible c with the smallest sum over the eligible o != c of Q(dist[c][o]), ties to the lowest index;
      - every further rank: the eligible non-medoid c with the largest gain(c) = dn(c) + the sum over the eligible non-medoids
        o != c of max(dn(o) - Q(dist[c][o]), 0), ties to the lowest index (a gain of 0 still picks);
      - after each pick dn(o) = min(dn(o), Q(dist[c][o])).
    `picks`, a list, receives (c, gain or sum) of every rank.  `order`: the medoids of a run with a larger K on the same matrix
    and anchor -- the walk is greedy, so its first K are this run's medoids and nothing is searched."""
    d = np.asarray(dist, dtype=F32)
    G = d.shape[0]
    assert d.shape == (G, G) and 1 <= K <= G
    if not 0 <= anchor < G:
        return _bad(G, K)
    eligible = eligible_of(d, anchor)
    if K > int(eligible.sum()):
        return _bad(G, K)
    if q is None:
        q = Q(d)
    if order is not None:
        return _finish(d, q, np.asarray(order[:K], dtype=np.int64), eligible, 0, 0)
    el = np.flatnonzero(eligible)
    is_med = np.zeros(G, dtype=bool)
    dn = np.zeros(G, dtype=U64)
    med = []
    for p in range(K):
        cands = np.flatnonzero(eligible & ~is_med)
        cols = el if p == 0 else el[dn[el] > 0]                        # (a column at dn = 0, a medoid's among them, adds nothing)
        score = np.empty(len(cands), dtype=I64)
        for a in range(0, len(cands), ROWS):
            c = cands[a:a + ROWS]
            x = q[np.ix_(c, cols)]
            at = np.minimum(np.searchsorted(cols, c), max(len(cols) - 1, 0))
            own = np.flatnonzero(cols[at] == c) if len(cols) else np.zeros(0, dtype=np.int64)
            x[own, at[own]] = 0                                        # (the diagonal is never read: x(c) = 0)
            if p == 0:
                score[a:a + ROWS] = -x.sum(axis=1, dtype=U64).astype(I64)
            else:                                                      # (c's own term is dn(c) - 0)
                score[a:a + ROWS] = (dn[cols][None, :] - np.minimum(dn[cols][None, :], x)).sum(axis=1, dtype=U64).astype(I64)
        best = int(np.argmax(score))                                   # (the first, i.e. lowest, index of the maximum)
        c = int(cands[best])
        if picks is not None:
            picks.append((c, int(abs(score[best]))))
        row = q[c].copy()
        row[c] = 0
        dn = row if p == 0 else np.minimum(dn, row)
        is_med[c] = True
        med.append(c)
    return _finish(d, q, np.asarray(med, dtype=np.int64), eligible, 0, 0)


def deltas(q, med, eligible):
    """(cands int64 [C], delta int64 [C, K]) of one SWAP iteration: for every candidate c (eligible, not a medoid), with
    x(o) = Q(dist[c][o]) and x(c) = 0,
        gain(c)     = the sum over all eligible o of dn(o) - min(dn(o), x(o))
        corr(c, r)  = the sum over the o with n(o) == r of min(ds(o), x(o)) - min(dn(o), x(o))
        delta(c, r) = corr(c, r) - gain(c)"""
    K = len(med)
    n, dn, ds = state(q, med, eligible)
    el = np.flatnonzero(eligible)
    order = el[np.argsort(n[el], kind="stable")]             # the eligible columns, rank by rank (every rank holds its medoid)
    starts = np.searchsorted(n[order], np.arange(K))
    is_med = np.zeros(q.shape[0], dtype=bool)
    is_med[med] = True
    cands = np.flatnonzero(eligible & ~is_med)
    delta = np.empty((len(cands), K), dtype=I64)
    pos = np.empty(q.shape[0], dtype=np.int64)
    pos[order] = np.arange(len(order))
    dno, dso = dn[order][None, :], ds[order][None, :]
    for a in range(0, len(cands), ROWS):
        c = cands[a:a + ROWS]
        x = q[np.ix_(c, order)]
        x[np.arange(len(c)), pos[c]] = 0
        m1 = np.minimum(dno, x)
        gain = (dno - m1).sum(axis=1, dtype=U64).astype(I64)
        np.minimum(dso, x, out=x)
        x -= m1
        corr = np.add.reduceat(x, starts, axis=1, dtype=U64).astype(I64)
        delta[a:a + ROWS] = corr - gain[:, None]
    return cands, delta


def swap(dist, init, anchor=None, max_swaps=64, trace=None, q=None):
    """agdiff_pam_swap: kmedoids' tuple with n_swaps in n_iter's place, from the seeds init [K] (anchor None: init[0]).
      - a seed or the anchor outside [0, G), a duplicate seed, a seed that is not eligible under the anchor: status 2;
      - an iteration takes the smallest delta(c, r), ties to the lowest candidate index, then to the lowest rank; if it is < 0,
        medoids[r] = c and n_swaps += 1; otherwise status 0; no candidate: status 0;
      - after max_swaps swaps, nothing looked for any more: status 1.
    `trace`, a list, receives the total cost (an int, in units of 2^-28) of the seeds and after every swap."""
    d = np.asarray(dist, dtype=F32)
    G = d.shape[0]
    init = np.asarray(init, dtype=np.int64).reshape(-1)
    K = len(init)
    assert d.shape == (G, G) and 1 <= K <= G and max_swaps >= 0
    if anchor is None:
        anchor = int(init[0])
    if not 0 <= anchor < G:
        return _bad(G, K)
    eligible = eligible_of(d, anchor)
    if ((init < 0) | (init >= G)).any() or len(set(init.tolist())) != K or not eligible[init].all():
        return _bad(G, K)
    if q is None:
        q = Q(d)
    med = init.copy()
    n_swaps, status = 0, 1
    if trace is not None:
        trace.append(total_cost(q, med, eligible))
    while n_swaps < max_swaps:
        cands, delta = deltas(q, med, eligible)
        if len(cands) == 0:
            status = 0
            break
        c, r = np.unravel_index(int(np.argmin(delta)), delta.shape)   # (row-major: the lowest candidate, then the lowest rank)
        if delta[c, r] >= 0:
            status = 0
            break
        med[r] = cands[c]
        n_swaps += 1
        if trace is not None:
            trace.append(total_cost(q, med, eligible))
    return _finish(d, q, med, eligible, n_swaps, status)


def check_invariants(d, anchor, res, trace=None, swapped=True):
    """what any run of BUILD (swapped=False: its status 0 says nothing about exchanges) or SWAP gives, from its outputs and the
    matrix alone"""
    med, labels, near, size, within, cost, n_swaps, status = res
    d = np.asarray(d, dtype=F32)
    K = len(med)
    assert status in (0, 1) and n_swaps >= 0
    q = Q(d)
    eligible = eligible_of(d, anchor)
    assert np.array_equal(labels >= 0, eligible) and np.isnan(near[~eligible]).all() and (labels < K).all()
    assert len(set(med.tolist())) == K and eligible[med].all()
    assert np.array_equal(labels[med], np.arange(K)) and (near[med] == 0).all()          # medoids own themselves
    rest = eligible.copy()
    rest[med] = False
    rows = q[med][:, rest]
    assert np.array_equal(labels[rest], rows.argmin(0))                                   # the LOWEST-rank nearest medoid
    assert np.array_equal(Q(near[rest]), rows.min(0))
    assert np.array_equal(size, np.bincount(labels[eligible], minlength=K)) and size.sum() == eligible.sum()
    total = int(Q(near[eligible]).sum(dtype=U64))
    assert total == total_cost(q, med, eligible) and cost == total / SCALE and within.sum() == cost
    if trace is not None:
        assert len(trace) == n_swaps + 1 and trace[-1] == total
        assert all(b < a for a, b in zip(trace, trace[1:]))                               # the total cost falls strictly
    if swapped and status == 0:
        cands, delta = deltas(q, med.astype(np.int64), eligible)
        assert len(cands) == 0 or delta.min() >= 0                                        # no exchange lowers the cost
