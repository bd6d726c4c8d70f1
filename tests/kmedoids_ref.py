"""The rule of agdiff_kmedoids (include/agdiff_hip.h) restated in numpy on the uint64 fixed-point image of the SAME float32 matrix,
so that every comparison with the kernels is exact: integers equal, floats and doubles bit-equal, NaN positions equal.  With it the
matrices of the structured cases.  Shared by tests/test_kmedoids_ref_cpu.py (which anchors it on hand-worked cases, on brute force
and on the invariants of the rule) and tests/test_hip_medoids.py (which holds the kernels to it).  Not a test module."""
import numpy as np

from maxmin_ref import line, maxmin, random_metric, small_values, with_inf  # noqa: F401  (the structured matrices are shared)

F32, U64 = np.float32, np.uint64
NAN = F32(np.nan)
CAP = F32(4096.0)                                            # AGDIFF_KMEDOIDS_MAX_DIST
SCALE = 2.0 ** 28
FAR = 1 << 40                                                # Q of an entry that is not valid


def valid(x):
    """x >= 0.0f && x <= 4096.0f: NaN, negative values, +-inf and anything above the cap are not valid; -0.0 is"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore"):
        return (x >= F32(0)) & (x <= CAP)


def Q(x):
    """uint64(rint((double)x * 2^28)), half to even, for a valid x (the product is exact in fp64); 2^40 otherwise"""
    x = np.asarray(x, dtype=F32)
    ok = valid(x)
    q = np.rint(np.where(ok, x, F32(0)).astype(np.float64) * SCALE).astype(U64)
    return np.where(ok, q, U64(FAR))


def lattice(nx, ny):
    """float32 [nx ny, nx ny]: the Manhattan distances of the integer points of an nx x ny lattice, x running slowest"""
    x, y = np.divmod(np.arange(nx * ny), ny)
    return (np.abs(x[:, None] - x[None, :]) + np.abs(y[:, None] - y[None, :])).astype(F32)


def _assign(d, q, med, eligible):
    """(labels int32 [G], near float32 [G]) of the medoids `med`"""
    K = len(med)
    labels = np.argmin(q[med], axis=0).astype(np.int32)      # (argmin returns the first, i.e. lowest, rank of the minimum)
    labels[med] = np.arange(K, dtype=np.int32)               # a medoid belongs to its own rank
    stored = d[med[labels], np.arange(d.shape[0])]
    near = np.where(stored == 0, F32(0), stored)             # (-0.0 is written as +0.0; a NaN stays)
    near[med] = 0
    labels[~eligible], near[~eligible] = -1, NAN
    return labels, near


def member_costs(q, labels, r):
    """(members int [n], cost uint64 [n]) of cluster r: cost_i = the sum of Q(dist[i][j]) over the members j != i, along row i"""
    idx = np.flatnonzero(labels == r)
    sub = q[np.ix_(idx, idx)]
    sub[np.arange(len(idx)), np.arange(len(idx))] = 0        # (the diagonal is never read)
    return idx, sub.sum(axis=1, dtype=U64)


def kmedoids(dist, init, max_iter=32, trace=None, q=None):
    """(medoids int32 [K], labels int32 [G], near float32 [G], size int32 [K], within float64 [K], cost float64, n_iter int,
    status int) of dist [G, G] from the seeds init [K], straight from the rule:
      - conformer j is eligible iff j == init[0] or valid(dist[init[0]][j]); an ineligible one takes no further part; among
        eligible conformers an entry that is not valid counts as 2^40;
      - a seed outside [0, G), a duplicate seed or an ineligible seed: status 2, medoids and labels -1, near NaN, the rest 0;
      - assign: a medoid belongs to its own rank with near 0; every other eligible j goes to the rank r with the smallest
        Q(dist[medoid_r][j]), ties to the lowest rank;
      - update: in every cluster the member with the smallest cost (member_costs), ties to the lowest index, becomes the medoid
        -- unless the incumbent's cost equals that minimum: then the incumbent stays;
      - assign and update repeat until an update changes nothing (status 0) or max_iter updates were made (status 1, and one
        more assign); n_iter counts the updates, the one that changed nothing included.
    `trace`, a list, receives the total cost (an int, in units of 2^-28) after every assign.  `q` may pass Q(dist) in."""
    d = np.asarray(dist, dtype=F32)
    G = d.shape[0]
    init = np.asarray(init, dtype=np.int64).reshape(-1)
    K = len(init)
    assert d.shape == (G, G) and 1 <= K <= G and max_iter >= 1
    bad = (np.full(K, -1, np.int32), np.full(G, -1, np.int32), np.full(G, NAN, F32), np.zeros(K, np.int32), np.zeros(K, np.float64),
           np.float64(0), 0, 2)
    if not 0 <= init[0] < G:
        return bad
    eligible = valid(d[init[0]])
    eligible[init[0]] = True
    if ((init < 0) | (init >= G)).any() or len(set(init.tolist())) != K or not eligible[init].all():
        return bad
    if q is None:
        q = Q(d)
    med = init.copy()
    n_iter, status = 0, 1
    labels, near = _assign(d, q, med, eligible)
    while True:
        if trace is not None:
            trace.append(int(Q(near[eligible]).sum(dtype=U64)))
        if n_iter == max_iter:
            break                                            # status 1: the assign above belongs to the returned medoids
        changed = False
        for r in range(K):
            idx, cost = member_costs(q, labels, r)
            best = int(np.argmin(cost))                      # (the first, i.e. lowest, index of the minimum)
            if cost[best] != cost[np.searchsorted(idx, med[r])]:
                med[r], changed = idx[best], True
        n_iter += 1
        if not changed:
            status = 0
            break
        labels, near = _assign(d, q, med, eligible)
    qn = np.where(eligible, Q(near), U64(0))
    size = np.bincount(labels[eligible], minlength=K).astype(np.int32)
    sums = np.array([qn[labels == r].sum(dtype=U64) for r in range(K)], dtype=U64)
    within = sums.astype(np.float64) / SCALE
    cost = np.float64(int(sums.sum(dtype=U64))) / SCALE
    return med.astype(np.int32), labels, near, size, within, cost, n_iter, status


def same(got, want):
    """True when two results are equal entry for entry: integers equal, float32 bit-equal and float64 bit-equal (NaN at the same
    places, +0 for +0)"""
    for a, b in zip(got, want):
        a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
        if a.shape != b.shape:
            return False
        if a.dtype == np.float64 or b.dtype == np.float64:
            if a.dtype != b.dtype or not np.array_equal(a.view(U64), b.view(U64)):
                return False
        elif a.dtype.kind == "f" or b.dtype.kind == "f":
            a, b = a.astype(F32), b.astype(F32)
            if not np.array_equal(np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32)),
                                  np.where(np.isnan(b), np.uint32(0x7fc00000), b.view(np.uint32))):
                return False
        elif not np.array_equal(a, b):
            return False
    return True


def check_invariants(d, init, res, trace=None):
    """what any run of the rule gives, from its outputs and the matrix alone"""
    med, labels, near, size, within, cost, n_iter, status = res
    d = np.asarray(d, dtype=F32)
    G, K = d.shape[0], len(med)
    assert status in (0, 1) and n_iter >= 1
    q = Q(d)
    eligible = valid(d[init[0]])
    eligible[init[0]] = True
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
    assert cost == total / SCALE and within.sum() == cost
    if trace is not None:
        assert len(trace) == n_iter + (status == 1) and trace[-1] == total
        assert all(b < a for a, b in zip(trace, trace[1:]))                               # the total cost falls strictly
    if status == 0:
        for r in range(K):
            idx, c = member_costs(q, labels, r)
            assert c.min() == c[np.searchsorted(idx, med[r])]                             # no member is cheaper than its medoid
