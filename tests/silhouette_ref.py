"""The rule of agdiff_silhouette (include/agdiff_hip.h) restated in numpy on the uint64 fixed-point image (kmedoids_ref.Q) of the
SAME float32 matrix, so that every comparison with the kernels is exact: integers equal, doubles bit-equal, NaN at the same places.
With it `textbook`, the plain float64 definition on the unquantised matrix.  Shared by tests/test_silhouette_ref_cpu.py (which
anchors the restatement on hand-worked cases, on the invariants of the rule and on `textbook`) and tests/test_hip_silhouette.py
(which holds the kernels to it).  Not a test module."""
import numpy as np

from kmedoids_ref import Q, kmedoids, lattice, line, maxmin, random_metric, same, small_values, with_inf  # noqa: F401  (shared with the tests)

F32, U64, F64 = np.float32, np.uint64, np.float64
SCALE = 2.0 ** 28
TSCALE = 2.0 ** 40


def _bad(G, K):
    nan = np.full(G, np.nan)
    return (nan, nan.copy(), nan.copy(), np.full(G, -1, np.int32), np.zeros(K, np.int32), np.full(K, np.nan), F64(np.nan), 2)


def silhouette(dist, labels, K, q=None):
    """(a float64 [G], b float64 [G], s float64 [G], other int32 [G], size int32 [K], cluster_mean float64 [K], mean float64,
    status int) of dist [G, G] under the clustering `labels` [G] (-1: left out; 0 .. K - 1: a member of that rank; anything else:
    status 2 and the fill), straight from the rule:
      - S_c(i) = the sum of Q(dist[i][j]) over the members j != i of rank c, along row i, as uint64;
      - ma = S_own / (size_own - 1) (0 for a singleton), m_c = S_c / size[c], one fp64 division each;
      - mb the smallest m_c over the non-empty ranks c != own, other that rank, ties to the lowest; none: other -1, b NaN;
      - s = 0 for a singleton, with no other non-empty rank or when max(ma, mb) == 0, else (mb - ma) / max(ma, mb);
      - a = ma / 2^28, b = mb / 2^28; a left-out conformer: a, b, s NaN and other -1;
      - T = rint(s 2^40) as int64; cluster_mean[c] = (sum of T over c / size[c]) / 2^40 (NaN when empty), mean the same over all.
    O(G^2): the member columns are sorted by rank and summed by np.add.reduceat along the rows.  `q` may pass Q(dist) in."""
    d = np.asarray(dist, dtype=F32)
    G = d.shape[0]
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    assert d.shape == (G, G) and labels.shape == (G,) and K >= 1
    if ((labels < -1) | (labels >= K)).any():
        return _bad(G, K)
    member = labels >= 0
    idx = np.flatnonzero(member)
    size = np.bincount(labels[idx], minlength=K).astype(np.int32)
    a, b, s = np.full(G, np.nan), np.full(G, np.nan), np.full(G, np.nan)
    other = np.full(G, -1, np.int32)
    cluster_mean = np.full(K, np.nan)
    if idx.size == 0:
        return a, b, s, other, size, cluster_mean, F64(np.nan), 0
    if q is None:
        q = Q(d)
    ranks = np.flatnonzero(size > 0)                         # the non-empty ranks, ascending
    order = idx[np.argsort(labels[idx], kind="stable")]      # the members, sorted by rank
    sub = q[np.ix_(idx, order)]                              # [members, members by rank]
    sub[order[None, :] == idx[:, None]] = 0                  # (the diagonal is never read)
    starts = np.concatenate([[0], np.cumsum(size[ranks])[:-1]])
    S = np.add.reduceat(sub, starts, axis=1)                 # uint64 [members, non-empty ranks]
    del sub
    own = np.searchsorted(ranks, labels[idx])                # each member's column of S
    rows = np.arange(idx.size)
    n_own = size[labels[idx]].astype(np.int64)
    ma = np.where(n_own > 1, S[rows, own].astype(F64) / np.maximum(n_own - 1, 1).astype(F64), 0.0)
    m = S.astype(F64) / size[ranks].astype(F64)[None, :]
    m[rows, own] = np.inf
    if ranks.size > 1:
        col = np.argmin(m, axis=1)                           # (argmin returns the first, i.e. lowest, rank of the minimum)
        mb = m[rows, col]
        top = np.maximum(ma, mb)
        zero = (n_own == 1) | (top == 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            si = np.where(zero, 0.0, (mb - ma) / np.where(zero, 1.0, top))
        b[idx] = mb / SCALE
        other[idx] = ranks[col].astype(np.int32)
    else:
        si = np.zeros(idx.size)
    a[idx], s[idx] = ma / SCALE, si
    T = np.rint(si * TSCALE).astype(np.int64)
    sums = np.zeros(K, np.int64)
    np.add.at(sums, labels[idx], T)
    cluster_mean[ranks] = (sums[ranks].astype(F64) / size[ranks].astype(F64)) / TSCALE
    mean = F64(F64(int(T.sum())) / F64(idx.size)) / TSCALE
    return a, b, s, other, size, cluster_mean, F64(mean), 0


def textbook(dist, labels):
    """(a, b, s float64 [G], other int32 [G], gap float64 [G]) by the plain float64 definition on the unquantised matrix: no fixed
    point, numpy's own summation.  `gap` is the difference between the two smallest mean distances to other clusters (+inf with
    fewer than two): where it is small, `other` is not determined.  Left-out conformers: NaN, -1."""
    d = np.asarray(dist, dtype=F64)
    G = d.shape[0]
    labels = np.asarray(labels).reshape(-1)
    a, b, s, gap = np.full(G, np.nan), np.full(G, np.nan), np.full(G, np.nan), np.full(G, np.inf)
    other = np.full(G, -1, np.int32)
    ranks = [c for c in np.unique(labels) if c >= 0]
    cols = {c: np.flatnonzero(labels == c) for c in ranks}
    for i in range(G):
        if labels[i] < 0:
            continue
        mine = cols[labels[i]]
        mine = mine[mine != i]
        a[i] = d[i, mine].mean() if mine.size else 0.0
        means = sorted((d[i, cols[c]].mean(), c) for c in ranks if c != labels[i])
        if not means:
            s[i] = 0.0
            continue
        b[i], other[i] = means[0]
        if len(means) > 1:
            gap[i] = means[1][0] - means[0][0]
        top = max(a[i], b[i])
        s[i] = 0.0 if mine.size == 0 or top == 0 else (b[i] - a[i]) / top
    return a, b, s, other, gap
