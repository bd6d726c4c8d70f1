"""The rule of agdiff_linkage and agdiff_linkage_cut (include/agdiff_hip.h) restated in numpy on the uint64 fixed-point image of the
SAME float32 matrix, so that every comparison with the kernels is exact: integers equal, doubles bit-equal, NaN at the same places.
Written to be obviously right, not fast: a full arg-min over the live upper triangle at every merge, only row and column a
recomputed after it.  Shared by tests/test_linkage_ref_cpu.py (which anchors it on hand-worked trees, on a brute force and on scipy)
and tests/test_hip_linkage.py (which holds the kernels to it).  Not a test module."""
import numpy as np

from kmedoids_ref import F32, FAR, NAN, SCALE, U64, Q, line, member_costs, random_metric, same, small_values, valid, with_inf  # noqa: F401

SINGLE, COMPLETE, AVERAGE = 0, 1, 2
METHODS = ("single", "complete", "average")
INF = np.inf


def eligible_of(d, anchor):
    """bool [G]: j == anchor or valid(dist[anchor][j]), along row `anchor`; nobody for an anchor outside [0, G)"""
    G = d.shape[0]
    if not 0 <= anchor < G:
        return np.zeros(G, dtype=bool)
    e = valid(d[anchor])
    e[anchor] = True
    return e


def star(G):
    """float32 [G, G]: one hub (conformer 0) at 1 from all, the rest at 2 from each other"""
    d = np.full((G, G), F32(2))
    d[0, :] = d[:, 0] = 1
    np.fill_diagonal(d, 0)
    return d


def upper_only(d, seed=0):
    """a copy of d with the diagonal and the lower triangle overwritten with NaN and garbage: nothing may change"""
    rng = np.random.default_rng(seed)
    G = d.shape[0]
    junk = rng.choice(np.array([np.nan, -1.0, 0.0, 1e30, np.inf, 0.5], dtype=F32), size=(G, G))
    out = np.where(np.triu(np.ones((G, G), dtype=bool), 1), d, junk).astype(F32)
    return out


def key_of(method, W, sa, sb):
    """the key of a pair of clusters, fp64 in units of 2^-28: (double)W, divided once by the exactly converted count for average"""
    x = np.asarray(W, dtype=U64).astype(np.float64)      # (round to nearest even; exact below 2^53)
    if method == AVERAGE:
        return x / (np.asarray(sa, dtype=np.int64) * np.asarray(sb, dtype=np.int64)).astype(np.float64)
    return x


def linkage(dist, method, anchor=0, q=None):
    """(left int32 [G], right int32 [G], height float64 [G], size int32 [G], order int32 [G], status) straight from the rule"""
    d = np.asarray(dist, dtype=F32)
    G = d.shape[0]
    method = METHODS.index(method) if isinstance(method, str) else method
    assert d.shape == (G, G) and method in (SINGLE, COMPLETE, AVERAGE)
    left, right = np.full(G, -1, np.int32), np.full(G, -1, np.int32)
    height, size, order = np.full(G, np.nan, np.float64), np.zeros(G, np.int32), np.full(G, -1, np.int32)
    if not 0 <= anchor < G:
        return left, right, height, size, order, 2
    idx = np.flatnonzero(eligible_of(d, anchor))         # the eligible conformers: everything below is in their numbering
    M = len(idx)
    sub = d[np.ix_(idx, idx)] if q is None else None
    W = (Q(sub) if q is None else np.asarray(q)[np.ix_(idx, idx)]).astype(U64)
    upper = np.triu(np.ones((M, M), dtype=bool), 1)
    W = np.where(upper, W, U64(0))                       # only the strict upper triangle is read
    csize = np.ones(M, dtype=np.int64)
    live = np.ones(M, dtype=bool)
    keys = np.where(upper, key_of(method, W, 1, 1), INF)
    nxt, tail = np.full(M, -1), np.arange(M)
    join = {SINGLE: np.minimum, COMPLETE: np.maximum, AVERAGE: np.add}[method]
    for t in range(M - 1):
        flat = int(np.argmin(keys))                      # row-major: the lowest a, then the lowest b, of the smallest key
        a, b = divmod(flat, M)
        assert a < b and live[a] and live[b]
        left[t], right[t], height[t], size[t] = idx[a], idx[b], keys[a, b] / SCALE, csize[a] + csize[b]
        wa = np.where(np.arange(M) < a, W[:, a], W[a, :])     # W(a, c) and W(b, c) for every c, from the upper triangle
        wb = np.where(np.arange(M) < b, W[:, b], W[b, :])
        new = join(wa, wb)
        csize[a] += csize[b]
        live[b] = False
        keys[b, :] = keys[:, b] = INF
        nxt[tail[a]], tail[a] = b, tail[b]
        lo, hi = live & (np.arange(M) < a), live & (np.arange(M) > a)     # the other live clusters: column a above, row a after
        W[lo, a], W[a, hi] = new[lo], new[hi]
        keys[lo, a] = key_of(method, new[lo], csize[a], csize[lo])
        keys[a, hi] = key_of(method, new[hi], csize[a], csize[hi])
    if M:
        j, pos = 0, 0                                    # the one list that is left starts at the lowest eligible conformer
        while j >= 0:
            order[idx[j]], pos, j = pos, pos + 1, nxt[j]
        assert pos == M
    return left, right, height, size, order, 0


def cut(dist, tree, count=1, stop=INF, q=None):
    """(medoids int32 [G], labels int32 [G], near float32 [G], size int32 [G], within float64 [G], cost float64, n_clusters,
    status) of the tree (left, right, height, size, order, ...) cut at `count` clusters and height `stop`"""
    d = np.asarray(dist, dtype=F32)
    G = d.shape[0]
    left, right, height, _, order = tree[:5]
    assert count >= 1 and (stop == INF or valid(F32(stop)))
    bound = INF if stop == INF else float(Q(F32(stop))) / SCALE
    eligible = order >= 0
    M = int(eligible.sum())
    parent = np.full(G, -1)
    remaining = M
    for t in range(G - 1):
        if left[t] < 0 or remaining <= count or not height[t] <= bound:
            break
        a, b = int(left[t]), int(right[t])
        if not (0 <= a < b < G and eligible[a] and eligible[b]):
            return (np.full(G, -1, np.int32), np.full(G, -1, np.int32), np.full(G, NAN, F32), np.zeros(G, np.int32),
                    np.zeros(G, np.float64), np.float64(0), 0, 2)
        parent[b] = a
        remaining -= 1
    root = np.arange(G)
    for j in range(G):                                   # (a parent has a lower index: its root is known already)
        if parent[j] >= 0:
            root[j] = root[parent[j]]
    slots = np.flatnonzero(eligible & (root == np.arange(G)))
    K = len(slots)
    labels = np.where(eligible, np.searchsorted(slots, root), -1).astype(np.int32)
    if q is None:
        q = Q(d)
    medoids, size, within = np.full(G, -1, np.int32), np.zeros(G, np.int32), np.zeros(G, np.float64)
    near = np.full(G, NAN, F32)
    total = 0
    for r in range(K):
        members, cost = member_costs(q, labels, r)
        m = members[int(np.argmin(cost))]                # (the first, i.e. lowest, index of the minimum)
        stored = d[m, members]
        row = np.where(stored == 0, F32(0), stored)      # (-0.0 is written as +0.0; a NaN stays)
        row[members == m] = 0
        near[members], medoids[r], size[r] = row, m, len(members)
        s = int(Q(row).sum(dtype=U64))
        within[r], total = np.float64(s) / SCALE, total + s
    return medoids, labels, near, size, within, np.float64(total) / SCALE, K, 0


def members_of(tree):
    """the member sets (frozensets of conformer indices) that the merges make, in order, and their heights"""
    left, right, height, size, order = tree[:5]
    sets = {int(j): frozenset([int(j)]) for j in np.flatnonzero(order >= 0)}
    out = []
    for t in range(len(sets) - 1):
        a, b = int(left[t]), int(right[t])
        sets[a] = sets[a] | sets.pop(b)
        assert len(sets[a]) == size[t]
        out.append(sets[a])
    return out, height[:len(out)]


def brute(dist, method, anchor=0):
    """the same tree by a pure-Python brute force that keeps member lists and recomputes every cluster pair's weight from the
    members' pairs at every merge: (merges [(a, b, key int-or-Fraction-free float, size)], leaf order list)"""
    d = np.asarray(dist, dtype=F32)
    method = METHODS.index(method) if isinstance(method, str) else method
    e = eligible_of(d, anchor)
    q = Q(d)
    clusters = {int(j): [int(j)] for j in np.flatnonzero(e)}
    merges = []
    while len(clusters) > 1:
        best = None
        slots = sorted(clusters)
        for x, a in enumerate(slots):
            for b in slots[x + 1:]:
                pairs = [int(q[min(i, j), max(i, j)]) for i in clusters[a] for j in clusters[b]]
                w = min(pairs) if method == SINGLE else max(pairs) if method == COMPLETE else sum(pairs)
                key = float(w) / float(len(pairs)) if method == AVERAGE else float(w)     # (int -> float rounds to nearest even)
                if best is None or key < best[0]:        # strict: the first, i.e. lowest (a, b), of the smallest key stays
                    best = (key, a, b)
        key, a, b = best
        clusters[a] = clusters[a] + clusters.pop(b)      # b's leaves after a's
        merges.append((a, b, key / SCALE, len(clusters[a])))
    return merges, (next(iter(clusters.values())) if clusters else [])


def same_tree(got, want):
    return same(list(got[:5]) + [int(got[5])], list(want[:5]) + [int(want[5])])
