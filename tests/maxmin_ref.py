"""The rule of agdiff_maxmin_pick (include/agdiff_hip.h) restated in numpy on the SAME float32 matrix with float32 comparisons, so
that every comparison with the kernel is exact: integers equal, floats bit-equal, NaN positions equal.  With it the matrices of
the structured cases.  Shared by tests/test_maxmin_ref_cpu.py (which anchors it on hand-worked cases and on the invariants of the
rule) and tests/test_hip_picks.py (which holds the kernel to it).  Not a test module."""
import numpy as np

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)


def maxmin(dist, K, first=0, stop=-1.0):
    """(picks int32 [K], radius float32 [K], owner int32 [G], near float32 [G], n_picked int, cover float32) of dist [G, G], straight
    from the rule:
      - every conformer starts eligible; whenever a pick p's row is read, every column j that is unpicked and still eligible is
        checked: dist[p][j] not a finite number >= 0 (NaN, +-inf, negative) makes j ineligible for good; -0.0 counts as 0 (and is
        taken as +0.0);
      - pick 0 is `first`, radius[0] = +inf;
      - after each pick p of rank r, every eligible unpicked j with dist[p][j] < near[j] (strict; near starts at +inf) gets
        near[j] = dist[p][j], owner[j] = r -- on ties the owner stays with the earlier pick;
      - the candidate is the eligible unpicked j with the largest near[j], ties to the lowest index;
      - it is picked iff fewer than K are picked and near[candidate] > stop (strict); radius[r] = near[candidate] when chosen;
      - the walk ends at the first candidate that is not picked (cover = its near) or when no candidate exists (cover = 0).
    Entries of picks / radius from n_picked on are -1 / NaN; an ineligible conformer has owner -1 and near NaN; a pick has its own
    rank and near 0.  The diagonal is never looked at."""
    d = np.asarray(dist, dtype=F32)
    G = d.shape[0]
    picks, radius = np.full(K, -1, dtype=np.int32), np.full(K, NAN, dtype=F32)
    owner, near = np.full(G, -1, dtype=np.int32), np.full(G, INF, dtype=F32)
    if G == 0:
        return picks, radius, owner, near, 0, F32(0)
    assert d.shape == (G, G) and 1 <= K <= G and 0 <= first < G and stop == stop
    stop = F32(stop)
    eligible, picked = np.ones(G, dtype=bool), np.zeros(G, dtype=bool)
    picks[0], radius[0], picked[first], owner[first], near[first] = first, INF, True, 0, 0
    n, cover, p = 1, F32(0), first
    for r in range(K):                                       # pick r's row
        row = np.where(d[p] == 0, F32(0), d[p])              # (-0.0 is +0.0)
        unpicked = eligible & ~picked
        with np.errstate(invalid="ignore"):
            bad = unpicked & ~(np.isfinite(row) & (row >= 0))
        eligible &= ~bad
        unpicked &= ~bad
        closer = unpicked & (row < near)                     # (strict, on float32)
        near[closer], owner[closer] = row[closer], r
        if not unpicked.any():
            break                                            # no candidate: cover = 0
        cand = int(np.argmax(np.where(unpicked, near, F32(-1))))       # (argmax returns the first, i.e. lowest, index of the maximum)
        far = near[cand]
        if not (n < K and far > stop):
            cover = far
            break
        picks[n], radius[n], picked[cand], owner[cand], near[cand] = cand, far, True, n, 0
        p, n = cand, n + 1
    owner[~eligible], near[~eligible] = -1, NAN
    return picks, radius, owner, near, n, cover


def same(got, want):
    """True when two results are equal entry for entry: integers equal, floats bit-equal (NaN at the same places, +0 for +0)"""
    for a, b in zip(got, want):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return False
        if a.dtype.kind == "f" or b.dtype.kind == "f":
            a, b = np.atleast_1d(a).astype(F32), np.atleast_1d(b).astype(F32)
            if not np.array_equal(np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32)),
                                  np.where(np.isnan(b), np.uint32(0x7fc00000), b.view(np.uint32))):
                return False
        elif not np.array_equal(a, b):
            return False
    return True


def check_invariants(d, res, K, stop):
    """what any run of the rule gives, from its outputs and the matrix alone (the matrix without -0.0, the eligible columns clean
    in the picked rows)"""
    picks, radius, owner, near, n, cover = res
    d = np.asarray(d, dtype=F32)
    G = d.shape[0]
    assert 1 <= n <= K and (picks[n:] == -1).all() and np.isnan(radius[n:]).all() and not np.isnan(radius[:n]).any()
    p = picks[:n]
    assert len(set(p.tolist())) == n and radius[0] == INF
    assert (np.diff(radius[1:n]) <= 0).all()                                   # radius[1:] non-increasing
    assert cover <= radius[n - 1]
    eligible = owner >= 0
    assert np.array_equal(eligible, ~np.isnan(near)) and eligible[p].all()
    assert np.array_equal(owner[p], np.arange(n)) and (near[p] == 0).all()
    assert cover >= 0 and (near[eligible] <= cover).all()                      # every eligible conformer within cover of a pick
    rest = eligible.copy()
    rest[p] = False
    rows = d[p][:, rest]                                                       # [n, the eligible unpicked]
    assert np.array_equal(near[rest], rows.min(0))                             # near[j] == min over the picks of dist[pick][j]
    assert np.array_equal(owner[rest], rows.argmin(0))                         # ... and owner the EARLIEST minimiser
    if rest.any():
        assert cover == near[rest].max()                                       # every eligible conformer within cover of a pick
    else:
        assert cover == 0
    if n > 1:
        assert (radius[1:n] > F32(stop)).all()
    assert n == K or not rest.any() or cover <= F32(stop)


def random_metric(G, seed, dim=3):
    """float32 [G, G]: the pairwise distances of G seeded random points in `dim` dimensions, summed in float32 one axis at a time;
    exactly symmetric, zero diagonal"""
    x = np.random.default_rng(seed).normal(size=(G, dim)).astype(F32)
    sq = np.zeros((G, G), dtype=F32)
    for a in range(dim):
        diff = x[:, a][:, None] - x[:, a][None, :]
        sq += diff * diff
    return np.sqrt(sq)


def small_values(G, seed, values=(1.0, 2.0, 3.0)):
    """float32 [G, G], symmetric, zero diagonal, every other entry drawn from `values`: nearly every arg-max is a tie"""
    rng = np.random.default_rng(seed)
    d = np.triu(rng.choice(np.asarray(values, dtype=F32), size=(G, G)), 1)
    return (d + d.T).astype(F32)


def line(n):
    """the points 0, 1, ..., n - 1 on a line"""
    x = np.arange(n, dtype=F32)
    return np.abs(x[:, None] - x[None, :])


def with_inf(d, bad):
    """a copy of d with +inf across the rows and columns `bad`, the diagonal left as it is: what agdiff_rmsd_self stores for
    conformers with a coordinate that is not finite"""
    out = np.array(d, dtype=F32)
    diag = np.diag(out).copy()
    out[bad, :] = INF
    out[:, bad] = INF
    out[np.arange(out.shape[0]), np.arange(out.shape[0])] = diag
    return out
