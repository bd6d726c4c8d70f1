"""No GPU: anchors for tests/silhouette_ref.py, the numpy restatement that tests/test_hip_silhouette.py holds the kernels to --
hand-worked cases with every number written out, brute force on matrices full of exact ties, the invariants of the rule, and the
plain float64 definition (`textbook`) on the unquantised matrix to a derived gate."""
import numpy as np
import pytest

import silhouette_ref as SR

F32, F64 = np.float32, np.float64
NAN = np.nan


def _eq(got, want):
    """doubles bit-equal (NaN at the same places), integers equal"""
    return SR.same([np.asarray(g, dtype=np.asarray(w).dtype) for g, w in zip(got, want)], [np.asarray(w) for w in want])


def _points(*x):
    x = np.array(x, dtype=F32)
    return np.abs(x[:, None] - x[None, :])


def test_four_points_on_a_line_two_and_two():
    a, b, s, other, size, cmean, mean, status = SR.silhouette(_points(0, 1, 10, 11), [0, 0, 1, 1], 2)
    assert status == 0 and size.tolist() == [2, 2] and other.tolist() == [1, 1, 0, 0]
    assert a.tolist() == [1.0, 1.0, 1.0, 1.0] and b.tolist() == [10.5, 9.5, 9.5, 10.5]
    want = [F64(9.5) / F64(10.5), F64(8.5) / F64(9.5), F64(8.5) / F64(9.5), F64(9.5) / F64(10.5)]
    assert s.tolist() == want
    T = [int(np.rint(v * 2.0 ** 40)) for v in want]                           # the means are made on the 2^-40 grid
    assert cmean.tolist() == [(T[0] + T[1]) / 2 / 2.0 ** 40, (T[2] + T[3]) / 2 / 2.0 ** 40] and mean == sum(T) / 4 / 2.0 ** 40
    assert abs(mean - np.mean(want)) < 2.0 ** -40


def test_four_points_on_a_line_one_and_three():
    a, b, s, other, size, cmean, mean, status = SR.silhouette(_points(0, 1, 10, 11), [0, 1, 1, 1], 2)
    assert status == 0 and size.tolist() == [1, 3] and other.tolist() == [1, 0, 0, 0]
    assert a.tolist() == [0.0, 9.5, 5.0, 5.5] and b.tolist() == [F64(22) / F64(3), 1.0, 10.0, 11.0]
    assert s.tolist() == [0.0, (F64(1) - F64(9.5)) / F64(9.5), 0.5, 0.5]     # the singleton scores 0; 1 sits next to the other cluster
    assert cmean[0] == 0.0 and abs(cmean[1] - (1 - 8.5 / 9.5) / 3) < 2.0 ** -40 and abs(mean - (1 - 8.5 / 9.5) / 4) < 2.0 ** -40


def test_a_singleton_between_two_pairs_and_k_one():
    d = _points(0, 1, 5, 9, 10)
    a, b, s, other, size, cmean, mean, status = SR.silhouette(d, [0, 0, 1, 2, 2], 3)
    assert size.tolist() == [2, 1, 2] and s[2] == 0.0 and a[2] == 0.0 and b[2] == 4.5 and other[2] == 0      # 4.5 = 4.5: the lowest rank
    assert other.tolist() == [1, 1, 0, 1, 1] and a.tolist() == [1.0, 1.0, 0.0, 1.0, 1.0] and b.tolist() == [5.0, 4.0, 4.5, 4.0, 5.0]
    assert s.tolist() == [0.8, 0.75, 0.0, 0.75, 0.8] and cmean[1] == 0.0
    # K = 1: no other cluster -- b NaN, other -1, s 0, a the mean distance to everybody else
    a, b, s, other, size, cmean, mean, status = SR.silhouette(d, [0] * 5, 1)
    assert status == 0 and size.tolist() == [5] and other.tolist() == [-1] * 5 and np.isnan(b).all() and s.tolist() == [0.0] * 5
    assert a.tolist() == [6.25, 5.5, 4.5, 5.5, 6.25] and cmean.tolist() == [0.0] and mean == 0.0
    # one conformer: a singleton with no other cluster
    one = SR.silhouette(np.zeros((1, 1), F32), [0], 1)
    assert _eq(one, ([0.0], [NAN], [0.0], np.array([-1], np.int32), np.array([1], np.int32), [0.0], F64(0), 0))


def test_left_out_bad_labels_and_nobody():
    d = _points(0, 1, 10, 11, 50)
    got = SR.silhouette(d, [0, 0, 1, 1, -1], 2)
    want = SR.silhouette(d[:4, :4], [0, 0, 1, 1], 2)
    assert _eq([x[:4] for x in got[:4]] + list(got[4:]), want)                # the left-out conformer changes nothing ...
    assert np.isnan(got[0][4]) and np.isnan(got[1][4]) and np.isnan(got[2][4]) and got[3][4] == -1       # ... and gets NaN / -1
    poisoned = np.array(d)
    poisoned[:, 4] = np.nan                                                   # its column is never read
    assert _eq(SR.silhouette(poisoned, [0, 0, 1, 1, -1], 2), got)
    diag = np.array(d)
    diag[np.arange(5), np.arange(5)] = np.inf                                 # neither is the diagonal
    assert _eq(SR.silhouette(diag, [0, 0, 1, 1, -1], 2), got)
    for labels in ([0, 0, 1, 2, -1], [0, 0, 1, 1, -2], [-5, 0, 1, 1, 0]):
        a, b, s, other, size, cmean, mean, status = SR.silhouette(d, labels, 2)
        assert status == 2 and np.isnan(a).all() and np.isnan(b).all() and np.isnan(s).all() and (other == -1).all()
        assert size.tolist() == [0, 0] and np.isnan(cmean).all() and np.isnan(mean)
    a, b, s, other, size, cmean, mean, status = SR.silhouette(d, [-1] * 5, 3)
    assert status == 0 and np.isnan(a).all() and np.isnan(s).all() and (other == -1).all() and size.tolist() == [0, 0, 0]
    assert np.isnan(cmean).all() and np.isnan(mean)


def test_an_asymmetric_matrix_is_read_along_row_i():
    d = np.array([[0, 1, 7], [2, 0, 8], [3, 4, 0]], dtype=F32)
    a, b, s, other, _, _, _, _ = SR.silhouette(d, [0, 0, 1], 2)
    assert a.tolist() == [1.0, 2.0, 0.0] and b.tolist() == [7.0, 8.0, 3.5] and s.tolist() == [F64(6) / F64(7), 0.75, 0.0]


def test_invalid_entries_count_as_two_to_the_forty():
    d = _points(0, 1, 10, 11)
    d[0, 1] = np.inf
    d[2, 0] = np.nan
    d[3, 1] = -1.0
    a, b, s, other, _, _, _, _ = SR.silhouette(d, [0, 0, 1, 1], 2)
    assert a[0] == 4096.0 and b[2] == (4096.0 + 9.0) / 2 and b[3] == (11.0 + 4096.0) / 2 and a[1] == 1.0


def _brute(d, labels, K):
    """(other, s) by loops over python floats: the rule read literally"""
    q = SR.Q(d)
    G = d.shape[0]
    size = [sum(1 for l in labels if l == c) for c in range(K)]
    other, s, ties = [], [], 0
    for i in range(G):
        own = labels[i]
        sums = [sum(int(q[i, j]) for j in range(G) if j != i and labels[j] == c) for c in range(K)]
        ma = float(sums[own]) / float(size[own] - 1) if size[own] > 1 else 0.0
        means = [(float(sums[c]) / float(size[c]), c) for c in range(K) if c != own and size[c] > 0]
        if not means:
            other.append(-1)
            s.append(0.0)
            continue
        mb, c = min(means)                                   # (lowest mean, then lowest rank)
        ties += sum(1 for v, _ in means if v == mb) > 1
        other.append(c)
        s.append(0.0 if size[own] == 1 or max(ma, mb) == 0 else (mb - ma) / max(ma, mb))
    return other, s, ties


@pytest.mark.parametrize("shape, K", [((5, 5), 4), ((7, 5), 6), ((6, 6), 9)])
def test_ties_go_to_the_lowest_rank(shape, K):
    """integer distances and clusters of equal sizes: many conformers have two nearest other clusters at exactly the same mean"""
    d = SR.lattice(*shape)
    G = d.shape[0]
    tied = 0
    for seed in range(4):
        labels = np.random.default_rng(seed).permutation(np.arange(G) % K)
        other, s, ties = _brute(d, labels.tolist(), K)
        got = SR.silhouette(d, labels, K)
        assert got[3].tolist() == other and got[2].tolist() == s
        tied += ties
    assert tied >= 8
    # three ranks at the corners of a symmetric arrangement: the centre is equally far from both ends
    line = SR.line(3)
    assert SR.silhouette(line, [0, 2, 1], 3)[3].tolist() == [2, 0, 2] and SR.silhouette(line, [1, 2, 0], 3)[3].tolist() == [2, 0, 2]


@pytest.mark.parametrize("G, K", [(40, 3), (129, 7), (300, 40)])
def test_invariants(G, K):
    rng = np.random.default_rng(G)
    d = SR.random_metric(G, seed=G)
    labels = rng.integers(0, K, size=G)
    labels[rng.random(G) < 0.1] = -1
    a, b, s, other, size, cmean, mean, status = base = SR.silhouette(d, labels, K)
    ok = labels >= 0
    assert status == 0 and (s[ok] >= -1).all() and (s[ok] <= 1).all() and size.sum() == ok.sum() and np.isnan(s[~ok]).all()
    assert -1 <= mean <= 1 and abs(mean - s[ok].mean()) < 2.0 ** -39 and (a[ok] >= 0).all() and (b[ok] > 0).all()
    for c in range(K):
        assert np.isnan(cmean[c]) if size[c] == 0 else abs(cmean[c] - s[labels == c].mean()) < 2.0 ** -39
    # a permutation of the ranks: s, a, b stay bit for bit, `other` goes through the permutation (no exact ties on this matrix)
    perm = rng.permutation(K)
    moved = np.where(ok, perm[np.maximum(labels, 0)], -1)
    pa, pb, ps, pother, psize, pcmean, pmean, _ = SR.silhouette(d, moved, K)
    assert _eq((pa, pb, ps, pmean), (a, b, s, mean)) and np.array_equal(pother, np.where(other >= 0, perm[np.maximum(other, 0)], -1))
    assert np.array_equal(psize[perm], size) and _eq((pcmean[perm],), (cmean,))
    # a permutation of the conformers: every sum is a sum of integers, so the outputs move with them bit for bit
    p = rng.permutation(G)
    qa, qb, qs, qother, qsize, qcmean, qmean, _ = SR.silhouette(d[np.ix_(p, p)], labels[p], K)
    assert _eq((qa, qb, qs, qother, qsize, qcmean, qmean), (a[p], b[p], s[p], other[p], size, cmean, mean))
    # empty ranks on top: nothing changes but the sizes and the NaN means
    more = SR.silhouette(d, labels, K + 5)
    assert _eq(more[:4] + more[6:], base[:4] + base[6:]) and more[4].tolist() == size.tolist() + [0] * 5
    assert _eq((more[5][:K],), (cmean,)) and np.isnan(more[5][K:]).all()
    # empty ranks in the middle: the ranks spread out to 2 c
    wide = SR.silhouette(d, np.where(ok, 2 * labels, -1), 2 * K)
    assert _eq(wide[:3] + wide[6:], base[:3] + base[6:]) and np.array_equal(wide[3], np.where(other >= 0, 2 * other, -1))


@pytest.mark.parametrize("G, K, kind", [(64, 2, "uniform"), (257, 5, "uniform"), (400, 30, "uniform"), (300, 4, "metric")])
def test_against_the_textbook_definition(G, K, kind):
    """The plain float64 silhouette on the UNQUANTISED matrix, off-diagonal entries in [2^-4, 4096].  The gate |ds| <= 2^-23 is
    derived, not measured: Q moves every entry by at most 2^-29 (half a step of the 2^-28 grid), so every mean of entries, a and b
    included, by at most 2^-29.  With M = max(a, b) >= 2^-4 (every entry is), s = (b - a) / M moves by at most
    (|db| + |da|) / M + |s| |dM| / M <= 3 * 2^-29 / M <= 3 * 2^-25 < 2^-23.  The fp64 roundings on both sides (a few 2^-53
    relative per operation, sums of at most 400 terms) are far below the slack between 3 * 2^-25 and 2^-23.
    `other` is compared where the textbook's two smallest means differ by more than 2^-28 -- twice what quantisation can move
    their difference -- and at most 1 % of the conformers may fall under that exclusion."""
    rng = np.random.default_rng(G + K)
    if kind == "uniform":
        d = rng.uniform(2.0 ** -4, 4096.0, size=(G, G)).astype(F32)
        d = np.maximum(np.triu(d, 1) + np.triu(d, 1).T, F32(2.0 ** -4))
    else:
        d = np.clip(SR.random_metric(G, seed=G) * F32(100), F32(2.0 ** -4), F32(4096))
    d[np.arange(G), np.arange(G)] = 0
    d = d.astype(F32)
    off = d[~np.eye(G, dtype=bool)]
    assert off.min() >= 2.0 ** -4 and off.max() <= 4096
    labels = rng.integers(0, K, size=G)
    labels[rng.random(G) < 0.05] = -1
    a, b, s, other, size, cmean, mean, status = SR.silhouette(d, labels, K)
    ta, tb, ts, tother, gap = SR.textbook(d, labels)
    ok = labels >= 0
    assert np.array_equal(np.isnan(s), ~ok) and np.array_equal(np.isnan(ts), ~ok)
    worst = np.abs(s[ok] - ts[ok]).max()
    print("G = %d, K = %d, %s: max |s - textbook| = %.3e (gate %.3e); max |a - textbook| = %.3e, |b| %.3e"
          % (G, K, kind, worst, 2.0 ** -23, np.abs(a[ok] - ta[ok]).max(), np.abs(b[ok] - tb[ok]).max()))
    assert worst <= 2.0 ** -23
    assert np.abs(a[ok] - ta[ok]).max() <= 2.0 ** -28 and np.abs(b[ok] - tb[ok]).max() <= 2.0 ** -28
    clear = ok & (gap > 2.0 ** -28)
    assert (ok & ~clear).sum() <= 0.01 * ok.sum()
    assert np.array_equal(other[clear], tother[clear])
    assert abs(mean - ts[ok].mean()) <= 2.0 ** -23 + 2.0 ** -40


def test_every_conformer_its_own_rank():
    """K = G = 1024: the restatement sorts the columns once and reduces along the rows (no one-hot product), so this is quick"""
    G = 1024
    d = SR.random_metric(G, seed=1)
    a, b, s, other, size, cmean, mean, status = SR.silhouette(d, np.arange(G), G)
    assert status == 0 and (s == 0).all() and (a == 0).all() and (size == 1).all() and mean == 0
    near = np.where(np.eye(G, dtype=bool), np.inf, SR.Q(d).astype(F64)).argmin(1)
    assert np.array_equal(other, near)                                       # every singleton's other cluster is its nearest neighbour
