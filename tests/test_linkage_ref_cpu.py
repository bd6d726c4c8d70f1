"""No GPU: anchors tests/linkage_ref.py, the numpy restatement of agdiff_linkage and agdiff_linkage_cut that the GPU tests hold the
kernels to -- on hand-worked trees of 3-5 points for each method, ties included; on a pure-Python brute force that recomputes every
cluster pair from the members at every merge; and, where scipy imports, on scipy.cluster.hierarchy.linkage.

The scipy gate is 2^-28, one unit of the fixed-point grid: half a unit is the quantiser's share (|Q(x) 2^-28 - x| <= 2^-29, and a
minimum, a maximum or a mean of numbers that are each within 2^-29 of their originals is within 2^-29 of the original's), the other
half is budgeted to scipy's float64 recurrences, whose errors on these sizes are near 1e-15."""
import numpy as np
import pytest

import linkage_ref as LR

F32 = np.float32
METHODS = ("single", "complete", "average")


def _matrix(G, pairs, fill):
    d = np.full((G, G), F32(fill))
    np.fill_diagonal(d, 0)
    for (i, j), v in pairs.items():
        d[i, j] = d[j, i] = v
    return d


def _records(tree):
    left, right, height, size, order, status = tree
    n = int((left >= 0).sum())
    return [(int(left[t]), int(right[t]), float(height[t]), int(size[t])) for t in range(n)], order.tolist(), status


# ------------------------------------------------------------------------------------------------ 1. by hand
def test_four_points_on_a_line_by_hand():
    x = np.array([0, 1, 3, 7], dtype=F32)                # d01 = 1, d02 = 3, d03 = 7, d12 = 2, d13 = 6, d23 = 4
    d = np.abs(x[:, None] - x[None, :])
    # single: (0,1) at 1; then W(0,2) = min(3, 2), W(0,3) = min(7, 6), W(2,3) = 4; then W(0,3) = min(6, 4)
    assert _records(LR.linkage(d, "single")) == ([(0, 1, 1.0, 2), (0, 2, 2.0, 3), (0, 3, 4.0, 4)], [0, 1, 2, 3], 0)
    # complete: W(0,2) = max(3, 2) = 3 < W(2,3) = 4; then W(0,3) = max(7, 6, 4)
    assert _records(LR.linkage(d, "complete")) == ([(0, 1, 1.0, 2), (0, 2, 3.0, 3), (0, 3, 7.0, 4)], [0, 1, 2, 3], 0)
    # average: W(0,2) = 3 + 2 over 2 pairs = 2.5 < 4; then W(0,3) = 7 + 6 + 4 over 3 pairs
    assert _records(LR.linkage(d, "average")) == ([(0, 1, 1.0, 2), (0, 2, 2.5, 3), (0, 3, 17.0 / 3.0, 4)], [0, 1, 2, 3], 0)


@pytest.mark.parametrize("method", METHODS)
def test_ties_go_to_the_lowest_first_slot_then_the_lowest_second(method):
    d = _matrix(4, {(0, 1): 2, (2, 3): 2}, 5)            # two pairs at 2, everything else at 5
    assert _records(LR.linkage(d, method)) == ([(0, 1, 2.0, 2), (2, 3, 2.0, 2), (0, 2, 5.0, 4)], [0, 1, 2, 3], 0)
    d = _matrix(3, {}, 1)                                # all equal: (0, 1), not (0, 2) or (1, 2)
    assert _records(LR.linkage(d, method)) == ([(0, 1, 1.0, 2), (0, 2, 1.0, 3)], [0, 1, 2], 0)
    d = _matrix(5, {(1, 4): 1, (1, 3): 1, (0, 2): 1}, 3)     # (0, 2) before (1, 3) before (1, 4)
    recs, order, _ = _records(LR.linkage(d, method))
    assert [r[:2] for r in recs[:2]] == [(0, 2), (1, 3)]
    if method == "single":                               # ... and {1, 3} - 4 at 1; then {0, 2} - {1, 3, 4} at 3
        assert recs == [(0, 2, 1.0, 2), (1, 3, 1.0, 2), (1, 4, 1.0, 3), (0, 1, 3.0, 5)] and order == [0, 2, 1, 3, 4]
    elif method == "complete":                           # {1, 3} - 4 is max(1, 3) = 3 like everything else: (0, 1) first
        assert recs == [(0, 2, 1.0, 2), (1, 3, 1.0, 2), (0, 1, 3.0, 4), (0, 4, 3.0, 5)] and order == [0, 2, 1, 3, 4]
    else:                                                # {1, 3} - 4 is (1 + 3) / 2 = 2 < 3
        assert recs == [(0, 2, 1.0, 2), (1, 3, 1.0, 2), (1, 4, 2.0, 3), (0, 1, 3.0, 5)] and order == [0, 2, 1, 3, 4]


@pytest.mark.parametrize("method", METHODS)
def test_leaf_order_and_cuts_by_hand(method):
    d = _matrix(4, {(0, 3): 1, (1, 2): 2}, 10)
    tree = LR.linkage(d, method)
    assert _records(tree) == ([(0, 3, 1.0, 2), (1, 2, 2.0, 2), (0, 1, 10.0, 4)], [0, 2, 3, 1], 0)     # leaves: 0 3 1 2
    med, labels, near, size, within, cost, K, status = LR.cut(d, tree, count=2)
    assert (K, status) == (2, 0) and labels.tolist() == [0, 1, 1, 0] and med.tolist() == [0, 1, -1, -1]      # equal costs: the lowest
    assert near.tolist() == [0, 0, 2, 1] and size.tolist() == [2, 2, 0, 0] and within.tolist() == [1, 2, 0, 0] and cost == 3
    for stop, want in ((1.0, [0, 1, 2, 0]), (0.5, [0, 1, 2, 3]), (1.9999, [0, 1, 2, 0]), (2.0, [0, 1, 1, 0]), (9.0, [0, 1, 1, 0]),
                       (10.0, [0, 0, 0, 0]), (np.inf, [0, 0, 0, 0])):      # <= is inclusive
        assert LR.cut(d, tree, stop=stop)[1].tolist() == want, stop
    assert LR.cut(d, tree, count=3, stop=10.0)[1].tolist() == [0, 1, 2, 0]           # both tests: the count stops it first
    assert LR.cut(d, tree, count=2, stop=0.5)[1].tolist() == [0, 1, 2, 3]            # ... the height
    for count in (4, 5, 100):
        got = LR.cut(d, tree, count=count)
        assert got[6] == 4 and got[0].tolist() == [0, 1, 2, 3] and got[5] == 0 and not got[2].any()
    whole = LR.cut(d, tree)                              # row sums 21, 22, 22, 21: the lowest index of the two
    assert whole[6] == 1 and whole[0].tolist() == [0, -1, -1, -1] and whole[2].tolist() == [0, 10, 10, 1] and whole[5] == 21


def test_the_first_failing_merge_ends_the_cut_whatever_comes_later():
    left, right = np.array([0, 2, 0, -1], np.int32), np.array([1, 3, 2, -1], np.int32)
    height = np.array([3.0, 1.0, 4.0, np.nan])           # not monotone: the cut at 2 stops at merge 0 and never sees merge 1
    tree = (left, right, height, np.array([2, 2, 4, 0], np.int32), np.array([0, 1, 2, 3], np.int32))
    d = _matrix(4, {}, 1)
    assert LR.cut(d, tree, stop=2.0)[1].tolist() == [0, 1, 2, 3]
    assert LR.cut(d, tree, stop=3.0)[1].tolist() == [0, 0, 1, 1]
    bad = (left, np.array([1, 2, 2, -1], np.int32)) + tree[2:]               # merge 1 is (2, 2): not a merge
    got = LR.cut(d, bad, stop=3.5)
    assert got[7] == 2 and got[6] == 0 and (got[0] == -1).all() and (got[1] == -1).all() and np.isnan(got[2]).all()


@pytest.mark.parametrize("method", METHODS)
def test_only_the_upper_triangle_and_the_anchors_row_are_read(method):
    d = LR.random_metric(9, seed=1)
    want = LR.linkage(d, method)
    assert LR.same_tree(LR.linkage(np.triu(d, 1), method), want)
    junk = LR.upper_only(d)
    junk[0, 0] = np.nan
    assert LR.same_tree(LR.linkage(junk, method), want)
    assert LR.same(LR.cut(junk, want, count=3)[1], LR.cut(d, want, count=3)[1])


@pytest.mark.parametrize("method", METHODS)
def test_ineligible_conformers_invalid_entries_and_anchors(method):
    base = LR.random_metric(7, seed=3)
    d = LR.with_inf(base, [2, 5])
    left, right, height, size, order, status = tree = LR.linkage(d, method)
    assert status == 0 and (order >= 0).tolist() == [True, True, False, True, True, False, True]
    assert sorted(order[order >= 0].tolist()) == list(range(5)) and (left[:4] >= 0).all() and (left[4:] == -1).all()
    assert np.isnan(height[4:]).all() and not size[4:].any() and not set(left[:4]) & {2, 5} and not set(right[:4]) & {2, 5}
    keep = [0, 1, 3, 4, 6]
    small = LR.linkage(base[np.ix_(keep, keep)], method)
    assert np.array_equal(np.array(keep)[small[0][:4]], left[:4]) and np.array_equal(height[:4], small[2][:4])
    got = LR.cut(d, tree, count=2)
    assert (got[1][[2, 5]] == -1).all() and np.isnan(got[2][[2, 5]]).all() and got[3].sum() == 5
    alone = LR.linkage(d, method, anchor=2)              # an unusable anchor is alone with itself: no merge
    assert alone[5] == 0 and alone[4].tolist() == [-1, -1, 0, -1, -1, -1, -1] and (alone[0] == -1).all()
    for anchor in (-1, 7, 1 << 30):
        out = LR.linkage(d, method, anchor=anchor)
        assert out[5] == 2 and (out[4] == -1).all() and (out[0] == -1).all() and np.isnan(out[2]).all() and not out[3].any()
        assert LR.cut(d, out)[6] == 0
    e = np.array(base)
    e[1, 4] = np.nan                                     # between two eligible conformers: as far as the cap, 2^40
    h = LR.linkage(e, method)[2]
    if method != "single":
        assert np.nanmax(h) * 2.0 ** 28 >= 2.0 ** 40 / 12
    assert LR.brute(e, method)[0] == _records(LR.linkage(e, method))[0]


# ------------------------------------------------------------------------------------------------ 2. brute force
def _cases():
    yield "metric", LR.random_metric(12, seed=12)
    yield "metric5", LR.random_metric(5, seed=5)
    yield "ties", LR.small_values(10, seed=4)
    yield "ties2", LR.small_values(11, seed=7, values=(1.0, 2.0))
    yield "line", LR.line(9)
    yield "star", LR.star(8)
    yield "inf", LR.with_inf(LR.random_metric(10, seed=2), [3, 9])
    top = np.nextafter(F32(4096), F32(0))
    yield "large", LR.small_values(10, seed=8, values=(4096.0, float(top), 4000.0, 3.0))
    yield "one", np.zeros((1, 1), F32)
    yield "two", _matrix(2, {}, 0.75)
    yield "zero", np.zeros((6, 6), F32)


@pytest.mark.parametrize("method", METHODS)
def test_restatement_equals_the_brute_force(method):
    for name, d in _cases():
        for anchor in (0, d.shape[0] - 1):
            tree = LR.linkage(d, method, anchor)
            merges, leaves = LR.brute(d, method, anchor)
            recs, order, status = _records(tree)
            assert status == 0 and recs == merges, (name, anchor)
            assert [order[j] for j in leaves] == list(range(len(leaves))), (name, anchor)
            sets, heights = LR.members_of(tree)
            assert len(sets) == max(len(leaves) - 1, 0) and (not sets or sets[-1] == frozenset(leaves))
            if method != "average":                      # exact arithmetic: monotone
                assert (np.diff(heights) >= 0).all()


def test_cut_labels_are_nested_and_medoids_are_the_cheapest_members():
    d = LR.random_metric(40, seed=40)
    q = LR.Q(d)
    for method in METHODS:
        tree = LR.linkage(d, method)
        before = None
        for K in range(40, 0, -1):
            med, labels, near, size, within, cost, n, status = LR.cut(d, tree, count=K)
            assert (n, status) == (K, 0) and size[:K].sum() == 40 and (size[K:] == 0).all() and (med[K:] == -1).all()
            firsts = [int(np.flatnonzero(labels == r)[0]) for r in range(K)]
            assert firsts == sorted(firsts)              # ranked by ascending slot
            if before is not None:                       # every cluster of K + 1 lies inside one of K
                assert all(len(set(labels[before == r])) == 1 for r in range(K + 1))
            before = labels
            for r in range(K):
                idx, c = LR.member_costs(q, labels, r)
                assert c[np.searchsorted(idx, med[r])] == c.min() and idx[int(np.argmin(c))] == med[r]
                assert within[r] * 2.0 ** 28 == c.min()
            assert within.sum() == cost
        if method == "average":
            continue
        for t, h in enumerate(tree[2][:39]):             # a cut at (the float32 at or above) a merge's own height applies it
            T = F32(h) if float(F32(h)) >= h else np.nextafter(F32(h), F32(np.inf))
            assert LR.cut(d, tree, stop=float(T))[6] <= 39 - t      # (these heights are on the grid and monotone)


# ------------------------------------------------------------------------------------------------ 3. scipy
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("G", [2, 3, 17, 64, 65, 130])
def test_member_sets_and_heights_equal_scipys(G, method):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    d = LR.random_metric(G, seed=G)
    Z = hierarchy.linkage(squareform(d.astype(np.float64), checks=False), method=method)
    sets = {i: frozenset([i]) for i in range(G)}
    want = []
    for t, (a, b, h, n) in enumerate(Z):
        sets[G + t] = sets.pop(int(a)) | sets.pop(int(b))
        assert len(sets[G + t]) == n
        want.append(sets[G + t])
    got, heights = LR.members_of(LR.linkage(d, method))
    assert got == want
    worst = float(np.abs(heights - Z[:, 2]).max())
    print("G = %d, %s: max |height - scipy's| = %.3e (gate 2^-28 = %.3e)" % (G, method, worst, 2.0 ** -28))
    assert worst <= 2.0 ** -28
