"""No GPU: anchors tests/maxmin_ref.py -- the numpy restatement of agdiff_maxmin_pick's rule that tests/test_hip_picks.py holds the
kernel to -- on hand-worked cases and on what the rule implies for any matrix."""
import numpy as np
import pytest

import maxmin_ref as MR

F32, INF = MR.F32, MR.INF


def _bits(x):
    return np.asarray(x, dtype=F32).view(np.uint32)


def test_nine_points_on_a_line_from_the_end():
    """0 .. 8 from 0: the far end, the middle, then 2 and 6 tie at distance 2 and the lower index goes first"""
    d = MR.line(9)
    picks, radius, owner, near, n, cover = MR.maxmin(d, 4, first=0)
    assert picks.tolist() == [0, 8, 4, 2] and radius.tolist() == [np.inf, 8.0, 4.0, 2.0] and n == 4
    # 1 is at distance 1 of pick 0 (rank 0) and of pick 2 (rank 3): the earlier pick owns it; so 3 (ranks 2, 3) and 6 (ranks 1, 2)
    assert owner.tolist() == [0, 0, 3, 2, 2, 2, 1, 1, 1] and near.tolist() == [0, 1, 0, 1, 0, 1, 2, 1, 0]
    assert cover == 2.0                                      # (6, the candidate that the count of 4 left out)
    picks, radius, owner, near, n, cover = MR.maxmin(d, 9, first=0)
    assert picks.tolist() == [0, 8, 4, 2, 6, 1, 3, 5, 7] and radius.tolist() == [np.inf, 8, 4, 2, 2, 1, 1, 1, 1]
    assert n == 9 and cover == 0 and owner.tolist() == [0, 5, 3, 6, 2, 7, 4, 8, 1] and not near.any()
    assert picks.dtype == np.int32 and owner.dtype == np.int32 and radius.dtype == F32 and near.dtype == F32
    one = MR.maxmin(d, 1, first=0)
    assert one[0].tolist() == [0] and one[4] == 1 and one[5] == 8.0 and one[2].tolist() == [0] * 9
    assert one[3].tolist() == list(range(9))


def test_nine_points_on_a_line_from_the_middle():
    """from 4: both ends tie at 4 (0 first), then 2 and 6 tie at 2"""
    picks, radius, owner, near, n, cover = MR.maxmin(MR.line(9), 9, first=4)
    assert picks.tolist() == [4, 0, 8, 2, 6, 1, 3, 5, 7] and radius.tolist() == [np.inf, 4, 4, 2, 2, 1, 1, 1, 1] and cover == 0
    picks, radius, owner, near, n, cover = MR.maxmin(MR.line(9), 3, first=4)
    assert picks.tolist() == [4, 0, 8] and n == 3 and cover == 2.0
    # 2 is at distance 2 of pick 4 (rank 0) and of pick 0 (rank 1): rank 0 keeps it; 6 likewise
    assert owner.tolist() == [1, 1, 0, 0, 0, 0, 0, 2, 2] and near.tolist() == [0, 1, 2, 1, 0, 1, 2, 1, 0]


def test_stop_is_a_strict_threshold():
    d = MR.line(9)
    picks, radius, owner, near, n, cover = MR.maxmin(d, 9, first=0, stop=4.0)
    assert picks.tolist() == [0, 8] + [-1] * 7 and n == 2 and cover == 4.0           # 4 is AT the threshold: not taken
    assert np.isnan(radius[2:]).all() and radius[:2].tolist() == [np.inf, 8.0]
    below = float(np.nextafter(F32(4.0), F32(0.0)))
    picks, radius, owner, near, n, cover = MR.maxmin(d, 9, first=0, stop=below)
    assert picks[:3].tolist() == [0, 8, 4] and n == 3 and cover == 2.0
    for r in (8.0, 2.0, 1.0):                                # at every radius value of the full run
        res = MR.maxmin(d, 9, first=0, stop=r)
        full = MR.maxmin(d, 9, first=0)
        assert res[4] == int((full[1] > F32(r)).sum()) and res[5] == r
    assert MR.maxmin(d, 9, first=0, stop=np.inf)[4] == 1
    assert MR.same(MR.maxmin(d, 9, first=0, stop=-1.0), MR.maxmin(d, 9, first=0, stop=0.0))  # (no two points coincide)
    z = np.zeros((5, 5), dtype=F32)
    assert MR.maxmin(z, 5, stop=0.0)[4] == 1 and MR.maxmin(z, 5, stop=0.0)[5] == 0
    assert MR.maxmin(z, 5, stop=-1.0)[0].tolist() == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("G", [1, 2, 7, 64, 200])
def test_invariants_on_random_metric_matrices(G):
    d = MR.random_metric(G, seed=G)
    assert np.array_equal(d, d.T) and not np.diag(d).any()
    med = float(np.median(d))
    for K in sorted({1, min(7, G), G}):
        for first in sorted({0, G - 1}):
            for stop in (-1.0, med):
                res = MR.maxmin(d, K, first=first, stop=stop)
                MR.check_invariants(d, res, K, stop)
                assert res[0][0] == first
    full = MR.maxmin(d, G)
    assert full[4] == G and sorted(full[0].tolist()) == list(range(G)) and full[5] == 0
    for K in (1, G // 2, G):                                 # a shorter run is a prefix of the longer one
        if K >= 1:
            res = MR.maxmin(d, K)
            assert np.array_equal(res[0], full[0][:K]) and np.array_equal(_bits(res[1]), _bits(full[1][:K]))
            assert res[5] == (full[1][K] if K < G else 0)


def test_ties_everywhere_go_to_the_lowest_index():
    for G in (5, 33):
        d = np.full((G, G), 2.5, dtype=F32)                  # the all-equal matrix: index order, whatever the diagonal says
        picks, radius, owner, near, n, cover = MR.maxmin(d, G, first=2)
        assert picks.tolist() == [2] + [j for j in range(G) if j != 2] and (radius[1:] == 2.5).all()
        d = MR.small_values(G, seed=G)
        MR.check_invariants(d, MR.maxmin(d, G), G, -1.0)
        MR.check_invariants(d, MR.maxmin(d, G, stop=1.0), G, 1.0)


def test_what_makes_a_conformer_ineligible():
    d = MR.line(9)
    base = MR.maxmin(d, 9)
    # +inf across row and column 3, as agdiff_rmsd_self writes it: 3 is out, the rest is the run without it
    res = MR.maxmin(MR.with_inf(d, [3]), 9)
    keep = [j for j in range(9) if j != 3]
    sub = MR.maxmin(d[np.ix_(keep, keep)], 8)
    assert res[2][3] == -1 and np.isnan(res[3][3]) and res[4] == 8 and res[0][8] == -1 and np.isnan(res[1][8])
    assert [keep[p] for p in sub[0]] == res[0][:8].tolist() and np.array_equal(_bits(sub[1]), _bits(res[1][:8]))
    assert np.array_equal(res[2][keep], sub[2]) and np.array_equal(_bits(res[3][keep]), _bits(sub[3]))
    # several: 0 (the first pick itself is never checked, but its row is all +inf) takes everybody out
    res = MR.maxmin(MR.with_inf(d, [0, 5]), 9, first=0)
    assert res[4] == 1 and res[5] == 0 and res[2].tolist() == [0] + [-1] * 8 and np.isnan(res[3][1:]).all() and res[3][0] == 0
    res = MR.maxmin(MR.with_inf(d, [2, 5]), 9, first=0)
    assert res[4] == 7 and (res[2][[2, 5]] == -1).all() and (res[2][[0, 1, 3, 4, 6, 7, 8]] >= 0).all()
    # a NaN in the first pick's row: that column only
    e = d.copy()
    e[0, 5] = np.nan
    res = MR.maxmin(e, 9)
    assert res[2][5] == -1 and np.isnan(res[3][5]) and (np.delete(res[2], 5) >= 0).all() and res[4] == 8
    # a negative entry in the SECOND pick's row (8), at a column not picked by then: out from there on
    e = d.copy()
    e[8, 3] = -1.0
    res = MR.maxmin(e, 9)
    assert res[0][:2].tolist() == [0, 8] and res[2][3] == -1 and res[4] == 8 and 3 not in res[0].tolist()
    e = d.copy()
    e[8, 3] = -np.inf
    assert MR.maxmin(e, 9)[2][3] == -1
    # entries that are never looked at change nothing: the diagonal, a picked column, a row that is never read
    e = d.copy()
    e[np.arange(9), np.arange(9)] = np.nan
    e[8, 0] = np.nan                                         # (0 is picked when row 8 is read)
    assert MR.same(MR.maxmin(e, 9), base)
    e = d.copy()
    e[7, :] = np.nan                                         # (with K = 4 the picks are 0, 8, 4, 2: row 7 is never read)
    assert MR.same(MR.maxmin(e, 4), MR.maxmin(d, 4))
    # an asymmetric matrix is read by rows: column 3 of row 0 decides, row 3 of column 0 does not
    e = d.copy()
    e[3, 0] = np.inf
    assert MR.maxmin(e, 2)[2][3] == 0


def test_minus_zero_is_a_zero():
    d = MR.line(6)
    d[2] = d[1]                                              # 2 coincides with 1
    d[:, 2] = d[:, 1]
    d[2, 2] = d[1, 2] = d[2, 1] = 0
    neg = np.where(d == 0, F32(-0.0), d)
    assert np.signbit(neg[1, 2]) and np.signbit(neg[0, 0])
    a, b = MR.maxmin(d, 6), MR.maxmin(neg, 6)
    assert MR.same(a, b) and b[4] == 6 and not np.signbit(b[1]).any() and not np.signbit(b[3]).any()
    assert a[1][-1] == 0 and _bits(b[1])[-1] == 0            # the last pick is the duplicate, taken at +0.0
    z = np.full((4, 4), -0.0, dtype=F32)
    res = MR.maxmin(z, 4)
    assert res[0].tolist() == [0, 1, 2, 3] and _bits(res[1])[1:].tolist() == [0, 0, 0] and (res[2] == np.arange(4)).all()
    assert MR.maxmin(z, 4, stop=0.0)[4] == 1                 # -0 > 0 is false: one pick


def test_same_tells_bit_patterns_apart():
    a = (np.array([0.0, np.nan], dtype=F32), np.array([1, 2], dtype=np.int32), 3, F32(0.5))
    assert MR.same(a, a)
    assert not MR.same(a, (np.array([-0.0, np.nan], dtype=F32),) + a[1:])
    assert not MR.same(a, (np.array([0.0, 1.0], dtype=F32),) + a[1:])
    assert not MR.same(a, a[:2] + (4, F32(0.5)))
    assert not MR.same(a, a[:3] + (F32(0.25),))


def test_no_conformers():
    picks, radius, owner, near, n, cover = MR.maxmin(np.zeros((0, 0), dtype=F32), 0)
    assert n == 0 and cover == 0 and picks.shape == radius.shape == owner.shape == near.shape == (0,)
