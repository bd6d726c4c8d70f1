"""The numpy restatement of agdiff_pam_build / agdiff_pam_swap (tests/pam_ref.py) is what tests/test_hip_pam.py holds the kernels
to, so it is anchored here first: hand-worked cases, brute force over every exchange and every addition on small matrices, the
invariants of the rule, and the claim that motivates the module -- BUILD + SWAP ends below the alternating walk -- as strict
integer inequalities."""
import itertools

import numpy as np
import pytest

import kmedoids_ref as KR
import pam_ref as PR

F32 = np.float32
INF = F32(np.inf)
ONE = 1 << 28                                                # Q(1.0)


def _cost(res):
    return int(round(float(res[5]) * PR.SCALE))


def _pam(d, K, anchor=0, max_swaps=10 ** 6, trace=None):
    b = PR.build(d, K, anchor)
    return b, PR.swap(d, b[0], anchor, max_swaps=max_swaps, trace=trace)


# ---- hand-worked ---------------------------------------------------------------------------------------------------------

def test_line4_k2():
    # the points 0 1 2 3.  Rank 0: row sums 6 4 4 6 -> 1 (the lower of the two).  dn = 1 0 1 2.  gains: c=0: 1; c=2: 1 + (2-1) = 2;
    # c=3: 2 + (1-1) = 2 -> 2, the lower index.  Medoids (1, 2), cost 1 + 0 + 0 + 1 = 2, which no exchange lowers.
    d = PR.line(4)
    picks = []
    b = PR.build(d, 2, picks=picks)
    assert picks == [(1, 4 * ONE), (2, 2 * ONE)]
    assert b[0].tolist() == [1, 2] and b[1].tolist() == [0, 0, 1, 1] and b[2].tolist() == [1, 0, 0, 1]
    assert b[3].tolist() == [2, 2] and b[4].tolist() == [1.0, 1.0] and b[5] == 2.0 and b[6:] == (0, 0)
    s = PR.swap(d, b[0], 0)
    assert KR.same(s, b)                                      # status 0, 0 swaps
    # from the seeds (0, 1): cost 0 + 0 + 1 + 2 = 3.  (c=2, r=0): medoids (2, 1): 1 + 0 + 0 + 1 = 2; (c=2, r=1): (0, 2): 0 + 1 + 0 + 1
    # = 2; (c=3, r=0): (3, 1): 1 + 0 + 1 + 0 = 2; (c=3, r=1): (0, 3): 0 + 1 + 1 + 0 = 2: all -1 -> the lowest candidate and rank
    cands, delta = PR.deltas(PR.Q(d), np.array([0, 1]), np.ones(4, bool))
    assert cands.tolist() == [2, 3] and delta.tolist() == [[-ONE, -ONE], [-ONE, -ONE]]
    s = PR.swap(d, [0, 1])
    assert s[0].tolist() == [2, 1] and s[1].tolist() == [1, 1, 0, 0] and s[5] == 2.0 and s[6:] == (1, 0)


def test_line5_k1_build_gives_the_middle():
    d = PR.line(5)
    picks = []
    b = PR.build(d, 1, picks=picks)
    assert picks == [(2, 6 * ONE)] and b[0].tolist() == [2] and b[5] == 6.0 and b[1].tolist() == [0] * 5
    s = PR.swap(d, [0])                                       # K = 1: ds is infinite; delta(c, 0) = rowsum(c) - 10
    assert s[0].tolist() == [2] and s[6:] == (1, 0) and s[5] == 6.0


def test_zero_matrix_and_two_identical_points():
    z = np.zeros((5, 5), dtype=F32)
    b, s = _pam(z, 3)
    assert b[0].tolist() == [0, 1, 2]                         # every sum and every gain is 0: the lowest index, and 0 still picks
    assert b[1].tolist() == [0, 1, 2, 0, 0] and b[5] == 0.0   # (ties to the lowest rank; a medoid keeps its own)
    assert KR.same(s, b)
    two = np.zeros((2, 2), dtype=F32)
    for K in (1, 2):
        b, s = _pam(two, K)
        assert b[0].tolist() == [0, 1][:K] and b[5] == 0.0 and s[6:] == (0, 0) and KR.same(s, b)


# ---- brute force ----------------------------------------------------------------------------------------------------------

def _matrices():
    for G in range(1, 10):
        yield PR.small_values(G, 10 + G)
        yield PR.random_metric(G, 20 + G)
    yield PR.with_inf(PR.random_metric(9, 3), [4, 7])
    d = PR.small_values(9, 5)
    d[2, 6] = np.nan                                          # a bad entry inside eligible rows: 2^40
    d[5, 1] = 5000.0
    yield d
    d = PR.random_metric(8, 6).copy()
    d[np.triu_indices(8, 1)] *= F32(1.5)                      # asymmetric
    yield d


def test_every_delta_is_the_brute_force_change_of_cost():
    for d in _matrices():
        G = d.shape[0]
        q = PR.Q(d)
        eligible = PR.eligible_of(d, 0)
        el = np.flatnonzero(eligible)
        for K in range(1, min(3, len(el)) + 1):
            for med in itertools.permutations(el.tolist(), K):
                med = np.array(med)
                cands, delta = PR.deltas(q, med, eligible)
                assert cands.tolist() == [j for j in el.tolist() if j not in med.tolist()]
                before = PR.total_cost(q, med, eligible)
                for a, c in enumerate(cands):
                    for r in range(K):
                        after = med.copy()
                        after[r] = c
                        assert delta[a, r] == PR.total_cost(q, after, eligible) - before


def test_status_0_means_no_exchange_lowers_the_cost_and_build_picks_the_best_addition():
    for d in _matrices():
        G = d.shape[0]
        q = PR.Q(d)
        eligible = PR.eligible_of(d, 0)
        el = np.flatnonzero(eligible).tolist()
        for K in range(1, min(3, len(el)) + 1):
            picks, trace = [], []
            b = PR.build(d, K, picks=picks)
            for p in range(K):                                # every pick is the best single addition, ties to the lowest index
                have = [c for c, _ in picks[:p]]
                costs = [(PR.total_cost(q, have + [c], eligible), c) for c in el if c not in have]
                assert min(costs)[1] == picks[p][0]
            PR.check_invariants(d, 0, b, swapped=False)
            s = PR.swap(d, b[0], 0, trace=trace)
            PR.check_invariants(d, 0, s, trace)
            assert s[7] == 0 and _cost(s) <= _cost(b)
            for r in range(K):
                for c in el:
                    if c not in s[0].tolist():
                        after = s[0].astype(np.int64)
                        after[r] = c
                        assert PR.total_cost(q, after, eligible) >= _cost(s)


# ---- the invariants of the rule ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,K,seed", [(40, 4, 1), (64, 7, 2), (90, 3, 3)])
def test_trace_falls_memoryless_fixed_point(G, K, seed):
    d = PR.random_metric(G, seed)
    init = np.arange(K)
    trace = []
    full = PR.swap(d, init, trace=trace)
    PR.check_invariants(d, 0, full, trace)
    assert full[7] == 0 and full[6] >= 2
    for a in range(full[6] + 2):                              # swap(a) then swap(b) from its medoids is swap(a + b)
        first = PR.swap(d, init, 0, max_swaps=a)
        assert first[7] == (1 if a <= full[6] else 0) and first[6] == min(a, full[6])
        second = PR.swap(d, first[0], 0, max_swaps=full[6] + 5 - a)
        assert KR.same(second[:6], full[:6]) and first[6] + second[6] == full[6] and second[7] == 0
    alt = KR.kmedoids(d, full[0])                             # a fixed point of the alternating rule
    assert alt[6] == 1 and alt[7] == 0 and KR.same(alt[:6], full[:6])


def test_ties_go_to_the_lowest_candidate_then_the_lowest_rank():
    # line(4) from (0, 1): all four exchanges are at -1 (worked above): candidate 2, rank 0
    s = PR.swap(PR.line(4), [0, 1], max_swaps=1)
    assert s[0].tolist() == [2, 1] and s[6:] == (1, 1)
    # two candidates at equal delta, one rank: line(5) from (0,): rowsums 10 7 6 7 10 -> 2 alone; lattice 2 x 2 from (0,): rowsums
    # 4 4 4 4: nothing lowers
    assert PR.swap(PR.lattice(2, 2), [0])[6:] == (0, 0)
    # two ranks at equal delta for one candidate: the points 0 0 5 with medoids on the two zeros: exchanging either for 2 gives
    # cost 0, from 5
    d = np.array([[0, 0, 5], [0, 0, 5], [5, 5, 0]], dtype=F32)
    cands, delta = PR.deltas(PR.Q(d), np.array([0, 1]), np.ones(3, bool))
    assert cands.tolist() == [2] and delta.tolist() == [[-5 * ONE, -5 * ONE]]
    assert PR.swap(d, [0, 1])[0].tolist() == [2, 1]
    assert PR.swap(d, [1, 0])[0].tolist() == [2, 0]


def test_ineligible_rows_bad_entries_bad_seeds_and_no_candidate():
    d = PR.with_inf(PR.random_metric(12, 4), [3, 8])
    b, s = _pam(d, 3)
    assert b[1][3] == -1 and b[1][8] == -1 and np.isnan(s[2][[3, 8]]).all() and s[3].sum() == 10
    PR.check_invariants(d, 0, s)
    assert 3 not in s[0] and 8 not in s[0]
    assert PR.build(d, 10)[7] == 0 and PR.build(d, 11)[7] == 2            # K against the eligible count
    assert PR.build(d, 2, anchor=12)[7] == 2 and PR.build(d, 2, anchor=-1)[7] == 2
    assert PR.build(d, 1, anchor=3)[0].tolist() == [3]                     # an unusable anchor is alone with itself
    full = PR.build(d, 10)
    s = PR.swap(d, full[0], 0)                                             # K = the eligible count: no candidate
    assert s[6:] == (0, 0) and KR.same(s[:6], full[:6])
    for init, anchor in (([0, 0], 0), ([0, 12], 0), ([-1, 1], 0), ([0, 3], 0), ([1, 2], 3), ([1, 2], 12)):
        bad = PR.swap(d, init, anchor)
        assert bad[7] == 2 and (bad[0] == -1).all() and (bad[1] == -1).all() and np.isnan(bad[2]).all() and bad[5] == 0
    assert PR.swap(d, [1, 2], 0)[7] == 0                                   # the anchor need not be a seed
    e = PR.random_metric(10, 9).copy()
    e[2, 6] = np.nan
    e[5, 1] = 5000.0
    e[4, 7] = -1.0
    b, s = _pam(e, 3)
    PR.check_invariants(e, 0, s)
    assert s[7] == 0


# ---- the claim that motivates the module ----------------------------------------------------------------------------------

@pytest.mark.parametrize("G,K,pam,swaps,alt_maxmin,alt_first", [(200, 5, 193.615, 3, 220.153, 207.582),
                                                                 (1000, 10, 859.893, 9, 889.709, 895.942),
                                                                 (1000, 100, 357.674, 64, 413.337, 419.712)])
def test_build_and_swap_end_below_the_alternating_walk(G, K, pam, swaps, alt_maxmin, alt_first):
    d = PR.random_metric(G, 1)
    q = PR.Q(d)
    b = PR.build(d, K, q=q)
    s = PR.swap(d, b[0], 0, max_swaps=10 ** 6, q=q)
    seeds = PR.maxmin(d, K)[0]
    a_maxmin = KR.kmedoids(d, seeds, max_iter=128, q=q)
    a_first = KR.kmedoids(d, np.arange(K), max_iter=128, q=q)
    assert s[7] == 0 and a_maxmin[7] == 0 and a_first[7] == 0
    assert _cost(s) < _cost(a_maxmin) and _cost(s) < _cost(a_first)        # strict, on integers
    # the figures of the prototype that proposed the rule: a different restatement would not reproduce them
    assert s[6] == swaps and abs(float(s[5]) - pam) < 1e-3
    assert abs(float(a_maxmin[5]) - alt_maxmin) < 1e-3 and abs(float(a_first[5]) - alt_first) < 1e-3
    alt = KR.kmedoids(d, s[0], q=q)
    assert alt[6] == 1 and KR.same(alt[:6], s[:6])
