"""No GPU: tests/kmedoids_ref.py, the numpy restatement of agdiff_kmedoids' rule that the GPU tests compare the kernels with, is
itself anchored here: on hand-worked cases, on the quantiser's corner values, on brute force for tiny matrices and on the
invariants of the rule on seeded matrices."""
import itertools

import numpy as np
import pytest

import kmedoids_ref as KR

F32 = np.float32


def _run(d, init, **kw):
    trace = []
    res = KR.kmedoids(d, init, trace=trace, **kw)
    KR.check_invariants(d, init, res, trace)
    return res


@pytest.mark.parametrize("n, seed, want", [(2, 1, 1), (2, 0, 0), (4, 0, 1), (4, 3, 1)])
def test_hand_worked_lines(n, seed, want):
    """line(2): the costs tie and the incumbent keeps its place; line(4): costs 6, 4, 4, 6, the lowest index among the ties"""
    med, labels, near, size, within, cost, n_iter, status = _run(KR.line(n), [seed])
    assert med.tolist() == [want] and status == 0 and labels.tolist() == [0] * n and size.tolist() == [n]
    assert near.tolist() == [abs(j - want) for j in range(n)]
    assert cost == sum(abs(j - want) for j in range(n)) == within[0]
    assert n_iter == (1 if seed == want else 2)
    if n == 4:
        assert KR.member_costs(KR.Q(KR.line(4)), labels, 0)[1].tolist() == [6 << 28, 4 << 28, 4 << 28, 6 << 28]


@pytest.mark.parametrize("seed", [0, 1, 31, 32, 33, 64])
def test_line_65_ends_in_the_middle(seed):
    med, _, near, _, _, cost, n_iter, status = _run(KR.line(65), [seed])
    assert med.tolist() == [32] and status == 0 and n_iter == (1 if seed == 32 else 2) and cost == 2 * sum(range(33))
    assert near.tolist() == [abs(j - 32) for j in range(65)]


def test_quantiser():
    q = lambda x: int(KR.Q(F32(x)))
    assert q(1.0) == 2 ** 28 and q(-0.0) == 0 and q(0.0) == 0
    for x in (np.nan, -1.0, np.inf, -np.inf, np.nextafter(F32(4096), F32(np.inf)), 4096.0, 5000.0, -1e-30):
        assert q(x) == 2 ** 40, x
    assert q(np.nextafter(F32(4096), F32(0))) == 2 ** 40 - 2 ** 16           # (the largest valid value below the cap: 24 bits)
    # half-way cases round to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert [q(k * 2.0 ** -29) for k in (1, 3, 5, 7)] == [0, 2, 2, 4]
    assert q(2.0 ** -30) == 0 and q(3 * 2.0 ** -30) == 1
    assert KR.valid(F32(-0.0)) and KR.valid(F32(4096)) and not KR.valid(np.nextafter(F32(4096), F32(np.inf)))
    assert KR.Q(np.array([[1.0, np.nan], [-0.0, 2.5]], F32)).tolist() == [[2 ** 28, 2 ** 40], [0, 5 << 27]]


def test_iteration_limit_and_status():
    d = KR.line(1025)
    full = _run(d, list(range(7)), max_iter=128)
    assert full[7] == 0 and full[6] > 64                                     # (not converged after 64 updates)
    for it in (1, 2, 64):
        med, labels, near, size, within, cost, n_iter, status = _run(d, list(range(7)), max_iter=it)
        assert status == 1 and n_iter == it
    again = _run(d, list(range(7)), max_iter=int(full[6]))
    assert again[7] == 0 and KR.same(again, full)                            # the update that changed nothing is counted
    short = _run(d, list(range(7)), max_iter=int(full[6]) - 1)
    assert short[7] == 1 and KR.same(short[:6], full[:6])                    # (the same medoids, one update earlier: not yet known)


def test_bad_seeds_give_status_two():
    d = KR.with_inf(KR.random_metric(9, seed=1), [4])
    for init in ([0, 0], [1, 2, 1], [-1], [0, 9], [9], [0, 4], [4, 0], [3, -1]):
        med, labels, near, size, within, cost, n_iter, status = KR.kmedoids(d, init)
        assert status == 2 and n_iter == 0 and cost == 0 and (med == -1).all() and (labels == -1).all() and np.isnan(near).all()
        assert len(med) == len(init) and not size.any() and not within.any()
    assert KR.kmedoids(d, [0, 3])[7] == 0


def test_ineligible_conformers_and_bad_entries():
    d = KR.with_inf(KR.random_metric(12, seed=3), [2, 7])
    res = _run(d, [0, 5, 11])
    assert res[1][[2, 7]].tolist() == [-1, -1] and np.isnan(res[2][[2, 7]]).all() and res[3].sum() == 10
    sub = np.delete(np.delete(KR.random_metric(12, seed=3), [2, 7], 0), [2, 7], 1)       # the same walk without them
    want = KR.kmedoids(sub, [0, 4, 9])
    keep = np.delete(np.arange(12), [2, 7])
    assert keep[want[0]].tolist() == res[0].tolist() and KR.same(want[3:], res[3:])
    for badv in (np.nan, -1.0, 5000.0, np.inf):                              # an eligible pair's bad entry counts as the cap
        e = KR.random_metric(12, seed=3)
        e[5, 6] = e[6, 5] = badv
        capped = e.copy()
        capped[5, 6] = capped[6, 5] = 4096.0
        a, b = _run(e, [0, 5]), _run(capped, [0, 5])
        assert KR.same(a[:2], b[:2]) and KR.same(a[3:], b[3:])
        if a[1][6] == 1:                                                     # near is the entry as stored
            assert KR.same([a[2][6]], [F32(badv)])
    z = KR.random_metric(6, seed=2)
    z[z == 0] = -0.0
    z[0, 1] = z[1, 0] = -0.0
    pos = np.where(z == 0, F32(0), z)
    assert KR.same(_run(z, [0, 3]), _run(pos, [0, 3])) and not np.signbit(_run(z, [0, 3])[2]).any()


def _brute_costs(d, labels, r):
    """the member costs of cluster r with python integers, entry by entry"""
    idx = [j for j in range(len(labels)) if labels[j] == r]
    return idx, [sum(int(KR.Q(d[i, j])) for j in idx if j != i) for i in idx]


@pytest.mark.parametrize("G", [2, 3, 5, 8])
def test_brute_force_no_swap_inside_a_cluster_lowers_the_cost(G):
    for seed in range(6):
        d = KR.random_metric(G, seed=100 * G + seed) if seed % 2 else KR.small_values(G, seed=seed)
        for init in itertools.permutations(range(G), 2):
            if seed > 1 and init[0] > 1:
                continue
            res = _run(d, list(init))
            med, labels = res[0], res[1]
            assert res[7] == 0
            for r in range(2):
                idx, costs = _brute_costs(d, labels, r)
                assert min(costs) == costs[idx.index(med[r])]                # no single-medoid swap inside the cluster is cheaper
                assert res[4][r] * 2 ** 28 == costs[idx.index(med[r])]       # within is the medoid's cost
            for j in range(G):                                               # and the labels are the lowest-rank nearest medoid
                if j not in med.tolist():
                    qs = [int(KR.Q(d[m, j])) for m in med]
                    assert labels[j] == qs.index(min(qs))


@pytest.mark.parametrize("G, K", [(1, 1), (2, 2), (17, 1), (17, 17), (65, 7), (130, 40), (257, 100)])
def test_invariants_on_seeded_matrices(G, K):
    d = KR.random_metric(G, seed=G)
    seeds = [list(range(K)), list(range(G - K, G)), KR.maxmin(d, K)[0].tolist()]
    for init in seeds:
        res = _run(d, init)
        assert res[7] == 0
        if K == G:
            assert res[6] == 1 and res[5] == 0 and res[0].tolist() == init
    for dd in (KR.small_values(G, seed=G), np.zeros((G, G), F32), np.full((G, G), F32(2.5)), KR.with_inf(d, [G // 2] if G > K else [])):
        if G > K or dd is not d:
            res = _run(dd, seeds[0])
    zero = _run(np.zeros((G, G), F32), seeds[0])                             # everybody but the seeds goes to rank 0: one update
    assert zero[6] == 1 and zero[3].tolist() == [G - K + 1] + [1] * (K - 1)


def test_lattice_and_long_walks():
    d = KR.lattice(3, 2)
    assert d.tolist() == [[0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2], [1, 2, 0, 1, 1, 2], [2, 1, 1, 0, 2, 1], [2, 3, 1, 2, 0, 1],
                          [3, 2, 2, 1, 1, 0]]
    for K in (3, 7, 40):
        for init in (list(range(K)), list(range(33 * 31 - K, 33 * 31))):
            res = _run(KR.lattice(33, 31), init)
            assert res[7] == 0 and res[6] >= 3
    res = _run(KR.line(1025), [0, 1, 2])
    assert res[7] == 0 and res[6] >= 8


def test_same_tells_bits_apart():
    a = (np.array([1, 2], np.int32), np.array([0.0, np.nan], F32), np.array([1.5]), np.float64(2.0), 3)
    assert KR.same(a, a)
    assert not KR.same(a, (a[0], np.array([-0.0, np.nan], F32), a[2], a[3], 3))
    assert not KR.same(a, (a[0], a[1], np.array([np.nextafter(1.5, 2)]), a[3], 3))
    assert not KR.same(a, (a[0], a[1], a[2], np.float64(-2.0), 3))
    assert not KR.same(a, (a[0], a[1], a[2], a[3], 4))
    assert not KR.same(a, (a[0][:1], a[1], a[2], a[3], 3))
