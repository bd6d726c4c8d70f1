"""No GPU: the numpy restatement of the Butina rule (tests/butina_ref.py) on graphs worked through by hand, its invariants on random
graphs, and an independent cross-check of the static mode against the plain leader loop."""
import numpy as np
import pytest

import butina_ref as BR


def _clusters(leader):
    return sorted(sorted(np.nonzero(leader == c)[0].tolist()) for c in np.unique(leader))


def test_the_seven_vertex_graph_tells_the_two_modes_apart():
    """edges 0-1 0-2 0-3 4-1 4-2 4-5 5-6; counts with the diagonal: 4 3 3 2 4 3 2.  0 wins the tie with 4 and takes 1, 2, 3.
    Static: 4 (count 4) takes 5, then 6 alone.  Reordering: the live counts are 4: 2, 5: 3, 6: 2, so 5 takes 4 and 6."""
    adj = BR.graph(7, BR.SEVEN)
    leader, count, rank = BR.butina(adj, reorder=False)
    assert leader.tolist() == [0, 0, 0, 0, 4, 4, 6]
    assert count.tolist() == [4, 0, 0, 0, 2, 0, 1]
    assert rank.tolist() == [0, 0, 0, 0, 1, 1, 2]
    leader, count, rank = BR.butina(adj, reorder=True)
    assert leader.tolist() == [0, 0, 0, 0, 5, 5, 5]
    assert count.tolist() == [4, 0, 0, 0, 0, 3, 0]
    assert rank.tolist() == [0, 0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("reorder", [False, True])
def test_small_exact_cases(reorder):
    G = 9
    leader, count, rank = BR.butina(np.eye(G, dtype=bool), reorder)                  # the empty graph
    assert leader.tolist() == list(range(G)) and rank.tolist() == list(range(G)) and count.tolist() == [1] * G
    leader, count, rank = BR.butina(np.ones((G, G), dtype=bool), reorder)            # the complete graph
    assert leader.tolist() == [0] * G and rank.tolist() == [0] * G and count.tolist() == [G] + [0] * (G - 1)
    two = BR.graph(6, [(0, 2), (2, 4), (0, 4), (1, 3), (3, 5), (1, 5)])              # two disjoint triangles, interleaved
    leader, count, rank = BR.butina(two, reorder)
    assert leader.tolist() == [0, 1, 0, 1, 0, 1] and rank.tolist() == [0, 1, 0, 1, 0, 1] and count.tolist() == [3, 3, 0, 0, 0, 0]
    star = BR.graph(G, [(G - 1, j) for j in range(G - 1)])                           # a star whose centre is the last index
    leader, count, rank = BR.butina(star, reorder)
    assert leader.tolist() == [G - 1] * G and rank.tolist() == [0] * G and count.tolist() == [0] * (G - 1) + [G]


def test_the_diagonal_is_taken_as_set():
    adj = BR.graph(7, BR.SEVEN)
    bare = adj & ~np.eye(7, dtype=bool)
    for reorder in (False, True):
        for a, b in zip(BR.butina(adj, reorder), BR.butina(bare, reorder)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("G,density", [(1, 0.5), (17, 0.3), (64, 0.1), (130, 0.05), (200, 0.02), (200, 0.3)])
@pytest.mark.parametrize("reorder", [False, True])
def test_invariants_on_random_graphs(G, density, reorder):
    adj = BR.random_graph(G, density, seed=1000 * G + int(100 * density))
    leader, count, rank = BR.butina(adj, reorder)
    cent = np.nonzero(leader == np.arange(G))[0]
    assert np.isin(leader, cent).all()                                   # a partition: every leader is a centroid
    assert adj[np.arange(G), leader].all()                               # every member has its bit to its centroid
    sub = adj[np.ix_(cent, cent)]
    assert not (sub & ~np.eye(cent.size, dtype=bool)).any()              # centroids are pairwise non-adjacent
    assert count.sum() == G and np.array_equal(np.nonzero(count)[0], cent)
    assert np.array_equal(count[cent], np.bincount(leader, minlength=G)[cent])
    assert np.array_equal(np.sort(rank[cent]), np.arange(cent.size)) and np.array_equal(rank, rank[leader])
    if reorder:
        sizes = count[cent][np.argsort(rank[cent])]
        assert (np.diff(sizes) <= 0).all()                               # the cluster sizes never grow again


@pytest.mark.parametrize("G,density", [(7, None), (65, 0.0), (65, 1.0), (130, 0.05), (200, 0.02), (200, 0.5), (1000, 0.02)])
def test_running_counts_equal_the_counts_taken_afresh(G, density):
    """the cheap form that the GPU tests use for their large cases, against the plain one"""
    adj = BR.graph(7, BR.SEVEN) if density is None else BR.random_graph(G, density, seed=7 * G + 1)
    for reorder in (False, True):
        for a, b in zip(BR.butina(adj, reorder), BR.butina(adj, reorder, running=True)):
            assert np.array_equal(a, b)


def _leader_loop(adj):
    """the greedy leader algorithm in conformer order on a boolean adjacency matrix (as tests/test_hip_ensemble.py states it)"""
    G = adj.shape[0]
    kept = np.zeros(G, dtype=bool)
    leader = np.zeros(G, dtype=np.int32)
    count = np.zeros(G, dtype=np.int32)
    for i in range(G):
        hits = np.nonzero(adj[i, :i] & kept[:i])[0]
        if hits.size == 0:
            kept[i], leader[i] = True, i
        else:
            leader[i] = hits[0]
        count[leader[i]] += 1
    return kept.astype(np.int32), leader, count


@pytest.mark.parametrize("G,density", [(7, None), (40, 0.2), (130, 0.05), (200, 0.1)])
def test_static_mode_is_the_leader_walk_in_count_order(G, density):
    adj = BR.graph(7, BR.SEVEN) if density is None else BR.random_graph(G, density, seed=G)
    order = np.lexsort((np.arange(G), -adj.sum(1)))                      # (count descending, index ascending)
    kept, lead, cnt = _leader_loop(adj[np.ix_(order, order)])
    leader, count, rank = BR.butina(adj, reorder=False)
    want_leader, want_count = np.empty(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
    want_leader[order] = order[lead]
    want_count[order] = cnt
    assert np.array_equal(leader, want_leader) and np.array_equal(count, want_count)
    assert np.array_equal(rank[order][kept.astype(bool)], np.arange(kept.sum()))       # created in walk order


def test_pack_follows_the_bit_layout():
    from agdiff_amd.ensemble import bits_pitch
    adj = BR.random_graph(70, 0.3, seed=3)
    for garbage in (None, True):
        b = BR.pack(adj, garbage=garbage)
        assert b.dtype == np.int64 and b.shape == (70, bits_pitch(70) // 8) == (70, 2)
        u = b.view(np.uint64)
        for i, j in ((0, 0), (3, 63), (3, 64), (69, 69), (12, 5)):
            assert bool((int(u[i, j >> 6]) >> (j & 63)) & 1) == bool(adj[i, j])
        pad = (u[:, 1] >> np.uint64(6)) != 0
        assert pad.all() if garbage else not pad.any()
