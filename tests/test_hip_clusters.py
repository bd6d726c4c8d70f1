"""GPU (MI355X): Taylor-Butina clustering (agdiff_amd.clusters; csrc/eval.hip: k_butina_cluster) against the numpy restatement of
its rule (tests/butina_ref.py), bit for bit, and end to end through cluster_conformers and the command line.

The clustering itself is integer work: every comparison with the restatement is exact.  The one tolerance is ALIGN_ATOL, for the
superposed centroids against a float64 Kabsch of the same fp32 inputs: tests/test_hip_ensemble.py measured 2.24e-7 Angstrom as the
largest deviation of agdiff_align_conformers on the MI355X (coordinates reaching 6.3 Angstrom; what rounding the float64 reference
to fp32 loses) and sets its bar at 4 x that, 8.96e-7 Angstrom; the same kernel runs here, under the same bar."""
import functools

import numpy as np
import pytest
import torch

import butina_ref as BR
import tfd_ref as TR

pytestmark = pytest.mark.gpu
ALIGN_MEASURED = 2.24e-7            # tests/test_hip_ensemble.py: ALIGN_MEASURED
ALIGN_ATOL = 4 * ALIGN_MEASURED
SENTINEL, TAIL = -7, 64


def _launch(bits, G, reorder):
    """agdiff_butina_cluster on int64 numpy rows, its three arrays filled with a sentinel and followed by a canary tail: every
    entry below G must have been written, the tail must be as it was.  (leader, count, rank) numpy, n_clusters int."""
    from agdiff_amd import _lib
    dev = torch.from_numpy(np.array(bits)).cuda()          # (a copy: the cached cases are read-only)
    arrays = [torch.full((G + TAIL,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
    n = torch.full((1 + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    _lib.call("agdiff_butina_cluster", dev, G, int(reorder), arrays[0], arrays[1], arrays[2], n)
    out = [a.cpu().numpy() for a in arrays]
    n = n.cpu().numpy()
    for a in out:
        assert (a[G:] == SENTINEL).all()
    assert (n[1:] == SENTINEL).all()
    leader, count, rank = (a[:G] for a in out)
    assert ((leader >= 0) & (leader < max(G, 1))).all() and (count >= 0).all() and (rank >= 0).all()
    return leader, count, rank, int(n[0])


def _same(got, want, what=""):
    leader, count, rank, n = got
    assert np.array_equal(leader, want[0]), what
    assert np.array_equal(count, want[1]), what
    assert np.array_equal(rank, want[2]), what
    assert n == int((want[1] > 0).sum()), what


@functools.lru_cache(maxsize=None)
def _random_case(G, density):
    """(adjacency, packed bits, {reorder: reference}) of a seeded random symmetric graph -- computed once, left unchanged"""
    adj = BR.random_graph(G, density, seed=G * 10 + int(10 * density))
    bits = BR.pack(adj)
    want = {r: BR.butina(adj, r, running=G > 200) for r in (False, True)}
    for a in (adj, bits) + want[False] + want[True]:
        a.setflags(write=False)
    return adj, bits, want


# ------------------------------------------------------------------------------------------------ 1. the kernel against the rule
@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, 128, 130, 1000, 4095, 4096])
def test_kernel_equals_the_restated_rule(G, reorder):
    for density in (0.0, 0.02, 0.5, 1.0):
        adj, bits, want = _random_case(G, density)
        got = _launch(bits, G, reorder)
        _same(got, want[reorder], "G = %d, density %.2f" % (G, density))
        if density == 0.0:                       # all singletons: G clusters in index order
            assert got[3] == G and np.array_equal(got[2], np.arange(G)) and (got[1] == 1).all()
        if density == 1.0:                       # a count of G: 4096 needs the key's 13th bit
            assert got[3] == 1 and got[1][0] == G and (got[0] == 0).all()


def test_no_conformers_is_no_cluster():
    from agdiff_amd import _lib
    n = torch.full((1 + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    other = torch.full((TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    bits = torch.zeros(1, dtype=torch.int64, device="cuda")
    for reorder in (0, 1):
        _lib.call("agdiff_butina_cluster", bits, 0, reorder, other, other, other, n)
        assert n.cpu().tolist() == [0] + [SENTINEL] * TAIL and (other == SENTINEL).all()
        n[0] = SENTINEL


# ------------------------------------------------------------------------------------------------ 2. structured graphs
def test_hand_worked_graphs():
    adj = BR.graph(7, BR.SEVEN)
    leader, count, rank, n = _launch(BR.pack(adj), 7, False)
    assert leader.tolist() == [0, 0, 0, 0, 4, 4, 6] and count.tolist() == [4, 0, 0, 0, 2, 0, 1] and rank.tolist() == [0, 0, 0, 0, 1, 1, 2]
    assert n == 3
    leader, count, rank, n = _launch(BR.pack(adj), 7, True)
    assert leader.tolist() == [0, 0, 0, 0, 5, 5, 5] and count.tolist() == [4, 0, 0, 0, 0, 3, 0] and rank.tolist() == [0, 0, 0, 0, 1, 1, 1]
    assert n == 2
    G = 9
    for reorder in (False, True):
        leader, count, rank, n = _launch(BR.pack(np.eye(G, dtype=bool)), G, reorder)
        assert leader.tolist() == list(range(G)) and rank.tolist() == list(range(G)) and count.tolist() == [1] * G and n == G
        leader, count, rank, n = _launch(BR.pack(np.ones((G, G), dtype=bool)), G, reorder)
        assert leader.tolist() == [0] * G and rank.tolist() == [0] * G and count.tolist() == [G] + [0] * (G - 1) and n == 1
        two = BR.graph(6, [(0, 2), (2, 4), (0, 4), (1, 3), (3, 5), (1, 5)])
        leader, count, rank, n = _launch(BR.pack(two), 6, reorder)
        assert leader.tolist() == [0, 1, 0, 1, 0, 1] and rank.tolist() == [0, 1, 0, 1, 0, 1] and count.tolist() == [3, 3, 0, 0, 0, 0]
        star = BR.graph(G, [(G - 1, j) for j in range(G - 1)])
        leader, count, rank, n = _launch(BR.pack(star), G, reorder)
        assert leader.tolist() == [G - 1] * G and rank.tolist() == [0] * G and count.tolist() == [0] * (G - 1) + [G] and n == 1


@pytest.mark.parametrize("reorder", [False, True])
def test_equal_cliques_come_out_by_lowest_index(reorder):
    """13 cliques of 10, member i in clique i mod 13: every count ties, so the centroids are 0 .. 12 in that order"""
    G, K = 130, 13
    label = np.arange(G) % K
    adj = label[:, None] == label[None, :]
    leader, count, rank, n = _launch(BR.pack(adj), G, reorder)
    assert np.array_equal(leader, label) and np.array_equal(rank, label) and n == K
    assert count[:K].tolist() == [G // K] * K and not count[K:].any()
    _same((leader, count, rank, n), BR.butina(adj, reorder))


@pytest.mark.parametrize("reorder", [False, True])
def test_disjoint_pairs_take_half_as_many_iterations_as_conformers(reorder):
    """G = 4096, i paired with i + 2048: every count is 2 to the end, so the loop runs 2048 times -- the longest run there is,
    since a conformer without a neighbour is finished in the singleton pass"""
    G = 4096
    adj = BR.graph(G, [(i, i + G // 2) for i in range(G // 2)])
    leader, count, rank, n = _launch(BR.pack(adj), G, reorder)
    assert np.array_equal(leader, np.arange(G) % (G // 2)) and np.array_equal(rank, np.arange(G) % (G // 2)) and n == G // 2
    assert (count[:G // 2] == 2).all() and not count[G // 2:].any()
    odd = adj.copy()                                 # ... and with the last pair cut: two singletons after 2047 pairs
    odd[G // 2 - 1, G - 1] = odd[G - 1, G // 2 - 1] = False
    _same(_launch(BR.pack(odd), G, reorder), BR.butina(odd, reorder, running=True))


@pytest.mark.parametrize("reorder", [False, True])
def test_path_of_200(reorder):
    G = 200
    adj = BR.graph(G, [(i, i + 1) for i in range(G - 1)])
    got = _launch(BR.pack(adj), G, reorder)
    _same(got, BR.butina(adj, reorder))
    assert got[0][:3].tolist() == [1, 1, 1]                  # 1 is the first vertex with two neighbours
    if reorder:
        assert got[3] == 67 and got[0][:198].tolist() == [3 * (i // 3) + 1 for i in range(198)]


@pytest.mark.parametrize("reorder", [False, True])
def test_largest_count_in_the_last_lane_word(reorder):
    """G = 130: vertex 129 -- bit 1 of the third word, the last one a lane holds -- has the most neighbours"""
    G = 130
    adj = BR.random_graph(G, 0.05, seed=5).copy()
    hub = np.zeros(G, dtype=bool)
    hub[np.arange(0, G, 3)] = True
    adj[G - 1, hub] = adj[hub, G - 1] = True
    assert adj.sum(1).argmax() == G - 1 and (adj.sum(1) == adj.sum(1).max()).sum() == 1
    got = _launch(BR.pack(adj), G, reorder)
    _same(got, BR.butina(adj, reorder))
    assert got[0][G - 1] == G - 1 and got[2][G - 1] == 0 and got[1][G - 1] == adj[G - 1].sum()


# ------------------------------------------------------------------------------------------------ 3. padding, 4. diagonal
@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("G", [65, 130])
def test_padding_filled_with_ones_changes_nothing(G, reorder):
    for density in (0.0, 0.02, 0.5):
        adj, bits, want = _random_case(G, density)
        dirty = BR.pack(adj, garbage=True)
        assert not np.array_equal(dirty, bits)
        _same(_launch(dirty, G, reorder), want[reorder], density)


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("G", [1, 65, 130, 1000])
def test_missing_diagonal_is_taken_as_set(G, reorder):
    """(a finite run by construction: the outer loop is counted and the centroid leaves the live set whatever its own bit says)"""
    for density in (0.0, 0.02, 0.5):
        adj, bits, want = _random_case(G, density)
        bare = adj & ~np.eye(G, dtype=bool)
        _same(_launch(BR.pack(bare), G, reorder), want[reorder], density)


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("G", [65, 1000])
def test_asymmetric_matrix_still_gives_a_partition_inside_the_arrays(G, reorder):
    """The partition of an asymmetric matrix is unspecified, its bounds are not: the loop is counted, every index written comes out
    of the live set, and the counts are clamped when they are packed into the key.  _launch checks the ranges and the canary tail;
    what any run must still give is a partition -- every conformer under a centroid that leads itself, the sizes adding up to G."""
    rng = np.random.default_rng(G)
    for density in (0.02, 0.5):
        adj = rng.random((G, G)) < density                   # bit (i, j) and bit (j, i) drawn independently, no diagonal
        leader, count, rank, n = _launch(BR.pack(adj, garbage=True), G, reorder)
        cent = np.nonzero(leader == np.arange(G))[0]
        assert n == cent.size and np.array_equal(leader[leader], leader)
        assert np.array_equal(count, np.where(leader == np.arange(G), np.bincount(leader, minlength=G), 0)) and count.sum() == G
        assert np.array_equal(np.sort(rank[cent]), np.arange(n)) and np.array_equal(rank, rank[leader])
        others = leader != np.arange(G)
        assert adj[leader[others], np.nonzero(others)[0]].all()          # a member has its centroid's bit (c, j)


# ------------------------------------------------------------------------------------------------ 5. determinism, 6. limit
def test_two_launches_give_equal_tensors():
    from agdiff_amd.clusters import butina_cluster
    for G, density in ((1000, 0.02), (4096, 0.02), (4096, 0.5)):
        bits = torch.from_numpy(np.array(_random_case(G, density)[1])).cuda()
        for reorder in (False, True):
            a, b = butina_cluster(bits, G, reorder=reorder), butina_cluster(bits, G, reorder=reorder)
            assert all(x.dtype == torch.int32 and x.is_cuda for x in a)
            assert all(torch.equal(x, y) for x, y in zip(a, b))
            _same(tuple(x.cpu().numpy() for x in a[:3]) + (int(a[3].item()),), _random_case(G, density)[2][reorder])


def test_more_conformers_than_the_limit_are_refused_before_any_launch():
    from agdiff_amd import _lib
    from agdiff_amd.clusters import butina_cluster, cluster_conformers
    from agdiff_amd.ensemble import bits_pitch
    G = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1
    assert G == 4097
    bits = torch.zeros((G, bits_pitch(G) // 8), dtype=torch.int64, device="cuda")
    for reorder in (False, True):
        with pytest.raises(_lib.AgdiffLimitError):
            butina_cluster(bits, G, reorder=reorder)
    with pytest.raises(_lib.AgdiffLimitError):
        cluster_conformers({"atom_type": np.array([6, 6]), "pos_gen": np.zeros((G, 2, 3), np.float32)}, 0.5)


# ------------------------------------------------------------------------------------------------ 7. end to end
# (the construction of tests/test_hip_ensemble.py, restated)
GROUP4 = lambda m: np.stack([np.r_[a, b, np.arange(4, m)] for a in ([0, 1], [1, 0]) for b in ([2, 3], [3, 2])]).astype(np.int32)
SIZES = {(20, 4, 37): [16, 11, 7, 3], (45, 7, 150): [40, 33, 27, 21, 15, 9, 5]}


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _moved(rng, x):
    return x @ _rotation(rng).T + rng.normal(size=3)


def _relabel(x, heavy, perm):
    """the same structure with heavy atom k sitting where heavy atom perm[k] sat"""
    y = x.copy()
    y[heavy] = x[heavy][perm]
    return y


def _kabsch_align(x, target, sel):
    """float64 Kabsch (SVD, proper rotation) of x onto target over the atoms `sel`, applied to every atom"""
    x, target = np.asarray(x, np.float64), np.asarray(target, np.float64)
    cx, ct = x[sel].mean(0), target[sel].mean(0)
    H = (x[sel] - cx).T @ (target[sel] - ct)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    R = (U @ np.diag([1.0, 1.0, d]) @ Vt).T
    return (x - cx) @ R.T + ct


@functools.lru_cache(maxsize=None)
def _families(n, K, G):
    """(item, label [G], gen fp32 [G, n, 3], heavy): K tight families of distinct sizes, every member moved rigidly and relabelled
    by an element of the molecule's group"""
    rng = np.random.default_rng(7 * n + G)
    at = np.where(rng.random(n) < 0.5, 1, rng.choice([6, 7, 8], size=n))
    at[:4] = 6                                       # (the four atoms the group acts on)
    heavy = np.nonzero(at != 1)[0]
    perms = GROUP4(heavy.size)
    sizes = SIZES[(n, K, G)]
    assert len(sizes) == K and sum(sizes) == G and len(set(sizes)) == K
    centres = [rng.normal(size=(n, 3)) * 1.5 for _ in range(K)]
    label = rng.permutation(np.repeat(np.arange(K), sizes))
    gen = np.stack([_moved(rng, _relabel(centres[c] + 0.03 * rng.normal(size=(n, 3)), heavy, perms[rng.integers(4)]))
                    for c in label]).astype(np.float32)
    for a in (at, label):
        a.setflags(write=False)
    return {"atom_type": at, "pos_gen": gen, "perms": perms}, label, gen, heavy


def _check_families(res, label, gen, thr, matrix, first, valid=None):
    """the result against the planted families: `first` [K] the expected centroid of every family (-1: the whole family is masked
    out by `valid`); the families are cliques, so every member ties and the lowest index leads.  population: count / clustered
    conformers in fp32, by a division or by the reciprocal and a product -- two roundings at most, 2 ulp of 1.0 = 2.4e-7."""
    G = label.shape[0]
    shown = np.ones(G, dtype=bool) if valid is None else valid
    sizes = np.array([(shown & (label == c)).sum() for c in range(len(first))])
    order = [c for c in np.argsort(-sizes, kind="stable") if sizes[c] > 0]
    K = len(order)
    for key, dtype, shape in (("centroids", torch.int32, (K,)), ("leader", torch.int32, (G,)), ("cluster", torch.int32, (G,)),
                              ("count", torch.int32, (K,)), ("population", torch.float32, (K,)), ("dist", torch.float32, (G,)),
                              ("pos", torch.float32, (K, gen.shape[1], 3))):
        assert res[key].dtype == dtype and tuple(res[key].shape) == shape and res[key].is_cuda, key
    assert res["centroids"].cpu().tolist() == [first[c] for c in order]
    assert res["count"].cpu().tolist() == [sizes[c] for c in order] and (np.diff(res["count"].cpu().numpy()) < 0).all()
    leader, cluster = res["leader"].cpu().numpy(), res["cluster"].cpu().numpy()
    place = {c: k for k, c in enumerate(order)}
    assert np.array_equal(leader[shown], np.array([first[c] for c in label])[shown]) and (leader[~shown] == -1).all()
    assert np.array_equal(cluster[shown], np.array([place.get(c, -1) for c in label])[shown]) and (cluster[~shown] == -1).all()
    pop = res["population"].cpu().numpy()
    assert np.abs(pop.astype(np.float64) - res["count"].cpu().numpy() / float(shown.sum())).max() <= 2.4e-7
    assert abs(float(pop.astype(np.float64).sum()) - 1.0) <= len(order) * 2.4e-7
    dist = res["dist"].cpu().numpy()
    assert np.isnan(dist[~shown]).all() and (dist[shown] <= thr).all() and (dist[leader[shown]] == 0).all()
    assert np.array_equal(dist[shown], matrix[leader[shown], np.nonzero(shown)[0]])


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("n,K,G", sorted(SIZES))
def test_rmsd_clusters_are_the_planted_families(n, K, G, reorder):
    from agdiff_amd.clusters import cluster_conformers
    from agdiff_amd.ensemble import self_rmsd_matrix
    item, label, gen, heavy = _families(n, K, G)
    thr = 0.5
    matrix = self_rmsd_matrix(item).cpu().numpy()
    off, same = matrix[np.triu_indices(G, 1)], (label[:, None] == label[None, :])[np.triu_indices(G, 1)]
    print("families n=%d: largest intra %.3f, smallest inter %.3f" % (n, off[same].max(), off[~same].min()))
    assert np.abs(off - thr).min() >= 0.1 and off[same].max() < thr < off[~same].min()       # nothing hinges on rounding
    first = np.array([np.nonzero(label == c)[0][0] for c in range(K)])
    res = cluster_conformers(item, thr, reorder=reorder, align=True)
    _check_families(res, label, gen, thr, matrix, first)
    cent = res["centroids"].cpu().numpy()
    assert torch.equal(res["pos"][0].cpu(), torch.from_numpy(gen[cent[0]]))                   # bit for bit
    want = np.stack([_kabsch_align(gen[c], gen[cent[0]], heavy) for c in cent])
    dev = np.abs(res["pos"].cpu().numpy() - want).max()
    print("aligned centroids n=%d: max |aligned - float64 Kabsch| = %.3e Angstrom" % (n, dev))
    assert dev <= ALIGN_ATOL
    raw = cluster_conformers(item, thr, reorder=reorder, align=False, distances=False)
    assert "dist" not in raw and torch.equal(raw["pos"].cpu(), torch.from_numpy(gen[cent]))
    assert all(torch.equal(raw[k], res[k]) for k in ("centroids", "leader", "cluster", "count", "population"))
    # the identity mapping alone does not see the relabelled members as one family
    plain = cluster_conformers({"atom_type": item["atom_type"], "pos_gen": gen}, thr, reorder=reorder, align=False)
    assert plain["centroids"].shape[0] > K


def test_valid_mask_takes_conformers_out_and_keeps_the_items_own_indices():
    from agdiff_amd.clusters import cluster_conformers
    from agdiff_amd.ensemble import self_rmsd_matrix
    n, K, G = 20, 4, 37
    item, label, gen, heavy = _families(n, K, G)
    matrix = self_rmsd_matrix(item).cpu().numpy()
    first = np.array([np.nonzero(label == c)[0][0] for c in range(K)])
    valid = np.ones(G, dtype=bool)
    valid[label == 2] = False                        # one whole family ...
    valid[first[0]] = False                          # ... and the member of another that would have led it
    want_first = first.copy()
    want_first[2] = -1
    want_first[0] = np.nonzero((label == 0) & valid)[0][0]
    for reorder in (False, True):
        for mask in (valid, torch.from_numpy(valid).cuda()):
            res = cluster_conformers(item, 0.5, reorder=reorder, valid=mask)
            assert np.array_equal(res["leader"].cpu().numpy() == -1, ~valid)
            assert np.array_equal(res["cluster"].cpu().numpy() == -1, ~valid)
            _check_families(res, label, gen, 0.5, matrix, want_first, valid=valid)
            assert res["count"].cpu().tolist() == [15, 11, 3]
    none = cluster_conformers(item, 0.5, valid=np.zeros(G, dtype=bool))
    assert all(tuple(none[k].shape) == (0,) for k in ("centroids", "count", "population")) and tuple(none["pos"].shape) == (0, n, 3)
    assert (none["leader"] == -1).all() and (none["cluster"] == -1).all() and bool(torch.isnan(none["dist"]).all())
    assert none["leader"].shape == (G,) and none["dist"].shape == (G,)


@pytest.mark.parametrize("reorder", [False, True])
def test_tfd_clusters_are_the_planted_rotamer_families(reorder):
    """pentane, two rotatable bonds: families at (anti, anti), (anti, gauche+), (gauche+, gauche+), (gauche-, gauche-), 0.03 rad of
    noise; a third of the members listed from the chain's other end, which swaps the two dihedrals and is the same conformer.
    Neighbouring families differ by 120 degrees in one dihedral at least: TFD >= 1/3 less the noise, against a threshold of 0.1."""
    from agdiff_amd.clusters import cluster_conformers
    from agdiff_amd.torsions import tfd_self
    rng = np.random.default_rng(17)
    g = np.pi / 3
    rotamers, sizes = [(np.pi, np.pi), (np.pi, g), (g, g), (-g, -g)], [9, 6, 4, 2]
    label = rng.permutation(np.repeat(np.arange(4), sizes))
    G = label.shape[0]
    gen = []
    for c in label:
        x = TR.chain_positions(np.array(rotamers[c]) + 0.03 * rng.normal(size=2))
        gen.append(_moved(rng, x[::-1] if rng.random() < 1 / 3 else x))
    gen = np.stack(gen).astype(np.float32)
    at, bi, bt = TR.alkane(5)
    item = dict(atom_type=at, bond_index=bi, bond_type=bt, pos_gen=gen)
    thr = 0.1
    matrix = tfd_self(item)[0].cpu().numpy()
    off, same = matrix[np.triu_indices(G, 1)], (label[:, None] == label[None, :])[np.triu_indices(G, 1)]
    print("rotamer families: largest intra %.3f, smallest inter %.3f" % (off[same].max(), off[~same].min()))
    assert np.abs(off - thr).min() >= 0.05 and off[same].max() < thr < off[~same].min()
    first = np.array([np.nonzero(label == c)[0][0] for c in range(4)])
    res = cluster_conformers(item, thr, metric="tfd", reorder=reorder, align=True)
    _check_families(res, label, gen, thr, matrix, first)
    assert res["count"].cpu().tolist() == sizes
    cent = res["centroids"].cpu().numpy()
    assert torch.equal(res["pos"][0].cpu(), torch.from_numpy(gen[cent[0]]))
    want = np.stack([_kabsch_align(gen[c], gen[cent[0]], np.arange(5)) for c in cent])
    assert np.abs(res["pos"].cpu().numpy() - want).max() <= ALIGN_ATOL


@pytest.mark.parametrize("reorder", [False, True])
def test_a_conformer_with_a_nan_is_a_singleton_and_changes_nobody_elses_cluster(reorder):
    """cluster_conformers does not mask a conformer with a coordinate that is not finite: it reaches the matrix, where by the header's
    rule it is +inf from everything (tests/test_hip_rmsd_kernels.py, section 5), so it is a cluster of its own, the last one, and the
    others come out as they do from the item without it.  Two planted families (0.03 of noise, centres 1.5 apart, threshold 0.5),
    conformer 3 broken in a heavy atom; with and without a `valid` mask that removes conformer 0, the first centroid.  The broken
    conformer's own `dist` reads the matrix diagonal and is not looked at."""
    from agdiff_amd.clusters import cluster_conformers
    rng = np.random.default_rng(31)
    n, G, bad, thr = 8, 6, 3, 0.5
    at = np.array([6, 6, 7, 6, 8, 1, 1, 6])
    label = np.array([0, 1, 0, 0, 1, 0])
    centres = rng.normal(size=(2, n, 3)) * 1.5
    gen = np.stack([_moved(rng, centres[c] + 0.03 * rng.normal(size=(n, 3))) for c in label]).astype(np.float32)
    gen[bad, 2, 1] = np.nan
    rest = np.delete(np.arange(G), bad)
    masked = np.ones(G, dtype=bool)
    masked[0] = False
    for valid, cent, leader, cluster, count in ((None, [0, 1, 3], [0, 1, 0, 3, 1, 0], [0, 1, 0, 2, 1, 0], [3, 2, 1]),
                                                (masked, [1, 2, 3], [-1, 1, 2, 3, 1, 2], [-1, 0, 1, 2, 0, 1], [2, 2, 1])):
        res = cluster_conformers({"atom_type": at, "pos_gen": gen}, thr, reorder=reorder, valid=valid)
        assert res["centroids"].cpu().tolist() == cent and res["leader"].cpu().tolist() == leader
        assert res["cluster"].cpu().tolist() == cluster and res["count"].cpu().tolist() == count
        ref = cluster_conformers({"atom_type": at, "pos_gen": gen[rest]}, thr, reorder=reorder, valid=None if valid is None else valid[rest])
        own = lambda x: np.where(x < 0, -1, rest[np.maximum(x, 0)])         # the smaller item's indices in this one's
        assert np.array_equal(own(ref["centroids"].cpu().numpy()), np.array(cent[:2]))
        assert np.array_equal(own(ref["leader"].cpu().numpy()), np.array(leader)[rest])
        assert np.array_equal(ref["cluster"].cpu().numpy(), np.array(cluster)[rest])
        assert ref["count"].cpu().tolist() == count[:2]
        got, want = res["dist"].cpu()[rest], ref["dist"].cpu()              # NaN where masked, else bit for bit
        shown = torch.from_numpy(np.ones(G, dtype=bool) if valid is None else valid)[rest]
        assert torch.equal(torch.isnan(got), ~shown) and torch.equal(torch.isnan(want), ~shown)
        assert torch.equal(got[shown], want[shown]) and bool((got[shown] <= thr).all())
        assert torch.equal(res["pos"][:2], ref["pos"])                      # superposed on the same first centroid


# ------------------------------------------------------------------------------------------------ 8. the command line
def seven_pattern_conformers(rng):
    """(atom_type, bonds as (i, j, type), gen fp32 [7, n, 3], threshold): seven conformers of a ten-atom chain whose adjacency under
    the threshold is the 7-vertex graph BR.SEVEN.  Conformer i = base + 0.1 (u_i D1 + v_i D2) with two displacement fields of unit
    RMS, orthogonal to each other and free of any translation or rotation, so the RMSD of i and j is 0.1 |(u, v)_i - (u, v)_j| up
    to second order; the plane points are 0.85 - 0.9 apart along the edges and >= 1.2 apart otherwise; the threshold is 0.105.
    The chain's atom types read differently from its two ends: no relabelling but the identity."""
    at = np.array([6, 6, 7, 6, 8, 6, 6, 7, 7, 6])
    n = at.shape[0]
    bonds = [(i, i + 1, 1) for i in range(n - 1)]
    base = TR.chain_positions(rng.uniform(-np.pi, np.pi, size=n - 3))
    base -= base.mean(0)
    rigid = [np.tile(e, (n, 1)) for e in np.eye(3)] + [np.cross(e, base) for e in np.eye(3)]
    fields = []
    for _ in range(2):
        d = rng.normal(size=(n, 3))
        for _ in range(2):
            for f in rigid + fields:
                d -= f * ((d * f).sum() / (f * f).sum())
        fields.append(d * np.sqrt(n / (d * d).sum()))
    plane = np.array([(0, 0), (0.6, 0.6), (0.6, -0.6), (-0.9, 0), (1.2, 0), (2.1, 0), (3.0, 0)])
    gen = np.stack([_moved(rng, base + 0.1 * (u * fields[0] + v * fields[1])) for u, v in plane]).astype(np.float32)
    return at, bonds, gen, 0.105


def test_command_line_writes_every_key_and_static_changes_the_seven_pattern(tmp_path, capsys):
    from agdiff_amd import clusters, driver, synth
    from agdiff_amd.ensemble import self_rmsd_matrix
    rng = np.random.default_rng(9)
    at, bonds, gen7, thr = seven_pattern_conformers(rng)
    _, bi, bt = TR.graph(at, bonds)
    mols, gens = [dict(atom_type=at, edge_index=bi, edge_type=bt, num_refs=4, name="seven")], [gen7]
    matrix = self_rmsd_matrix(dict(atom_type=at, edge_index=bi, edge_type=bt, pos_gen=gen7)).cpu().numpy()
    assert np.array_equal(matrix <= thr, BR.graph(7, BR.SEVEN)) and np.abs(matrix - thr)[~np.eye(7, dtype=bool)].min() > 0.01
    for i, (n, G) in enumerate(((15, 7), (12, 5))):
        a, r, c, ty = synth.random_molecule(rng, n)
        mols.append(dict(atom_type=a, edge_index=np.stack([r, c]), edge_type=ty, num_refs=3, name="m%d" % (i + 1)))
        base = rng.normal(size=(2, n, 3)) * 1.5
        gens.append(np.stack([_moved(rng, base[k % 2] + 0.02 * rng.normal(size=(n, 3))) for k in range(G)]).astype(np.float32))
    driver.save_testset(str(tmp_path / "test.npz"), mols)
    np.savez(str(tmp_path / "samples_all.npz"), **{"pos_gen_%d" % i: g for i, g in enumerate(gens)})
    base = ["--samples", str(tmp_path / "samples_all.npz"), "--testset", str(tmp_path / "test.npz"), "--rms", str(thr), "--align"]
    out = clusters.main(base + ["--out", str(tmp_path / "clusters.npz")])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and "19 conformers" in line[0] and "6 clusters" in line[0]
    z = np.load(str(tmp_path / "clusters.npz"))
    keys = ("centroid", "cluster", "leader", "count", "population", "dist", "pos", "name")
    assert set(z.files) == {"%s_%d" % (k, i) for k in keys for i in range(3)} == set(out)
    for i, g in enumerate(gens):
        G, n = g.shape[0], g.shape[1]
        K = z["centroid_%d" % i].shape[0]
        for k, dtype, shape in (("centroid", np.int32, (K,)), ("cluster", np.int32, (G,)), ("leader", np.int32, (G,)),
                                ("count", np.int32, (K,)), ("population", np.float32, (K,)), ("dist", np.float32, (G,)),
                                ("pos", np.float32, (K, n, 3))):
            assert z["%s_%d" % (k, i)].dtype == dtype and z["%s_%d" % (k, i)].shape == shape, (k, i)
            assert np.array_equal(z["%s_%d" % (k, i)], out["%s_%d" % (k, i)])
        assert str(z["name_%d" % i]) == mols[i]["name"]
        assert np.array_equal(z["pos_%d" % i][0], g[z["centroid_%d" % i][0]])
        assert np.array_equal(z["centroid_%d" % i][z["cluster_%d" % i]], z["leader_%d" % i])
    assert z["leader_0"].tolist() == [0, 0, 0, 0, 5, 5, 5] and z["centroid_0"].tolist() == [0, 5] and z["count_0"].tolist() == [4, 3]
    assert z["leader_1"].tolist() == [0, 1, 0, 1, 0, 1, 0] and z["count_1"].tolist() == [4, 3]
    assert z["leader_2"].tolist() == [0, 1, 0, 1, 0] and np.abs(z["population_2"] - [0.6, 0.4]).max() <= 2.4e-7
    clusters.main(base + ["--static", "--out", str(tmp_path / "static.npz")])
    s = np.load(str(tmp_path / "static.npz"))
    assert s["leader_0"].tolist() == [0, 0, 0, 0, 4, 4, 6] and s["centroid_0"].tolist() == [0, 4, 6] and s["count_0"].tolist() == [4, 2, 1]
    assert s["cluster_0"].tolist() == [0, 0, 0, 0, 1, 1, 2]
    for i in (1, 2):
        assert all(np.array_equal(s["%s_%d" % (k, i)], z["%s_%d" % (k, i)]) for k in keys)
    # --drop-invalid writes valid_<i> next to the rest, as the ensemble command line does
    more = clusters.main(base + ["--drop-invalid", "--out", str(tmp_path / "checked.npz")])
    assert all("valid_%d" % i in more and more["valid_%d" % i].dtype == np.int8 for i in range(3))
    for i in range(3):
        assert np.array_equal(more["leader_%d" % i] == -1, more["valid_%d" % i] == 0)
