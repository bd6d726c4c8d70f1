"""GPU (MI355X): k-medoids (agdiff_amd.medoids; csrc/eval.hip: k_kmed_*) against the numpy restatement of its rule
(tests/kmedoids_ref.py) on the same float32 matrix -- integers equal, floats and doubles bit-equal, NaN at the same places, n_iter
and status included -- and end to end through medoid_conformers and the command line.

Every sum the walk makes is a sum of integers (the matrix entries on a 2^-28 grid) and every float it writes is a copy of a matrix
entry or such a sum divided by 2^28, so every comparison with the restatement is exact.  The one tolerance is ALIGN_ATOL, for the
superposed medoids against a float64 Kabsch of the same fp32 inputs: the bar that tests/test_hip_clusters.py carries for
agdiff_align_conformers, the same kernel under the same bar; nothing new is measured here."""
import functools

import numpy as np
import pytest
import torch

import kmedoids_ref as KR
import rings_ref as RR
import tfd_ref as TR
from test_hip_clusters import ALIGN_ATOL, _families, _kabsch_align, _moved, seven_pattern_conformers

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL, FSENTINEL, TAIL = -7, -777.0, 64           # (no output is negative but the -1 of medoids / labels)


def _launch(dist, G, init, max_iter=32):
    """agdiff_kmedoids on a device tensor [G, G] (or a numpy matrix), its eight arrays filled with a sentinel and followed by a
    canary tail, the scratch followed by one too: every entry must have been written, the tails must be as they were.  The result
    in the restatement's form."""
    from agdiff_amd import _lib
    dev = dist if torch.is_tensor(dist) else torch.from_numpy(np.array(dist, dtype=F32)).cuda()
    K = len(init)
    seeds = torch.tensor(list(init), dtype=torch.int32, device="cuda")
    full = lambda m, v, dtype: torch.full((m + TAIL,), v, dtype=dtype, device="cuda")
    medoids, labels, size, n_iter, status = (full(m, SENTINEL, torch.int32) for m in (K, G, K, 1, 1))
    near = full(G, FSENTINEL, torch.float32)
    within, cost = full(K, FSENTINEL, torch.float64), full(1, FSENTINEL, torch.float64)
    words = _lib.DEFINES["AGDIFF_KMEDOIDS_WORK_BYTES"] // 8
    work = full(words, SENTINEL, torch.int64)
    _lib.call("agdiff_kmedoids", dev, G, K, seeds, int(max_iter), medoids, labels, near, size, within, cost, n_iter, status, work)
    assert (work[words:] == SENTINEL).all() and seeds.cpu().tolist() == list(init)
    out = []
    for a, m, s in ((medoids, K, SENTINEL), (labels, G, SENTINEL), (near, G, FSENTINEL), (size, K, SENTINEL), (within, K, FSENTINEL),
                    (cost, 1, FSENTINEL), (n_iter, 1, SENTINEL), (status, 1, SENTINEL)):
        a = a.cpu().numpy()
        assert (a[m:] == s).all() and not (a[:m] == s).any()
        out.append(a[:m])
    medoids, labels, near, size, within, cost, n_iter, status = out
    assert ((medoids >= -1) & (medoids < G)).all() and ((labels >= -1) & (labels < K)).all() and status[0] in (0, 1, 2)
    return medoids, labels, near, size, within, cost[0], int(n_iter[0]), int(status[0])


@functools.lru_cache(maxsize=None)
def _case(name, *args):
    """(matrix, its fixed-point image, the same matrix on the device) of a named structured matrix -- made once, left unchanged"""
    d = getattr(KR, name)(*args) if name != "metric" else KR.random_metric(args[0], seed=args[0])
    d.setflags(write=False)
    q = KR.Q(d)
    q.setflags(write=False)
    return d, q, torch.from_numpy(np.array(d)).cuda()


def _both(case, init, max_iter=32):
    d, q, dev = case
    trace = []
    want = KR.kmedoids(d, init, max_iter=max_iter, trace=trace, q=q)
    got = _launch(dev, d.shape[0], init, max_iter=max_iter)
    assert KR.same(got, want), "G = %d, init = %s ..., max_iter = %d: got %s, want %s" % (
        d.shape[0], list(init)[:8], max_iter, (got[0][:8], got[3][:8], got[5:]), (want[0][:8], want[3][:8], want[5:]))
    return got, trace


# ------------------------------------------------------------------------------------------------ 1. the kernels against the rule
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096]


@pytest.mark.parametrize("G, K", [(G, K) for G in SIZES for K in sorted({1, min(7, G), min(100, G)} | ({G} if G <= 257 else set()))])
def test_kernels_equal_the_restated_rule(G, K):
    """across a wave, a workgroup of the assign (64 columns) and of the costs (4 rows), odd sizes and the limit; the first K, the
    last K and the restatement's MaxMin picks as seeds.  On the CPU all of these converge within 11 updates."""
    case = _case("metric", G)
    for init in (list(range(K)), list(range(G - K, G)), KR.maxmin(case[0], K)[0].tolist()):
        got, trace = _both(case, init)
        assert got[7] == 0 and got[6] <= 11
        if K == G:                                           # every conformer is its own medoid: one update
            assert got[6] == 1 and got[5] == 0 and got[0].tolist() == init and got[3].tolist() == [1] * G
    KR.check_invariants(case[0], init, got, trace)


def test_two_launches_give_equal_bytes_through_the_wrapper():
    from agdiff_amd.medoids import kmedoids
    for G, K in ((1000, 100), (4096, 10)):
        d, q, dev = _case("metric", G)
        init = torch.arange(K, dtype=torch.int32, device="cuda")
        a, b = kmedoids(dev, G, init), kmedoids(dev, G, init)
        for x, y, dtype, m in zip(a, b, (torch.int32, torch.int32, torch.float32, torch.int32, torch.float64, torch.float64,
                                        torch.int32, torch.int32), (K, G, G, K, K, 1, 1, 1)):
            assert x.dtype == dtype and tuple(x.shape) == (m,) and x.is_cuda
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        assert KR.same([t.cpu().numpy() for t in a[:6]] + [int(a[6]), int(a[7])], KR.kmedoids(d, list(range(K)), q=q))


# ------------------------------------------------------------------------------------------------ 2. ties and long walks
@pytest.mark.parametrize("name, args, K", [("line", (65,), 3), ("line", (1025,), 3)]
                         + [("lattice", shape, K) for shape in ((33, 31), (65, 63)) for K in (3, 7, 40)])
def test_ties_and_long_walks(name, args, K):
    """integer distances: nearly every arg-min is a tie, and from seeds at one end the medoids walk a long way"""
    case = _case(name, *args)
    G = case[0].shape[0]
    for init in (list(range(K)), list(range(G - K, G))):
        got, trace = _both(case, init)
        assert got[7] == 0 and got[6] >= 4
        KR.check_invariants(case[0], init, got, trace)


@pytest.mark.parametrize("G", [65, 257, 1025])
def test_small_values_equal_and_zero_matrices(G):
    for K in (1, 7, 40):
        for seed in (0, 1):
            d = KR.small_values(G, seed=G + seed)
            _both((d, None, torch.from_numpy(d).cuda()), list(range(K)))
            _both((d, None, torch.from_numpy(d).cuda()), list(range(G - K, G)))
        equal = np.full((G, G), F32(2.5))
        got, _ = _both((equal, None, torch.from_numpy(equal).cuda()), list(range(G - K, G)))
        assert got[6] == 1 and got[3].tolist() == [G - K + 1] + [1] * (K - 1)
        zero = np.zeros((G, G), F32)
        got, _ = _both((zero, None, torch.from_numpy(zero).cuda()), list(range(1, K + 1)))
        # everybody but the seeds goes to rank 0, every cost is 0 and the incumbents stay: one update
        assert got[6] == 1 and got[7] == 0 and got[0].tolist() == list(range(1, K + 1)) and got[3].tolist() == [G - K + 1] + [1] * (K - 1)
        assert got[5] == 0 and not got[2].any()


@pytest.mark.parametrize("name, args, want", [("line", (2,), {1: 1, 0: 0}), ("line", (4,), {0: 1, 3: 1}),
                                              ("line", (65,), {0: 32, 64: 32, 31: 32, 32: 32})])
def test_hand_worked_anchors(name, args, want):
    for seed, end in want.items():
        got, _ = _both(_case(name, *args), [seed])
        assert got[0].tolist() == [end] and got[6] == (1 if seed == end else 2)


# ------------------------------------------------------------------------------------------------ 3. the iteration limit
@pytest.mark.parametrize("max_iter", [1, 2, 64])
def test_iteration_limit(max_iter):
    """line(1025) from the first 7: the restatement has not converged after 64 updates.  The labels belong to the returned medoids."""
    case = _case("line", 1025)
    got, trace = _both(case, list(range(7)), max_iter=max_iter)
    assert got[7] == 1 and got[6] == max_iter
    KR.check_invariants(case[0], list(range(7)), got, trace)


def test_the_update_that_changes_nothing_is_counted():
    case = _case("line", 1025)
    full, _ = _both(case, list(range(7)), max_iter=128)
    assert full[7] == 0 and 64 < full[6] <= 128
    again, _ = _both(case, list(range(7)), max_iter=full[6])
    assert KR.same(again, full)
    short, _ = _both(case, list(range(7)), max_iter=full[6] - 1)
    assert short[7] == 1 and KR.same(short[:6], full[:6])


# ------------------------------------------------------------------------------------------------ 4. eligibility and bad entries
@pytest.mark.parametrize("G", [65, 257, 1025])
def test_ineligible_conformers_and_bad_entries(G):
    base = _case("metric", G)[0]
    bad = sorted({1, G // 3, G - 1, 64} & set(range(1, G)))
    d = KR.with_inf(base, bad)
    ok = [j for j in range(G) if j not in bad]
    for init in ([0], ok[:7], ok[-7:], KR.maxmin(d, 7)[0].tolist()):
        got, trace = _both((d, None, torch.from_numpy(d).cuda()), init)
        assert (got[1][bad] == -1).all() and np.isnan(got[2][bad]).all() and got[3].sum() == G - len(bad)
        KR.check_invariants(d, init, got, trace)
    for value in (np.nan, -1.0, 5000.0, np.inf, -np.inf):    # an eligible pair's bad entry counts as the cap, and near copies it
        e = np.array(base)
        e[5, 6] = e[6, 5] = e[ok[-1], ok[-2]] = e[7, 0] = value
        for init in ([0, 5], [5, 0, ok[-1]], ok[:7]):
            got, _ = _both((e, None, torch.from_numpy(e).cuda()), init)
            if init[0] == 5:                                 # row 5 decides: 6 is out
                assert got[1][6] == -1
    capped = np.array(base)
    capped[5, 6] = capped[6, 5] = 4096.0
    _both((capped, None, torch.from_numpy(capped).cuda()), [0, 5])
    at_cap = np.array(base)
    at_cap[0, 3] = at_cap[3, 0] = np.nextafter(F32(4096), F32(np.inf))      # just above the cap: 3 is out when 0 leads
    got, _ = _both((at_cap, None, torch.from_numpy(at_cap).cuda()), [0, 5])
    assert got[1][3] == -1


@pytest.mark.parametrize("G", [64, 257])
def test_minus_zero_entries_are_zeros(G):
    d = np.array(_case("metric", G)[0])
    rng = np.random.default_rng(G)
    dup = rng.choice(G, size=G // 4, replace=False)
    d[dup[:, None], dup[None, :]] = -0.0                     # a clique of duplicates at distance -0.0, diagonal included
    pos = np.where(d == 0, F32(0), d)
    for init in ([int(dup[0])], [0, 1, 2], sorted(dup.tolist())[:5]):
        got, _ = _both((d, None, torch.from_numpy(d).cuda()), init)
        assert KR.same(got, KR.kmedoids(pos, init)) and not np.signbit(got[2]).any()


@pytest.mark.parametrize("G", [63, 1023, 1025])
def test_matrix_one_float_into_its_allocation(G):
    """dist needs 4-byte alignment only; with G odd no row of it is 8-byte aligned"""
    d, q, _ = _case("metric", G)
    buf = torch.full((G * G + 2,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    off = buf[1:1 + G * G].view(G, G)
    off.copy_(torch.from_numpy(np.array(d)))
    assert off.data_ptr() % 8 == 4 and off.is_contiguous()
    for init in ([G - 1], list(range(7)), list(range(G - 40, G))):
        _both((d, q, off), init)


# ------------------------------------------------------------------------------------------------ 5. bad seeds, nothing to do
@pytest.mark.parametrize("G", [9, 300])
def test_bad_seeds_give_status_two(G):
    """ordinary inputs with a defined result: the kernel checks the seeds and fills every output"""
    d = KR.with_inf(_case("metric", G)[0], [4])
    dev = torch.from_numpy(d).cuda()
    for init in ([0, 0], [1, 2, 1], [-1], [0, G], [G], [0, 4], [4, 0], [3, -1], [0, 1 << 30], list(range(5, 9)) + [5]):
        got, _ = _both((d, None, dev), init)
        assert got[7] == 2 and got[6] == 0 and got[5] == 0 and (got[0] == -1).all() and (got[1] == -1).all() and np.isnan(got[2]).all()
        assert not got[3].any() and not got[4].any()
    got, _ = _both((d, None, dev), [0, 3])
    assert got[7] == 0


def test_no_conformers_is_no_launch():
    from agdiff_amd import _lib
    n_iter, status = (torch.full((1 + TAIL,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2))
    cost = torch.full((1 + TAIL,), FSENTINEL, dtype=torch.float64, device="cuda")
    ints = torch.full((TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    floats = torch.full((TAIL,), FSENTINEL, dtype=torch.float32, device="cuda")
    doubles = torch.full((TAIL,), FSENTINEL, dtype=torch.float64, device="cuda")
    work = torch.full((TAIL,), SENTINEL, dtype=torch.int64, device="cuda")
    dist = torch.zeros(1, dtype=torch.float32, device="cuda")
    _lib.call("agdiff_kmedoids", dist, 0, 1, ints, 32, ints, ints, floats, ints, doubles, cost, n_iter, status, work)
    assert n_iter.cpu().tolist() == [0] + [SENTINEL] * TAIL and status.cpu().tolist() == [0] + [SENTINEL] * TAIL
    assert cost.cpu().tolist() == [0.0] + [FSENTINEL] * TAIL
    assert (ints == SENTINEL).all() and (floats == FSENTINEL).all() and (doubles == FSENTINEL).all() and (work == SENTINEL).all()


def test_wrapper_refuses_what_the_header_refuses():
    from agdiff_amd import _lib
    from agdiff_amd.medoids import kmedoids, medoid_conformers
    G = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.AgdiffLimitError):
        kmedoids(torch.zeros((G, G), dtype=torch.float32, device="cuda"), G, one)
    with pytest.raises(_lib.AgdiffLimitError):
        medoid_conformers({"atom_type": np.array([6, 6]), "pos_gen": np.zeros((G, 2, 3), np.float32)}, 10)
    small = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    for bad in (lambda: kmedoids(torch.zeros((4, 5), dtype=torch.float32, device="cuda"), 4, one),
                lambda: kmedoids(small.double(), 4, one), lambda: kmedoids(small, 4, one.long()), lambda: kmedoids(small, 4, one.cpu()),
                lambda: kmedoids(small, 4, one, max_iter=0), lambda: kmedoids(small, 4, one, max_iter=129)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.AgdiffHipError):
        kmedoids(small, 4, torch.zeros(5, dtype=torch.int32, device="cuda"))              # K > G


# ------------------------------------------------------------------------------------------------ 6. end to end
def _check_result(res, want, G, n_atoms, sel=None):
    """a medoid_conformers result against the restatement run on the matrix of the usable conformers (`sel`: their indices in the
    item)"""
    med, labels, near, size, within, cost, n_iter, status = want
    K = len(med)
    sel = np.arange(G) if sel is None else np.asarray(sel)
    for key, dtype, shape in (("medoids", torch.int32, (K,)), ("labels", torch.int32, (G,)), ("near", torch.float32, (G,)),
                              ("count", torch.int32, (K,)), ("population", torch.float32, (K,)), ("within", torch.float64, (K,)),
                              ("pos", torch.float32, (K, n_atoms, 3))):
        assert res[key].dtype == dtype and tuple(res[key].shape) == shape and res[key].is_cuda, key
    assert isinstance(res["cost"], float) and res["cost"] == cost and res["iters"] == n_iter and res["converged"] is (status == 0)
    assert res["medoids"].cpu().tolist() == sel[med].tolist()
    full_labels, full_near = np.full(G, -1, dtype=np.int32), np.full(G, np.nan, dtype=F32)
    full_labels[sel], full_near[sel] = labels, near
    assert KR.same((res["labels"].cpu().numpy(), res["near"].cpu().numpy(), res["count"].cpu().numpy(), res["within"].cpu().numpy()),
                   (full_labels, full_near, size, within))
    assert KR.same((res["population"].cpu().numpy(),), (size.astype(F32) / F32(sel.size),))
    assert int(res["count"].sum()) == sel.size


def _seven(rng=None):
    at, bonds, gen, _ = seven_pattern_conformers(np.random.default_rng(9) if rng is None else rng)
    _, bi, bt = TR.graph(at, bonds)
    return dict(atom_type=at, bond_index=bi, bond_type=bt, pos_gen=gen), gen


@pytest.mark.parametrize("metric, rings", [("rmsd", False), ("tfd", False), ("tfd", True)])
def test_seven_pattern_equals_the_restatement_on_the_devices_matrix(metric, rings):
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.medoids import medoid_conformers
    from agdiff_amd.picks import pick_conformers
    from agdiff_amd.torsions import tfd_self
    item, gen = _seven()
    G, n = gen.shape[0], gen.shape[1]
    matrix = (self_rmsd_matrix(item) if metric == "rmsd" else tfd_self(item, rings=rings)[0]).cpu().numpy()
    kw = dict(metric=metric, tfd_rings=rings, align=False)
    for k in (1, 2, 3, 7, 12):
        K = min(k, G)
        picks = pick_conformers(item, k=K, **kw)["picks"].cpu().tolist()                  # the three forms of init
        for init, seeds in (("maxmin", picks), ("first", list(range(K))), (list(range(G - K, G)), list(range(G - K, G))),
                            (np.array(picks[::-1]), picks[::-1])):
            if not isinstance(init, str) and k != K:
                continue                                     # (an explicit init is k indices)
            want = KR.kmedoids(matrix, seeds)
            res = medoid_conformers(item, k, init=init, **kw)
            _check_result(res, want, G, n)
            assert torch.equal(res["pos"].cpu(), torch.from_numpy(gen[want[0]]))
    # K = 1 returns the conformer with the smallest row sum (the lowest index among equals)
    sums = KR.Q(matrix).sum(axis=1, dtype=np.uint64) - KR.Q(np.diag(matrix))
    central = medoid_conformers(item, 1, **kw)
    assert sums[int(central["medoids"][0])] == sums.min() and central["converged"]
    assert central["cost"] * 2 ** 28 == sums.min() and central["count"].tolist() == [G] and central["population"].tolist() == [1.0]
    one = medoid_conformers(item, 1, max_iter=1, init=[int(np.argmax(sums))], **kw)
    assert (one["converged"], one["iters"]) == (False, 1) and one["cost"] == central["cost"]   # one update from anywhere gets there


@pytest.mark.parametrize("n,K,G", [(20, 4, 37), (45, 7, 150)])
def test_families_give_one_cluster_each_with_their_populations(n, K, G):
    """K tight families (0.03 Angstrom of noise) far apart, of distinct sizes: with K medoids from MaxMin seeds -- one per family,
    as tests/test_hip_picks.py shows -- every cluster is one family and `population` its share"""
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.medoids import medoid_conformers
    from agdiff_amd.picks import pick_conformers
    item, label, gen, heavy = _families(n, K, G)
    matrix = self_rmsd_matrix(item).cpu().numpy()
    seeds = pick_conformers(item, k=K, align=False)["picks"].cpu().tolist()
    res = medoid_conformers(item, K)
    _check_result(res, KR.kmedoids(matrix, seeds), G, n)
    med, labels = res["medoids"].cpu().numpy(), res["labels"].cpu().numpy()
    assert sorted(label[med].tolist()) == list(range(K)) and np.array_equal(label[med][labels], label) and res["converged"]
    sizes = [int((label == label[m]).sum()) for m in med]
    assert res["count"].cpu().tolist() == sizes
    assert res["population"].cpu().tolist() == [float(F32(s) / F32(G)) for s in sizes]
    for r, m in enumerate(med):                              # each medoid is the most central member of its family
        idx = np.flatnonzero(label == label[m])
        sub = KR.Q(matrix[np.ix_(idx, idx)]).sum(axis=1, dtype=np.uint64) - KR.Q(matrix[idx, idx])
        assert sub[np.searchsorted(idx, m)] == sub.min() and res["within"][r].item() * 2 ** 28 == sub.min()
    assert float(res["near"].max()) < 0.5
    # align: rank 0 bit for bit, the others on it within the bar of agdiff_align_conformers
    assert torch.equal(res["pos"][0].cpu(), torch.from_numpy(gen[med[0]]))
    want = np.stack([_kabsch_align(gen[m], gen[med[0]], heavy) for m in med])
    dev = np.abs(res["pos"].cpu().numpy() - want).max()
    print("aligned medoids n=%d: max |aligned - float64 Kabsch| = %.3e Angstrom" % (n, dev))
    assert dev <= ALIGN_ATOL
    # "first" seeds may start several medoids in one family: still the restatement's result, a different local optimum
    plain = medoid_conformers(item, K, init="first", align=False)
    _check_result(plain, KR.kmedoids(matrix, list(range(K))), G, n)


def test_valid_mask_and_broken_coordinates_keep_the_items_own_indices():
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.medoids import medoid_conformers
    n, K, G = 20, 4, 37
    item, label, gen, heavy = _families(n, K, G)
    valid = np.ones(G, dtype=bool)
    valid[label == 2] = False                                # one whole family ...
    valid[[0, 5]] = False                                    # ... and the conformer that would have been the first seed
    sel = np.nonzero(valid)[0]
    matrix = self_rmsd_matrix(dict(item, pos_gen=gen[sel])).cpu().numpy()
    for mask in (valid, torch.from_numpy(valid).cuda()):
        for k, init, seeds in ((3, "first", [0, 1, 2]), (G, "first", list(range(sel.size))), (3, "maxmin", KR.maxmin(matrix, 3)[0].tolist()),
                               (2, [int(sel[-1]), int(sel[4])], [sel.size - 1, 4])):
            res = medoid_conformers(item, k, init=init, valid=mask, align=False)
            _check_result(res, KR.kmedoids(matrix, seeds), G, n, sel=sel)
            assert np.array_equal(res["labels"].cpu().numpy() == -1, ~valid) and bool(torch.isnan(res["near"][~torch.from_numpy(valid)]).all())
    res = medoid_conformers(item, 3, valid=valid)
    assert sorted(label[res["medoids"].cpu().numpy()].tolist()) == [0, 1, 3]
    for init in ([0, 1, 2], [1, 2, int(np.nonzero(label == 2)[0][0])], [1, 2, G], [1, 1, 2]):
        with pytest.raises(ValueError):
            medoid_conformers(item, 3, init=init, valid=valid)
    # a conformer with a coordinate that is not finite is masked before the matrix is made: the same result as with the mask
    broken = gen.copy()
    broken[0, 3, 1], broken[5, 0, 0] = np.nan, np.inf
    for c in np.nonzero(label == 2)[0]:
        broken[c, -1, 2] = -np.inf
    got = medoid_conformers(dict(item, pos_gen=broken), G, init="first", align=False)
    _check_result(got, KR.kmedoids(matrix, list(range(sel.size))), G, n, sel=sel)
    assert torch.equal(got["pos"].cpu(), torch.from_numpy(gen[got["medoids"].cpu().numpy()]))
    with pytest.raises(ValueError):
        medoid_conformers(dict(item, pos_gen=broken), 1, init=[5])
    none = medoid_conformers(item, 3, valid=np.zeros(G, dtype=bool))
    assert all(tuple(none[k].shape) == (0,) for k in ("medoids", "count", "population", "within")) and tuple(none["pos"].shape) == (0, n, 3)
    assert (none["labels"] == -1).all() and bool(torch.isnan(none["near"]).all()) and none["cost"] == 0.0
    assert none["labels"].shape == (G,) and none["near"].shape == (G,) and none["iters"] == 0 and none["converged"] is True
    assert none["medoids"].dtype == torch.int32 and none["within"].dtype == torch.float64 and none["count"].dtype == torch.int32


def test_tfd_families_and_ring_terms():
    """pentane rotamers (the construction of tests/test_hip_picks.py) by TFD, and a six-ring's chairs, boats and twist-boats by the
    TFD with ring terms: without them a six-ring has no torsion at all and every TFD is 0"""
    from agdiff_amd.medoids import medoid_conformers
    from agdiff_amd.torsions import tfd_self
    rng = np.random.default_rng(17)
    g = np.pi / 3
    rotamers, sizes = [(np.pi, np.pi), (np.pi, g), (g, g), (-g, -g)], [9, 6, 4, 2]
    label = rng.permutation(np.repeat(np.arange(4), sizes))
    gen = np.stack([_moved(rng, TR.chain_positions(np.array(rotamers[c]) + 0.03 * rng.normal(size=2))) for c in label]).astype(F32)
    at, bi, bt = TR.alkane(5)
    item = dict(atom_type=at, bond_index=bi, bond_type=bt, pos_gen=gen)
    G = label.shape[0]
    matrix = tfd_self(item)[0].cpu().numpy()
    res = medoid_conformers(item, 4, metric="tfd")
    _check_result(res, KR.kmedoids(matrix, KR.maxmin(matrix, 4)[0].tolist()), G, 5)
    med = res["medoids"].cpu().numpy()
    assert sorted(label[med].tolist()) == [0, 1, 2, 3] and np.array_equal(label[med][res["labels"].cpu().numpy()], label)
    assert res["count"].cpu().tolist() == [sizes[label[m]] for m in med]
    assert torch.equal(res["pos"][0].cpu(), torch.from_numpy(gen[med[0]]))
    want = np.stack([_kabsch_align(gen[m], gen[med[0]], np.arange(5)) for m in med])
    assert np.abs(res["pos"].cpu().numpy() - want).max() <= ALIGN_ATOL
    pos = np.stack([RR.chair()] * 6 + [RR.boat()] * 5 + [RR.twist_boat()] * 4)
    ring = (pos + 0.01 * np.random.default_rng(6).normal(size=pos.shape)).astype(F32)
    at, bi, bt = TR.cyclohexane()
    item = dict(atom_type=at, bond_index=bi, bond_type=bt, pos_gen=ring)
    matrix = tfd_self(item, rings=True)[0].cpu().numpy()
    res = medoid_conformers(item, 3, metric="tfd", tfd_rings=True, align=False)
    _check_result(res, KR.kmedoids(matrix, KR.maxmin(matrix, 3)[0].tolist()), 15, 6)
    assert sorted(res["count"].cpu().tolist()) == [4, 5, 6] and res["labels"].cpu().tolist()[:6] == [0] * 6
    flat = medoid_conformers(item, 3, metric="tfd", align=False)          # every TFD is 0: the seeds stay, the rest goes to rank 0
    assert flat["medoids"].cpu().tolist() == [0, 1, 2] and flat["count"].tolist() == [13, 1, 1] and flat["cost"] == 0.0
    assert flat["iters"] == 1 and flat["converged"]


# ------------------------------------------------------------------------------------------------ 7. the command line
def test_command_line_round_trip(tmp_path, capsys):
    from agdiff_amd import driver, medoids, synth
    rng = np.random.default_rng(9)
    at, bonds, gen7, thr = seven_pattern_conformers(rng)
    _, bi, bt = TR.graph(at, bonds)
    mols, gens = [dict(atom_type=at, edge_index=bi, edge_type=bt, num_refs=4, name="seven")], [gen7]
    for i, (n, G) in enumerate(((15, 7), (12, 5))):
        a, r, c, ty = synth.random_molecule(rng, n)
        mols.append(dict(atom_type=a, edge_index=np.stack([r, c]), edge_type=ty, num_refs=3, name="m%d" % (i + 1)))
        base = rng.normal(size=(2, n, 3)) * 1.5
        gens.append(np.stack([_moved(rng, base[k % 2] + 0.02 * rng.normal(size=(n, 3))) for k in range(G)]).astype(F32))
    driver.save_testset(str(tmp_path / "test.npz"), mols)
    np.savez(str(tmp_path / "samples_all.npz"), **{"pos_gen_%d" % i: g for i, g in enumerate(gens)})
    base = ["--samples", str(tmp_path / "samples_all.npz"), "--testset", str(tmp_path / "test.npz")]
    out = medoids.main(base + ["--count", "2", "--align", "--out", str(tmp_path / "medoids.npz")])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and "6 medoids of 19 conformers" in line[0] and "RMSD" in line[0] and "0 molecules did not converge" in line[0]
    z = np.load(str(tmp_path / "medoids.npz"))
    keys = ("medoid", "cluster", "dist", "count", "population", "within", "cost", "iters", "converged", "pos", "name")
    assert set(z.files) == {"%s_%d" % (k, i) for k in keys for i in range(3)} == set(out)
    for i, g in enumerate(gens):
        G, n = g.shape[0], g.shape[1]
        for k, dtype, shape in (("medoid", np.int32, (2,)), ("cluster", np.int32, (G,)), ("dist", np.float32, (G,)),
                                ("count", np.int32, (2,)), ("population", np.float32, (2,)), ("within", np.float64, (2,)),
                                ("cost", np.float64, ()), ("iters", np.int32, ()), ("converged", np.int8, ()),
                                ("pos", np.float32, (2, n, 3))):
            assert z["%s_%d" % (k, i)].dtype == dtype and z["%s_%d" % (k, i)].shape == shape, (k, i)
            assert np.array_equal(z["%s_%d" % (k, i)], out["%s_%d" % (k, i)], equal_nan=True)
        assert str(z["name_%d" % i]) == mols[i]["name"]
        med = z["medoid_%d" % i]
        assert np.array_equal(z["cluster_%d" % i][med], np.arange(2)) and z["count_%d" % i].sum() == G and z["converged_%d" % i] == 1
        assert np.array_equal(z["pos_%d" % i][0], g[med[0]]) and z["within_%d" % i].sum() == z["cost_%d" % i]
        assert np.array_equal(z["population_%d" % i], z["count_%d" % i].astype(F32) / F32(G))
    # molecules 1 and 2 are two tight families each, the even and the odd conformers: one medoid in each
    for i in (1, 2):
        assert sorted(z["medoid_%d" % i] % 2) == [0, 1] and np.array_equal(z["cluster_%d" % i] == z["cluster_%d" % i][0],
                                                                          np.arange(gens[i].shape[0]) % 2 == 0)
        assert z["dist_%d" % i].max() < 0.2
    first = medoids.main(base + ["--count", "2", "--init", "first", "--max-iter", "1", "--out", str(tmp_path / "first.npz")])
    assert "first seeds, at most 1 updates" in capsys.readouterr().out
    assert all(first["iters_%d" % i] == 1 for i in range(3))
    more = medoids.main(base + ["--count", "2", "--drop-invalid", "--out", str(tmp_path / "checked.npz")])
    capsys.readouterr()
    for i in range(3):
        assert more["valid_%d" % i].dtype == np.int8
        assert np.array_equal(more["cluster_%d" % i] == -1, more["valid_%d" % i] == 0)
        assert np.array_equal(np.isnan(more["dist_%d" % i]), more["valid_%d" % i] == 0)
    tfd = medoids.main(base + ["--count", "2", "--tfd", "--out", str(tmp_path / "tfd.npz")])
    assert "TFD" in capsys.readouterr().out and all(tfd["cluster_%d" % i].shape == (gens[i].shape[0],) for i in range(3))
