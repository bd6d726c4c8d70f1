"""GPU (MI355X): PAM (agdiff_amd.pam; csrc/eval.hip: k_pam_*) against the numpy restatement of its rule (tests/pam_ref.py) on the
same float32 matrix -- integers equal, floats and doubles bit-equal, NaN at the same places, n_swaps and status included -- and end
to end through pam_conformers and the command line.

Every sum the walk makes is a sum of integers (the matrix entries on a 2^-28 grid) and every float it writes is a copy of a matrix
entry or such a sum divided by 2^28, so every comparison with the restatement is exact.  The one tolerance is ALIGN_ATOL, for the
superposed medoids against a float64 Kabsch of the same fp32 inputs: the bar that tests/test_hip_clusters.py carries for
agdiff_align_conformers, the same kernel under the same bar; nothing new is measured here."""
import functools

import numpy as np
import pytest
import torch

import kmedoids_ref as KR
import pam_ref as PR
import rings_ref as RR
import tfd_ref as TR
from test_hip_clusters import ALIGN_ATOL, _families, _kabsch_align, _moved, seven_pattern_conformers

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL, FSENTINEL, TAIL = -7, -777.0, 64           # (no output is negative but the -1 of medoids / labels)


def _launch(dist, G, K, anchor, init=None, max_swaps=64):
    """agdiff_pam_build (init None) or agdiff_pam_swap on a device tensor [G, G] (or a numpy matrix), the eight arrays filled with
    a sentinel and followed by a canary tail, the scratch followed by one too: every entry must have been written, the tails must
    be as they were.  The result in the restatement's form."""
    from agdiff_amd import _lib
    dev = dist if torch.is_tensor(dist) else torch.from_numpy(np.array(dist, dtype=F32)).cuda()
    full = lambda m, v, dtype: torch.full((m + TAIL,), v, dtype=dtype, device="cuda")
    medoids, labels, size, n_swaps, status = (full(m, SENTINEL, torch.int32) for m in (K, G, K, 1, 1))
    near = full(G, FSENTINEL, torch.float32)
    within, cost = full(K, FSENTINEL, torch.float64), full(1, FSENTINEL, torch.float64)
    words = _lib.DEFINES["AGDIFF_PAM_WORK_BYTES"] // 8
    work = full(words, SENTINEL, torch.int64)
    outs = (medoids, labels, near, size, within, cost, n_swaps, status, work)
    if init is None:
        _lib.call("agdiff_pam_build", dev, G, K, int(anchor), *outs)
    else:
        seeds = torch.tensor(list(init), dtype=torch.int32, device="cuda")
        _lib.call("agdiff_pam_swap", dev, G, K, seeds, int(anchor), int(max_swaps), *outs)
        assert seeds.cpu().tolist() == list(init)
    assert (work[words:] == SENTINEL).all()
    out = []
    for a, m, s in ((medoids, K, SENTINEL), (labels, G, SENTINEL), (near, G, FSENTINEL), (size, K, SENTINEL), (within, K, FSENTINEL),
                    (cost, 1, FSENTINEL), (n_swaps, 1, SENTINEL), (status, 1, SENTINEL)):
        a = a.cpu().numpy()
        assert (a[m:] == s).all() and not (a[:m] == s).any()
        out.append(a[:m])
    medoids, labels, near, size, within, cost, n_swaps, status = out
    assert ((medoids >= -1) & (medoids < G)).all() and ((labels >= -1) & (labels < K)).all() and status[0] in (0, 1, 2)
    return medoids, labels, near, size, within, cost[0], int(n_swaps[0]), int(status[0])


@functools.lru_cache(maxsize=None)
def _case(name, *args):
    """(matrix, its fixed-point image, the same matrix on the device) of a named structured matrix -- made once, left unchanged"""
    d = getattr(PR, name)(*args) if name != "metric" else PR.random_metric(args[0], seed=args[0])
    d.setflags(write=False)
    q = PR.Q(d)
    q.setflags(write=False)
    return d, q, torch.from_numpy(np.array(d)).cuda()


def _fresh(d):
    d = np.ascontiguousarray(d, dtype=F32)
    return d, None, torch.from_numpy(d.copy()).cuda()


@functools.lru_cache(maxsize=None)
def _build_order(name, *args):
    """the restatement's BUILD picks for every rank the matrix has, from anchor 0: the medoids of any K are its first K"""
    d, q, _ = _case(name, *args)
    return PR.build(d, int(PR.eligible_of(d, 0).sum()), q=q)[0]


def _describe(r):
    return r[0][:8], r[3][:8], r[5:]


def _both_build(case, K, anchor=0, order=None):
    d, q, dev = case
    want = PR.build(d, K, anchor, q=q, order=order)
    got = _launch(dev, d.shape[0], K, anchor)
    assert KR.same(got, want), "BUILD G = %d, K = %d, anchor = %d: got %s, want %s" % (d.shape[0], K, anchor, _describe(got), _describe(want))
    return got


def _both_swap(case, init, anchor=0, max_swaps=64):
    d, q, dev = case
    trace = []
    want = PR.swap(d, init, anchor, max_swaps=max_swaps, trace=trace, q=q)
    got = _launch(dev, d.shape[0], len(init), anchor, init=init, max_swaps=max_swaps)
    assert KR.same(got, want), "SWAP G = %d, init = %s ..., anchor = %d, max_swaps = %d: got %s, want %s" % (
        d.shape[0], list(init)[:8], anchor, max_swaps, _describe(got), _describe(want))
    return got, trace


# ------------------------------------------------------------------------------------------------ 1. the kernels against the rule
SIZES = [1, 2, 3, 63, 64, 65, 257, 1025]


@pytest.mark.parametrize("G", SIZES)
def test_kernels_equal_the_restated_rule(G):
    """across a wave, a workgroup of the state (64 columns) and of the candidates (4 rows), odd sizes; K from 1 to G; BUILD, and
    SWAP from the first K, the restatement's MaxMin picks and BUILD's medoids.  The larger sizes are cut short by max_swaps."""
    case = _case("metric", G)
    order = _build_order("metric", G)
    max_swaps = 64 if G <= 65 else (12 if G == 257 else 5)
    swapped = 0
    for K in sorted({1, min(2, G), min(7, G), min(100, G), max(G - 1, 1), G}):
        built = _both_build(case, K, order=order)
        assert built[6:] == (0, 0) and built[0].tolist() == order[:K].tolist()
        PR.check_invariants(case[0], 0, built, swapped=False)
        for init in (list(range(K)), PR.maxmin(case[0], K)[0].tolist(), built[0].tolist()):
            got, trace = _both_swap(case, init, max_swaps=max_swaps)
            assert got[7] == 0 or got[6] == max_swaps
            PR.check_invariants(case[0], 0, got, trace)
            swapped += got[6]
            if K == G:                                       # no candidate: status 0 with 0 swaps
                assert got[6:] == (0, 0) and got[5] == 0 and got[0].tolist() == init and got[3].tolist() == [1] * G
    assert swapped > 0 or G <= 3


@pytest.mark.parametrize("K", [1024, 1025])
def test_bin_layout_boundary(K):
    """one candidate row per wave up to K = 1024 (4 K bins a workgroup), one per workgroup of four waves above"""
    case = _case("metric", 1100)
    for init in (list(range(K)), list(range(1100 - K, 1100))):
        got, trace = _both_swap(case, init, max_swaps=4)
        assert got[6:] == (4, 1)
        PR.check_invariants(case[0], 0, got, trace)


def test_size_limit():
    case = _case("metric", 4096)
    got, trace = _both_swap(case, list(range(100)), max_swaps=8)
    assert got[6:] == (8, 1)
    PR.check_invariants(case[0], 0, got, trace)
    built = _both_build(case, 3)
    assert built[6:] == (0, 0)


def test_two_launches_give_equal_bytes_through_the_wrappers():
    from agdiff_amd.pam import pam_build, pam_swap
    for G, K in ((1000, 100), (1025, 10)):
        d, q, dev = _case("metric", G)
        a, b = pam_build(dev, G, K), pam_build(dev, G, K)
        c, e = pam_swap(dev, G, a[0], max_swaps=6), pam_swap(dev, G, b[0], anchor=int(a[0][0]), max_swaps=6)
        for x, y in ((a, b), (c, e)):
            for u, v, dtype, m in zip(x, y, (torch.int32, torch.int32, torch.float32, torch.int32, torch.float64, torch.float64,
                                            torch.int32, torch.int32), (K, G, G, K, K, 1, 1, 1)):
                assert u.dtype == dtype and tuple(u.shape) == (m,) and u.is_cuda
                assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
        want = PR.build(d, K, q=q)
        assert KR.same([t.cpu().numpy() for t in a[:6]] + [int(a[6]), int(a[7])], want)
        # (anchor None is init[0]: the metric matrix is clean, so every anchor marks everybody)
        assert KR.same([t.cpu().numpy() for t in c[:6]] + [int(c[6]), int(c[7])], PR.swap(d, want[0], max_swaps=6, q=q))


# ------------------------------------------------------------------------------------------------ 2. where the walk stops
def test_max_swaps_stops_and_launches_past_convergence_change_nothing():
    case = _case("metric", 257)
    init = list(range(7))
    full, trace = _both_swap(case, init, max_swaps=256)      # (256 iterations enqueued, all but a few return at once)
    n = full[6]
    assert full[7] == 0 and 3 <= n < 64 and len(trace) == n + 1
    for max_swaps, status in ((0, 1), (1, 1), (2, 1), (n - 1, 1), (n, 1), (n + 1, 0), (n + 2, 0)):
        got, _ = _both_swap(case, init, max_swaps=max_swaps)
        assert got[6:] == (min(max_swaps, n), status)
        if max_swaps >= n:
            assert KR.same(got[:6], full[:6])
    # memoryless: from the medoids of a stopped walk, with the same anchor, the walk goes on to the same end
    half, _ = _both_swap(case, init, max_swaps=2)
    rest, _ = _both_swap(case, half[0].tolist(), anchor=0, max_swaps=64)
    assert KR.same(rest[:6], full[:6]) and rest[6:] == (n - 2, 0)


# ------------------------------------------------------------------------------------------------ 3. ties and structured matrices
@pytest.mark.parametrize("name, args, K", [("line", (65,), 3), ("line", (1025,), 3), ("lattice", (33, 31), 7), ("lattice", (9, 7), 40)])
def test_exact_ties_across_candidates_and_ranks(name, args, K):
    """integer distances: nearly every arg-min is a tie between candidates, and between ranks wherever medoids are neighbours"""
    case = _case(name, *args)
    G = case[0].shape[0]
    built = _both_build(case, K)
    for init in (list(range(K)), list(range(G - K, G)), built[0].tolist()):
        got, trace = _both_swap(case, init, max_swaps=64 if G <= 65 else 6)
        PR.check_invariants(case[0], 0, got, trace)


@pytest.mark.parametrize("G", [65, 257])
def test_small_values_equal_and_zero_matrices(G):
    for K in (1, 7, 40):
        d = PR.small_values(G, seed=G + K)
        case = _fresh(d)
        built = _both_build(case, K)
        _both_swap(case, list(range(K)), max_swaps=8)
        _both_swap(case, built[0].tolist(), max_swaps=8)
        equal = _fresh(np.full((G, G), F32(2.5)))
        got = _both_build(equal, K)
        assert got[0].tolist() == list(range(K))             # every sum and every gain ties: the lowest index
        got, _ = _both_swap(equal, list(range(G - K, G)), max_swaps=8)
        assert got[6:] == (0, 0)
        zero = _fresh(np.zeros((G, G), F32))
        got = _both_build(zero, K)
        assert got[0].tolist() == list(range(K)) and got[5] == 0 and got[3].tolist() == [G - K + 1] + [1] * (K - 1)
        got, _ = _both_swap(zero, list(range(1, K + 1)), max_swaps=8)
        assert got[6:] == (0, 0) and got[0].tolist() == list(range(1, K + 1)) and not got[2].any()


@pytest.mark.parametrize("G", [64, 257])
def test_minus_zero_entries_are_zeros(G):
    d = np.array(_case("metric", G)[0])
    rng = np.random.default_rng(G)
    dup = rng.choice(G, size=G // 4, replace=False)
    d[dup[:, None], dup[None, :]] = -0.0                     # a clique of duplicates at distance -0.0, diagonal included
    pos = np.where(d == 0, F32(0), d)
    case = _fresh(d)
    for K in (1, 5):
        got = _both_build(case, K)
        assert KR.same(got, PR.build(pos, K)) and not np.signbit(got[2]).any()
    for init in ([int(dup[0])], [0, 1, 2], sorted(dup.tolist())[:5]):
        got, _ = _both_swap(case, init, anchor=init[0], max_swaps=8)
        assert KR.same(got, PR.swap(pos, init, max_swaps=8)) and not np.signbit(got[2]).any()


@pytest.mark.parametrize("G", [65, 257])
def test_ineligible_conformers_and_bad_entries(G):
    base = _case("metric", G)[0]
    bad = sorted({1, G // 3, G - 1, 64} & set(range(1, G)))
    d = PR.with_inf(base, bad)
    ok = [j for j in range(G) if j not in bad]
    case = _fresh(d)
    for K in (1, 7, len(ok)):
        built = _both_build(case, K)
        assert (built[1][bad] == -1).all() and np.isnan(built[2][bad]).all() and built[3].sum() == len(ok)
    assert _both_build(case, len(ok) + 1)[7] == 2            # K above the eligible count
    assert _both_build(case, 1, anchor=bad[0])[0].tolist() == [bad[0]]     # an unusable anchor is alone with itself
    for init in ([0], ok[:7], ok[-7:]):
        got, trace = _both_swap(case, init, max_swaps=8)
        assert (got[1][bad] == -1).all() and np.isnan(got[2][bad]).all() and got[3].sum() == len(ok)
        PR.check_invariants(d, 0, got, trace)
    got, _ = _both_swap(case, ok, max_swaps=8)               # K = the eligible count: no candidate
    assert got[6:] == (0, 0)
    for value in (np.nan, -1.0, 5000.0, np.inf, -np.inf):    # an eligible pair's bad entry counts as 2^40, and near copies it
        e = np.array(base)
        e[5, 6] = e[6, 5] = e[ok[-1], ok[-2]] = e[7, 0] = e[9, 20] = value
        case_e = _fresh(e)
        _both_build(case_e, 7)
        for init, anchor in (([0, 5], 0), ([5, 0, ok[-1]], 5), (ok[:7], 0), ([9, 6], 0)):
            got, _ = _both_swap(case_e, init, anchor=anchor, max_swaps=8)
            if anchor == 5:                                  # row 5 decides: 6 is out
                assert got[1][6] == -1
    at_cap = np.array(base)
    at_cap[5, 6] = at_cap[6, 5] = 4096.0                     # the cap itself is a distance
    at_cap[0, 3] = at_cap[3, 0] = np.nextafter(F32(4096), F32(np.inf))      # just above it: 3 is out when 0 is the anchor
    case_c = _fresh(at_cap)
    assert _both_build(case_c, 3)[1][3] == -1
    got, _ = _both_swap(case_c, [0, 5], max_swaps=8)
    assert got[1][3] == -1


def test_rows_are_read_not_columns():
    d = np.array(_case("metric", 65)[0])
    d[np.triu_indices(65, 1)] *= F32(1.75)                   # dist[c][o] != dist[o][c]
    case = _fresh(d)
    flipped = _fresh(d.T)
    for K in (1, 4):
        a, b = _both_build(case, K), _both_build(flipped, K)
        assert not KR.same(a[:6], b[:6])
        a, _ = _both_swap(case, list(range(K)))
        b, _ = _both_swap(flipped, list(range(K)))
        assert not KR.same(a[:6], b[:6])


@pytest.mark.parametrize("G", [63, 1023, 1025])
def test_matrix_one_float_into_its_allocation(G):
    """dist needs 4-byte alignment only; with G odd no row of it is 8-byte aligned"""
    d, q, _ = _case("metric", G)
    buf = torch.full((G * G + 2,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    off = buf[1:1 + G * G].view(G, G)
    off.copy_(torch.from_numpy(np.array(d)))
    assert off.data_ptr() % 8 == 4 and off.is_contiguous()
    built = _both_build((d, q, off), 7)
    for init in ([G - 1], list(range(7)), built[0].tolist(), list(range(G - 40, G))):
        _both_swap((d, q, off), init, max_swaps=4)


# ------------------------------------------------------------------------------------------------ 4. status 2, nothing to do
@pytest.mark.parametrize("G", [9, 300])
def test_bad_seeds_and_bad_anchors_give_status_two(G):
    """ordinary inputs with a defined result: the kernels check the seeds and the anchor and fill every output"""
    d = PR.with_inf(_case("metric", G)[0], [4])
    case = _fresh(d)

    def filled(got):
        assert got[7] == 2 and got[6] == 0 and got[5] == 0 and (got[0] == -1).all() and (got[1] == -1).all() and np.isnan(got[2]).all()
        assert not got[3].any() and not got[4].any()
    for init in ([0, 0], [1, 2, 1], [-1], [0, G], [G], [0, 4], [4, 0], [3, -1], [0, 1 << 30], list(range(5, 9)) + [5]):
        filled(_both_swap(case, init)[0])
    for anchor in (-1, G, 1 << 30, 4):                       # out of range; or a row that marks nobody but itself
        filled(_both_swap(case, [0, 3], anchor=anchor)[0])
    for anchor in (-1, G, 1 << 30):
        filled(_both_build(case, 2, anchor=anchor))
    filled(_both_build(case, 2, anchor=4))                   # K above the one eligible conformer
    filled(_both_build(case, G))                             # ... and above the G - 1
    assert _both_swap(case, [0, 3])[0][7] == 0 and _both_swap(case, [0, 3], anchor=7)[0][7] == 0


def test_no_conformers_is_no_launch():
    from agdiff_amd import _lib
    for build in (True, False):
        n_swaps, status = (torch.full((1 + TAIL,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2))
        cost = torch.full((1 + TAIL,), FSENTINEL, dtype=torch.float64, device="cuda")
        ints = torch.full((TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
        floats = torch.full((TAIL,), FSENTINEL, dtype=torch.float32, device="cuda")
        doubles = torch.full((TAIL,), FSENTINEL, dtype=torch.float64, device="cuda")
        work = torch.full((TAIL,), SENTINEL, dtype=torch.int64, device="cuda")
        dist = torch.zeros(1, dtype=torch.float32, device="cuda")
        outs = (ints, ints, floats, ints, doubles, cost, n_swaps, status, work)
        if build:
            _lib.call("agdiff_pam_build", dist, 0, 1, 0, *outs)
        else:
            _lib.call("agdiff_pam_swap", dist, 0, 1, ints, 0, 32, *outs)
        assert n_swaps.cpu().tolist() == [0] + [SENTINEL] * TAIL and status.cpu().tolist() == [0] + [SENTINEL] * TAIL
        assert cost.cpu().tolist() == [0.0] + [FSENTINEL] * TAIL
        assert (ints == SENTINEL).all() and (floats == FSENTINEL).all() and (doubles == FSENTINEL).all() and (work == SENTINEL).all()


def test_wrappers_refuse_what_the_header_refuses():
    from agdiff_amd import _lib
    from agdiff_amd.pam import pam_build, pam_conformers, pam_swap
    G = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    big = torch.zeros((G, G), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.AgdiffLimitError):
        pam_build(big, G, 1)
    with pytest.raises(_lib.AgdiffLimitError):
        pam_swap(big, G, one)
    with pytest.raises(_lib.AgdiffLimitError):
        pam_conformers({"atom_type": np.array([6, 6]), "pos_gen": np.zeros((G, 2, 3), np.float32)}, 10)
    small = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    for bad in (lambda: pam_swap(torch.zeros((4, 5), dtype=torch.float32, device="cuda"), 4, one), lambda: pam_build(small.double(), 4, 1),
                lambda: pam_swap(small, 4, one.long()), lambda: pam_swap(small, 4, one.cpu()), lambda: pam_swap(small, 4, one, max_swaps=-1),
                lambda: pam_swap(small, 4, one, max_swaps=257), lambda: pam_build(small, 4, 0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.AgdiffHipError):
        pam_build(small, 4, 5)                                                            # K > G
    with pytest.raises(_lib.AgdiffHipError):
        pam_swap(small, 4, torch.zeros(5, dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------------------------------------ 5. end to end
def _check_result(res, want, G, n_atoms, sel=None, build_cost=None):
    """a pam_conformers result against the restatement run on the matrix of the usable conformers (`sel`: their indices in the
    item)"""
    med, labels, near, size, within, cost, n_swaps, status = want
    K = len(med)
    sel = np.arange(G) if sel is None else np.asarray(sel)
    for key, dtype, shape in (("medoids", torch.int32, (K,)), ("labels", torch.int32, (G,)), ("near", torch.float32, (G,)),
                              ("count", torch.int32, (K,)), ("population", torch.float32, (K,)), ("within", torch.float64, (K,)),
                              ("pos", torch.float32, (K, n_atoms, 3))):
        assert res[key].dtype == dtype and tuple(res[key].shape) == shape and res[key].is_cuda, key
    assert isinstance(res["cost"], float) and res["cost"] == cost and res["swaps"] == n_swaps and res["converged"] is (status == 0)
    assert "iters" not in res and (res.get("build_cost") == build_cost)
    assert res["medoids"].cpu().tolist() == sel[med].tolist()
    full_labels, full_near = np.full(G, -1, dtype=np.int32), np.full(G, np.nan, dtype=F32)
    full_labels[sel], full_near[sel] = labels, near
    assert KR.same((res["labels"].cpu().numpy(), res["near"].cpu().numpy(), res["count"].cpu().numpy(), res["within"].cpu().numpy()),
                   (full_labels, full_near, size, within))
    assert KR.same((res["population"].cpu().numpy(),), (size.astype(F32) / F32(sel.size),))
    assert int(res["count"].sum()) == sel.size


def _pam_ref(matrix, K, max_swaps=4096):
    b = PR.build(matrix, K)
    return PR.swap(matrix, b[0], 0, max_swaps=max_swaps), float(b[5])


def _seven():
    at, bonds, gen, _ = seven_pattern_conformers(np.random.default_rng(9))
    _, bi, bt = TR.graph(at, bonds)
    return dict(atom_type=at, bond_index=bi, bond_type=bt, pos_gen=gen), gen


def _same_result(a, b):
    assert set(a) == set(b)
    for key in a:
        if torch.is_tensor(a[key]):
            assert a[key].dtype == b[key].dtype and torch.equal(a[key].view(torch.uint8), b[key].view(torch.uint8)), key
        else:
            assert a[key] == b[key] and type(a[key]) is type(b[key]), key


@pytest.mark.parametrize("metric, rings", [("rmsd", False), ("tfd", False), ("tfd", True)])
def test_seven_pattern_equals_the_restatement_on_the_devices_matrix(metric, rings):
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.pam import pam_conformers
    from agdiff_amd.picks import pick_conformers
    from agdiff_amd.torsions import tfd_self
    item, gen = _seven()
    G, n = gen.shape[0], gen.shape[1]
    matrix = (self_rmsd_matrix(item) if metric == "rmsd" else tfd_self(item, rings=rings)[0]).cpu().numpy()
    kw = dict(metric=metric, tfd_rings=rings, align=False)
    for k in (1, 2, 3, 7, 12):
        K = min(k, G)
        want, build_cost = _pam_ref(matrix, K)
        res = pam_conformers(item, k, **kw)
        _check_result(res, want, G, n, build_cost=build_cost)
        assert res["converged"] and torch.equal(res["pos"].cpu(), torch.from_numpy(gen[want[0]]))
        for chunk in (1, 5):                                 # chunking does not show
            _same_result(pam_conformers(item, k, chunk=chunk, **kw), res)
        only, _ = _pam_ref(matrix, K, max_swaps=0)           # BUILD alone: nothing was looked for
        _check_result(pam_conformers(item, k, max_swaps=0, **kw), only, G, n, build_cost=build_cost)
        picks = pick_conformers(item, k=K, **kw)["picks"].cpu().tolist()                  # the other forms of init
        alt = KR.kmedoids(matrix, picks, max_iter=128)[0].tolist()
        for init, seeds in (("maxmin", picks), ("first", list(range(K))), ("alternate", alt),
                            (list(range(G - K, G)), list(range(G - K, G))), (np.array(picks[::-1]), picks[::-1])):
            if not isinstance(init, str) and k != K:
                continue                                     # (an explicit init is k indices)
            anchor = 0 if isinstance(init, str) else seeds[0]
            for max_swaps in (4096, 1):
                res = pam_conformers(item, k, init=init, max_swaps=max_swaps, **kw)
                _check_result(res, PR.swap(matrix, seeds, anchor, max_swaps=max_swaps), G, n)
                _same_result(pam_conformers(item, k, init=init, max_swaps=max_swaps, chunk=1, **kw), res)
    # K = 1 returns the conformer with the smallest row sum (the lowest index among equals), from BUILD alone
    sums = KR.Q(matrix).sum(axis=1, dtype=np.uint64) - KR.Q(np.diag(matrix))
    central = pam_conformers(item, 1, **kw)
    assert sums[int(central["medoids"][0])] == sums.min() and central["swaps"] == 0 and central["build_cost"] == central["cost"]


@pytest.mark.parametrize("n,K,G", [(20, 4, 37), (45, 7, 150)])
def test_families_give_one_medoid_each_with_their_populations(n, K, G):
    """K tight families (0.03 Angstrom of noise) far apart, of distinct sizes: every cluster is one family, `population` its share,
    each medoid its family's most central member -- from BUILD, and from `first` seeds, which start several medoids in one family
    and leave the alternating walk (tests/test_hip_medoids.py) in a worse optimum"""
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.medoids import medoid_conformers
    from agdiff_amd.pam import pam_conformers
    item, label, gen, heavy = _families(n, K, G)
    matrix = self_rmsd_matrix(item).cpu().numpy()
    want, build_cost = _pam_ref(matrix, K)
    res = pam_conformers(item, K)
    for r, init in ((res, "build"), (pam_conformers(item, K, init="first"), "first")):
        if init == "build":
            _check_result(r, want, G, n, build_cost=build_cost)
        else:
            _check_result(r, PR.swap(matrix, list(range(K)), 0, max_swaps=4096), G, n)
        med, labels = r["medoids"].cpu().numpy(), r["labels"].cpu().numpy()
        assert sorted(label[med].tolist()) == list(range(K)) and np.array_equal(label[med][labels], label) and r["converged"]
        sizes = [int((label == label[m]).sum()) for m in med]
        assert r["count"].cpu().tolist() == sizes
        assert r["population"].cpu().tolist() == [float(F32(s) / F32(G)) for s in sizes]
        for rank, m in enumerate(med):                       # each medoid is the most central member of its family
            idx = np.flatnonzero(label == label[m])
            sub = KR.Q(matrix[np.ix_(idx, idx)]).sum(axis=1, dtype=np.uint64) - KR.Q(matrix[idx, idx])
            assert sub[np.searchsorted(idx, m)] == sub.min() and r["within"][rank].item() * 2 ** 28 == sub.min()
        assert float(r["near"].max()) < 0.5
    assert res["cost"] <= medoid_conformers(item, K, init="first", align=False)["cost"]
    # align: rank 0 bit for bit, the others on it within the bar of agdiff_align_conformers
    med = res["medoids"].cpu().numpy()
    assert torch.equal(res["pos"][0].cpu(), torch.from_numpy(gen[med[0]]))
    aligned = np.stack([_kabsch_align(gen[m], gen[med[0]], heavy) for m in med])
    dev = np.abs(res["pos"].cpu().numpy() - aligned).max()
    print("aligned medoids n=%d: max |aligned - float64 Kabsch| = %.3e Angstrom" % (n, dev))
    assert dev <= ALIGN_ATOL


def test_valid_mask_and_broken_coordinates_keep_the_items_own_indices():
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.pam import pam_conformers
    n, K, G = 20, 4, 37
    item, label, gen, heavy = _families(n, K, G)
    valid = np.ones(G, dtype=bool)
    valid[label == 2] = False                                # one whole family ...
    valid[[0, 5]] = False                                    # ... and the conformer that would have been the anchor
    sel = np.nonzero(valid)[0]
    matrix = self_rmsd_matrix(dict(item, pos_gen=gen[sel])).cpu().numpy()
    for mask in (valid, torch.from_numpy(valid).cuda()):
        for k in (3, G):
            want, build_cost = _pam_ref(matrix, min(k, sel.size))
            res = pam_conformers(item, k, valid=mask, align=False)
            _check_result(res, want, G, n, sel=sel, build_cost=build_cost)
            assert np.array_equal(res["labels"].cpu().numpy() == -1, ~valid) and bool(torch.isnan(res["near"][~torch.from_numpy(valid)]).all())
        res = pam_conformers(item, 2, init=[int(sel[-1]), int(sel[4])], valid=mask, align=False)
        _check_result(res, PR.swap(matrix, [sel.size - 1, 4], max_swaps=4096), G, n, sel=sel)
    res = pam_conformers(item, 3, valid=valid)
    assert sorted(label[res["medoids"].cpu().numpy()].tolist()) == [0, 1, 3]
    for init in ([0, 1, 2], [1, 2, int(np.nonzero(label == 2)[0][0])], [1, 2, G], [1, 1, 2]):
        with pytest.raises(ValueError):
            pam_conformers(item, 3, init=init, valid=valid)
    # a conformer with a coordinate that is not finite is masked before the matrix is made: the same result as with the mask
    broken = gen.copy()
    broken[0, 3, 1], broken[5, 0, 0] = np.nan, np.inf
    for c in np.nonzero(label == 2)[0]:
        broken[c, -1, 2] = -np.inf
    want, build_cost = _pam_ref(matrix, 3)
    got = pam_conformers(dict(item, pos_gen=broken), 3, align=False)
    _check_result(got, want, G, n, sel=sel, build_cost=build_cost)
    assert torch.equal(got["pos"].cpu(), torch.from_numpy(gen[got["medoids"].cpu().numpy()]))
    with pytest.raises(ValueError):
        pam_conformers(dict(item, pos_gen=broken), 1, init=[5])
    none = pam_conformers(item, 3, valid=np.zeros(G, dtype=bool))
    assert all(tuple(none[k].shape) == (0,) for k in ("medoids", "count", "population", "within")) and tuple(none["pos"].shape) == (0, n, 3)
    assert (none["labels"] == -1).all() and bool(torch.isnan(none["near"]).all()) and none["cost"] == 0.0 and none["build_cost"] == 0.0
    assert none["labels"].shape == (G,) and none["near"].shape == (G,) and none["swaps"] == 0 and none["converged"] is True


def test_ring_terms_of_the_tfd():
    """a six-ring's chairs, boats and twist-boats by the TFD with ring terms: one medoid each"""
    from agdiff_amd.pam import pam_conformers
    from agdiff_amd.torsions import tfd_self
    pos = np.stack([RR.chair()] * 6 + [RR.boat()] * 5 + [RR.twist_boat()] * 4)
    ring = (pos + 0.01 * np.random.default_rng(6).normal(size=pos.shape)).astype(F32)
    at, bi, bt = TR.cyclohexane()
    item = dict(atom_type=at, bond_index=bi, bond_type=bt, pos_gen=ring)
    matrix = tfd_self(item, rings=True)[0].cpu().numpy()
    want, build_cost = _pam_ref(matrix, 3)
    res = pam_conformers(item, 3, metric="tfd", tfd_rings=True, align=False)
    _check_result(res, want, 15, 6, build_cost=build_cost)
    assert sorted(res["count"].cpu().tolist()) == [4, 5, 6]
    flat = pam_conformers(item, 3, metric="tfd", align=False)             # every TFD is 0: the lowest indices, nothing to swap
    assert flat["medoids"].cpu().tolist() == [0, 1, 2] and flat["count"].tolist() == [13, 1, 1] and flat["cost"] == 0.0
    assert flat["swaps"] == 0 and flat["converged"]


# ------------------------------------------------------------------------------------------------ 6. the command line
def test_command_line_round_trip_and_silhouette_of_its_labels(tmp_path, capsys):
    from agdiff_amd import driver, pam, silhouette, synth
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
    out = pam.main(base + ["--count", "2", "--align", "--out", str(tmp_path / "pam.npz")])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and "6 medoids of 19 conformers" in line[0] and "RMSD" in line[0] and "PAM from build" in line[0]
    assert "0 molecules did not converge" in line[0]
    z = np.load(str(tmp_path / "pam.npz"))
    keys = ("medoid", "cluster", "dist", "count", "population", "within", "cost", "swaps", "converged", "build_cost", "pos", "name")
    assert set(z.files) == {"%s_%d" % (k, i) for k in keys for i in range(3)} == set(out)
    for i, g in enumerate(gens):
        G, n = g.shape[0], g.shape[1]
        for k, dtype, shape in (("medoid", np.int32, (2,)), ("cluster", np.int32, (G,)), ("dist", np.float32, (G,)),
                                ("count", np.int32, (2,)), ("population", np.float32, (2,)), ("within", np.float64, (2,)),
                                ("cost", np.float64, ()), ("swaps", np.int32, ()), ("converged", np.int8, ()),
                                ("build_cost", np.float64, ()), ("pos", np.float32, (2, n, 3))):
            assert z["%s_%d" % (k, i)].dtype == dtype and z["%s_%d" % (k, i)].shape == shape, (k, i)
            assert np.array_equal(z["%s_%d" % (k, i)], out["%s_%d" % (k, i)], equal_nan=True)
        assert str(z["name_%d" % i]) == mols[i]["name"]
        med = z["medoid_%d" % i]
        assert np.array_equal(z["cluster_%d" % i][med], np.arange(2)) and z["count_%d" % i].sum() == G and z["converged_%d" % i] == 1
        assert np.array_equal(z["pos_%d" % i][0], g[med[0]]) and z["within_%d" % i].sum() == z["cost_%d" % i]
        assert z["cost_%d" % i] <= z["build_cost_%d" % i]
        assert np.array_equal(z["population_%d" % i], z["count_%d" % i].astype(F32) / F32(G))
    # molecules 1 and 2 are two tight families each, the even and the odd conformers: one medoid in each
    for i in (1, 2):
        assert sorted(z["medoid_%d" % i] % 2) == [0, 1] and np.array_equal(z["cluster_%d" % i] == z["cluster_%d" % i][0],
                                                                          np.arange(gens[i].shape[0]) % 2 == 0)
        assert z["dist_%d" % i].max() < 0.2
    first = pam.main(base + ["--count", "2", "--init", "first", "--max-swaps", "0", "--out", str(tmp_path / "first.npz")])
    assert "PAM from first, 0 swaps, at most 0 per molecule; 3 molecules did not converge" in capsys.readouterr().out
    assert all(first["swaps_%d" % i] == 0 and first["medoid_%d" % i].tolist() == [0, 1] for i in range(3))
    assert not any(k.startswith("build_cost") for k in first)
    tfd = pam.main(base + ["--count", "2", "--tfd", "--init", "alternate", "--drop-invalid", "--out", str(tmp_path / "tfd.npz")])
    assert "TFD" in capsys.readouterr().out and all(tfd["cluster_%d" % i].shape == (gens[i].shape[0],) for i in range(3))
    for i in range(3):
        assert np.array_equal(tfd["cluster_%d" % i] == -1, tfd["valid_%d" % i] == 0)
    # python -m agdiff_amd.silhouette scores the file as it is
    sil = silhouette.main(base + ["--labels", str(tmp_path / "pam.npz"), "--out", str(tmp_path / "sil.npz")])
    assert "labels cluster of" in capsys.readouterr().out
    for i in range(3):
        assert np.array_equal(sil["count_%d" % i], z["count_%d" % i]) and sil["sil_%d" % i].shape == (gens[i].shape[0],)
    for i in (1, 2):                                         # two tight families far apart
        assert sil["sil_mean_%d" % i] > 0.8
