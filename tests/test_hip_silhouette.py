"""GPU (MI355X): silhouette coefficients (agdiff_amd.silhouette; csrc/eval.hip: k_sil_*) against the numpy restatement of the rule
(tests/silhouette_ref.py) on the same float32 matrix -- integers equal, doubles bit-equal, NaN at the same places, status
included -- and end to end through silhouette_conformers, sweep_medoids and the command line.

Every sum the kernels make is a sum of integers (the matrix entries on a 2^-28 grid, the coefficients on a 2^-40 grid) and every
double they write is one correctly rounded division of two such integers, an exact scaling of one, or one subtraction and one
division of two of them, so every comparison with the restatement is exact.  The one tolerance is ALIGN_ATOL, for the superposed
medoids of the sweep: the bar that tests/test_hip_clusters.py carries for agdiff_align_conformers; nothing new is measured here."""
import functools

import numpy as np
import pytest
import torch

import kmedoids_ref as KR
import silhouette_ref as SR
import tfd_ref as TR
from test_hip_clusters import ALIGN_ATOL, _families, _kabsch_align, _moved, seven_pattern_conformers

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL, FSENTINEL, TAIL = -7, -777.0, 64           # (no output is -7 or -777: integers are >= -1, doubles >= -1 or NaN)
WAVE_ROW_MAX_K = 1024                                # the launcher's threshold: one row per wave up to here, one per workgroup above


def _launch(dist, G, labels, K):
    """agdiff_silhouette on a device tensor [G, G] (or a numpy matrix), its eight arrays filled with a sentinel and followed by a
    canary tail, the scratch followed by one too: every entry must have been written, the tails and the labels must be as they
    were.  The result in the restatement's form."""
    from agdiff_amd import _lib
    dev = dist if torch.is_tensor(dist) else torch.from_numpy(np.array(dist, dtype=F32)).cuda()
    given = np.array(labels, dtype=np.int32)
    lab = torch.from_numpy(given.copy()).cuda()
    full = lambda m, v, dtype: torch.full((m + TAIL,), v, dtype=dtype, device="cuda")
    a, b, s, cmean, mean = (full(m, FSENTINEL, torch.float64) for m in (G, G, G, K, 1))
    other, size, status = (full(m, SENTINEL, torch.int32) for m in (G, K, 1))
    words = _lib.DEFINES["AGDIFF_SILHOUETTE_WORK_BYTES"] // 8
    work = full(words, SENTINEL, torch.int64)
    _lib.call("agdiff_silhouette", dev, G, K, lab, a, b, s, other, size, cmean, mean, status, work)
    assert (work[words:] == SENTINEL).all() and np.array_equal(lab.cpu().numpy(), given)
    out = []
    for x, m, v in ((a, G, FSENTINEL), (b, G, FSENTINEL), (s, G, FSENTINEL), (other, G, SENTINEL), (size, K, SENTINEL),
                    (cmean, K, FSENTINEL), (mean, 1, FSENTINEL), (status, 1, SENTINEL)):
        x = x.cpu().numpy()
        assert (x[m:] == v).all() and not (x[:m] == v).any()
        out.append(x[:m])
    a, b, s, other, size, cmean, mean, status = out
    assert ((other >= -1) & (other < K)).all() and ((size >= 0) & (size <= G)).all() and status[0] in (0, 2)
    return a, b, s, other, size, cmean, mean[0], int(status[0])


@functools.lru_cache(maxsize=None)
def _case(name, *args):
    """(matrix, its fixed-point image, the same matrix on the device) of a named structured matrix -- made once, left unchanged"""
    d = getattr(SR, name)(*args) if name != "metric" else SR.random_metric(args[0], seed=args[0])
    d.setflags(write=False)
    q = SR.Q(d)
    q.setflags(write=False)
    return d, q, torch.from_numpy(np.array(d)).cuda()


def _both(case, labels, K):
    d, q, dev = case
    want = SR.silhouette(d, labels, K, q=q)
    got = _launch(dev, d.shape[0], labels, K)
    assert SR.same(got, want), "G = %d, K = %d, labels = %s ...: got %s, want %s" % (
        d.shape[0], K, list(labels)[:8], [np.asarray(x).reshape(-1)[:6] for x in got], [np.asarray(x).reshape(-1)[:6] for x in want])
    return got


def _on(d):
    return d, None, torch.from_numpy(np.array(d, dtype=F32)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the kernels against the rule
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096]
SHAPES = sorted({(G, K) for G in SIZES for K in {1, 2, min(7, G), min(100, G)} | ({G} if G <= 257 else set())}
                | {(4096, 4096), (5, 4096)}
                | {(G, K) for G in (257, 1025) for K in range(WAVE_ROW_MAX_K - 1, WAVE_ROW_MAX_K + 3)})


def _label_families(d, q, G, K):
    """the clusterings of one (G, K): name -> labels"""
    rng = np.random.default_rng(1000 * G + K)
    uniform = rng.integers(0, K, size=G)
    fam = {"uniform": uniform}
    if K <= WAVE_ROW_MAX_K:                                  # (above: the restated k-medoids walk is what takes the time, not the kernel)
        seeds = KR.maxmin(d, min(K, G))[0]
        fam["k-medoids from MaxMin seeds"] = KR.kmedoids(d, seeds[seeds >= 0].tolist(), q=q)[1]
    giant = np.zeros(G, dtype=np.int64)
    singles = min(K - 1, G - 1)
    if singles > 0:
        giant[G - singles:] = np.arange(1, singles + 1)
    fam["one giant cluster plus singletons"] = giant
    fam["a tenth left out"] = np.where(rng.random(G) < 0.1, -1, uniform)
    allowed = np.array([c for c in range(K) if c % 3 != 1] or [0])
    fam["a third of the ranks empty"] = allowed[rng.integers(0, allowed.size, size=G)]
    fam["everybody left out"] = np.full(G, -1)
    return fam


@pytest.mark.parametrize("G, K", SHAPES)
def test_kernels_equal_the_restated_rule(G, K):
    """across a wave, a workgroup of the rows kernel (4 rows), odd sizes and the limit; K = 1, K above G, every conformer its own
    rank, and K on both sides of the threshold at which the rows kernel goes from one row per wave to one per workgroup"""
    case = _case("metric", G)
    for name, labels in _label_families(case[0], case[1], G, K).items():
        a, b, s, other, size, cmean, mean, status = _both(case, labels, K)
        ok = np.asarray(labels) >= 0
        assert status == 0 and size.sum() == ok.sum() and np.array_equal(np.isnan(s), ~ok), name
        assert ((s[ok] >= -1) & (s[ok] <= 1)).all(), name
        if name == "everybody left out":
            assert np.isnan(mean) and np.isnan(cmean).all() and not size.any() and (other == -1).all()
        if name == "one giant cluster plus singletons" and K > 1 and G > 1:
            assert (s[np.asarray(labels) > 0] == 0).all() and size[0] == G - min(K - 1, G - 1)      # a singleton scores 0
        if K == 1:
            assert (other == -1).all() and np.isnan(b).all() and not s[ok].any()


def test_two_launches_give_equal_bytes_through_the_wrapper():
    from agdiff_amd.silhouette import silhouette
    for G, K in ((1000, 100), (4096, 10), (300, 2000)):
        d, q, dev = _case("metric", G)
        labels = np.random.default_rng(G).integers(0, K, size=G).astype(np.int32)
        lab = torch.from_numpy(labels).cuda()
        x, y = silhouette(dev, G, lab, K), silhouette(dev, G, lab, K)
        for u, v, dtype, m in zip(x, y, (torch.float64,) * 3 + (torch.int32, torch.int32, torch.float64, torch.float64, torch.int32),
                                  (G, G, G, G, K, K, 1, 1)):
            assert u.dtype == dtype and tuple(u.shape) == (m,) and u.is_cuda
            assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
        assert SR.same([t.cpu().numpy() for t in x[:6]] + [x[6].cpu().numpy()[0], int(x[7])], SR.silhouette(d, labels, K, q=q))


# ------------------------------------------------------------------------------------------------ 2. structured matrices
@pytest.mark.parametrize("shape, K", [((9, 7), 3), ((9, 7), 9), ((33, 31), 4), ((33, 31), 33)])
def test_lattice_ties_go_to_the_lowest_rank(shape, K):
    """integer distances and clusters of equal sizes: many conformers have two other clusters at exactly the same mean"""
    case = _case("lattice", *shape)
    G = case[0].shape[0]
    for seed in range(3):
        labels = np.random.default_rng(seed).permutation(np.arange(G) % K)
        _both(case, labels, K)
    stripes, K = np.arange(G) % shape[1], shape[1]                          # one rank per column of the lattice: the two neighbouring columns tie
    a, b, s, other, size, cmean, mean, status = _both(case, stripes, K)
    q, n = case[1], size.astype(np.float64)
    tied = 0
    for i in range(0, G, max(G // 40, 1)):                                  # ties are really there, and the lowest rank has them
        m = np.array([q[i, (stripes == c) & (np.arange(G) != i)].sum(dtype=np.uint64) for c in range(K)]).astype(np.float64) / n
        m[stripes[i]] = np.inf
        tied += (m == m.min()).sum() > 1
        assert other[i] == int(np.argmin(m))
    assert tied >= 5


@pytest.mark.parametrize("G", [65, 257, 1025])
def test_invalid_entries_count_as_the_cap(G):
    base = _case("metric", G)[0]
    bad = sorted({1, G // 3, G - 1, 64} & set(range(1, G)))
    d = SR.with_inf(base, bad)
    rng = np.random.default_rng(G)
    for K in (2, 7):
        labels = rng.integers(0, K, size=G)
        a, b, s, other, size, cmean, mean, status = _both(_on(d), labels, K)
        assert (a[bad] > 2048).all() and (b[bad] == 4096).all()              # every entry of a bad row counts as 4096
        left = labels.copy()
        left[bad] = -1                                                        # left out, the +inf columns are not read
        got = _both(_on(d), left, K)
        clean = _both(_on(base), left, K)
        assert SR.same(got, clean)
    for value in (np.nan, -1.0, 5000.0, np.inf, -np.inf, np.nextafter(F32(4096), F32(np.inf))):
        e = np.array(base)
        e[5, 6] = e[6, 5] = e[G - 1, G - 2] = e[7, 0] = value
        _both(_on(e), rng.integers(0, 3, size=G), 3)
    capped = np.array(base)
    capped[5, 6] = capped[6, 5] = 4096.0
    _both(_on(capped), rng.integers(0, 3, size=G), 3)


@pytest.mark.parametrize("G", [64, 257])
def test_zero_matrices_minus_zero_and_asymmetry(G):
    rng = np.random.default_rng(G)
    labels = rng.integers(0, 5, size=G)
    a, b, s, other, size, cmean, mean, status = _both(_on(np.zeros((G, G), F32)), labels, 5)
    assert not a.any() and not b.any() and not s.any() and mean == 0 and not cmean.any()      # max(a, b) == 0: s = 0
    assert np.array_equal(other, np.where(labels == 0, 1, 0))                                 # every mean ties at 0: the lowest rank
    d = np.array(_case("metric", G)[0])
    dup = rng.choice(G, size=G // 4, replace=False)
    d[dup[:, None], dup[None, :]] = -0.0                     # a clique of duplicates at distance -0.0, diagonal included
    got = _both(_on(d), labels, 5)
    assert SR.same(got, SR.silhouette(np.where(d == 0, F32(0), d), labels, 5)) and not np.signbit(got[0]).any()
    # an asymmetric matrix: row i is what is read
    asym = rng.uniform(0.5, 3.0, size=(G, G)).astype(F32)
    got = _both(_on(asym), labels, 5)
    back = _both(_on(asym.T.copy()), labels, 5)
    assert not SR.same(got[:3], back[:3])
    diag = np.array(asym)
    diag[np.arange(G), np.arange(G)] = np.nan               # the diagonal is never read
    assert SR.same(_both(_on(diag), labels, 5), got)


@pytest.mark.parametrize("G", [63, 1025])
def test_matrix_one_float_into_its_allocation(G):
    """dist needs 4-byte alignment only; with G odd no row of it is 8-byte aligned"""
    d, q, _ = _case("metric", G)
    buf = torch.full((G * G + 2,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    off = buf[1:1 + G * G].view(G, G)
    off.copy_(torch.from_numpy(np.array(d)))
    assert off.data_ptr() % 8 == 4 and off.is_contiguous()
    for K in (3, 40):
        _both((d, q, off), np.random.default_rng(K).integers(0, K, size=G), K)


# ------------------------------------------------------------------------------------------------ 3. bad labels, nothing to do
@pytest.mark.parametrize("G, K", [(9, 3), (300, 7), (1025, 2000)])
def test_a_bad_label_gives_status_two(G, K):
    """an ordinary input with a defined result: the kernel checks the labels and fills every output"""
    case = _case("metric", G)
    good = np.random.default_rng(G).integers(-1, K, size=G)
    assert _both(case, good, K)[7] == 0
    for where in (0, G // 2, G - 1):
        for value in (K, -2, 1 << 30, -(1 << 31)):
            labels = good.copy()
            labels[where] = value
            a, b, s, other, size, cmean, mean, status = _both(case, labels, K)
            assert status == 2 and np.isnan(a).all() and np.isnan(b).all() and np.isnan(s).all() and (other == -1).all()
            assert not size.any() and np.isnan(cmean).all() and np.isnan(mean)


def test_no_conformers_is_no_launch():
    from agdiff_amd import _lib
    K = 5
    size, status = (torch.full((m + TAIL,), SENTINEL, dtype=torch.int32, device="cuda") for m in (K, 1))
    cmean, mean = (torch.full((m + TAIL,), FSENTINEL, dtype=torch.float64, device="cuda") for m in (K, 1))
    ints = torch.full((TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    doubles = torch.full((TAIL,), FSENTINEL, dtype=torch.float64, device="cuda")
    work = torch.full((TAIL,), SENTINEL, dtype=torch.int64, device="cuda")
    dist = torch.zeros(1, dtype=torch.float32, device="cuda")
    _lib.call("agdiff_silhouette", dist, 0, K, ints, doubles, doubles, doubles, ints, size, cmean, mean, status, work)
    assert size.cpu().tolist() == [0] * K + [SENTINEL] * TAIL and status.cpu().tolist() == [0] + [SENTINEL] * TAIL
    cmean, mean = cmean.cpu().numpy(), mean.cpu().numpy()
    assert np.isnan(cmean[:K]).all() and (cmean[K:] == FSENTINEL).all() and np.isnan(mean[0]) and (mean[1:] == FSENTINEL).all()
    assert (ints == SENTINEL).all() and (doubles == FSENTINEL).all() and (work == SENTINEL).all()


def test_wrapper_refuses_what_the_header_refuses():
    from agdiff_amd import _lib
    from agdiff_amd.silhouette import silhouette
    G = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1
    with pytest.raises(_lib.AgdiffLimitError):
        silhouette(torch.zeros((G, G), dtype=torch.float32, device="cuda"), G, torch.zeros(G, dtype=torch.int32, device="cuda"), 1)
    small = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    lab = torch.zeros(4, dtype=torch.int32, device="cuda")
    for bad in (lambda: silhouette(torch.zeros((4, 5), dtype=torch.float32, device="cuda"), 4, lab, 1), lambda: silhouette(small.double(), 4, lab, 1),
                lambda: silhouette(small, 4, lab.long(), 1), lambda: silhouette(small, 4, lab.cpu(), 1), lambda: silhouette(small, 4, lab[:3], 1),
                lambda: silhouette(small, 4, lab, 0), lambda: silhouette(small, 4, lab, 4097), lambda: silhouette(small, 4, lab, 1.5)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ 4. planted answers, in plain numbers
def test_two_tight_families_score_high_and_a_random_split_scores_low():
    rng = np.random.default_rng(3)
    G = 90
    family = (np.arange(G) >= 50).astype(np.int64)
    x = (np.array([[0.0, 0, 0], [10.0, 0, 0]])[family] + 0.05 * rng.normal(size=(G, 3))).astype(F32)
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)).astype(F32)
    a, b, s, other, size, cmean, mean, status = _both(_on(d), family, 2)
    assert (s > 0.9).all() and mean > 0.9 and size.tolist() == [50, 40] and np.array_equal(other, 1 - family)
    split = np.where((family == 0) & (rng.random(G) < 0.5), 2, family)       # family 0 cut in two at random
    a2, b2, s2, other2, size2, cmean2, mean2, _ = _both(_on(d), split, 3)
    assert (s2[family == 0] < 0.5).all() and (s2[family == 0] < 0).any() and mean2 < mean - 0.3
    assert (s2[family == 1] > 0.9).all() and cmean2[1] > 0.9                 # the untouched family still scores high


# ------------------------------------------------------------------------------------------------ 5. end to end
def _seven():
    at, bonds, gen, thr = seven_pattern_conformers(np.random.default_rng(9))
    _, bi, bt = TR.graph(at, bonds)
    return dict(atom_type=at, bond_index=bi, bond_type=bt, pos_gen=gen), gen, thr


def _check_result(res, want, values, G, sel=None):
    """a silhouette_conformers result against the restatement run on the matrix of the usable conformers (`sel`: their indices in
    the item) with ranks; `values`: the caller's label of each rank"""
    a, b, s, other, size, cmean, mean, status = want
    K = len(values)
    sel = np.arange(G) if sel is None else np.asarray(sel)
    for key, dtype, shape in (("s", torch.float64, (G,)), ("a", torch.float64, (G,)), ("b", torch.float64, (G,)), ("other", torch.int32, (G,)),
                              ("count", torch.int32, (K,)), ("cluster_mean", torch.float64, (K,))):
        assert res[key].dtype == dtype and tuple(res[key].shape) == shape and res[key].is_cuda, key
    assert isinstance(res["mean"], float) and SR.same((np.float64(res["mean"]),), (mean,)) and status == 0
    assert isinstance(res["values"], np.ndarray) and res["values"].tolist() == list(values)
    full = [np.full(G, np.nan), np.full(G, np.nan), np.full(G, np.nan), np.full(G, -1, np.int32)]
    for f, x in zip(full[:3], (a, b, s)):
        f[sel] = x
    if K:
        full[3][sel] = np.where(other >= 0, np.asarray(values)[np.maximum(other, 0)], -1)
    assert SR.same([res[k].cpu().numpy() for k in ("a", "b", "s", "other", "count", "cluster_mean")], full + [size, cmean])


@pytest.mark.parametrize("metric, rings", [("rmsd", False), ("tfd", False), ("tfd", True)])
def test_seven_pattern_equals_the_restatement_on_the_devices_matrix(metric, rings):
    from agdiff_amd.clusters import cluster_conformers
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.silhouette import silhouette_conformers
    from agdiff_amd.torsions import tfd_self
    item, gen, thr = _seven()
    G = gen.shape[0]
    matrix = (self_rmsd_matrix(item) if metric == "rmsd" else tfd_self(item, rings=rings)[0]).cpu().numpy()
    kw = dict(metric=metric, tfd_rings=rings)
    if metric == "tfd":
        thr = float(np.median(matrix[np.triu_indices(G, 1)]))
    found = cluster_conformers(item, thr, align=False, **kw)
    ranks, leader = found["cluster"].cpu().numpy(), found["leader"].cpu().numpy()
    K = int(ranks.max()) + 1
    want = SR.silhouette(matrix, ranks, K)
    _check_result(silhouette_conformers(item, found["cluster"], **kw), want, list(range(K)), G)       # a device tensor of ranks
    _check_result(silhouette_conformers(item, ranks.astype(np.int64), **kw), want, list(range(K)), G)
    # the same clustering named by its centroids (what python -m agdiff_amd.ensemble writes): ranks in ascending order of the names
    values = sorted(set(leader.tolist()))
    by_name = np.searchsorted(values, leader)
    _check_result(silhouette_conformers(item, leader, **kw), SR.silhouette(matrix, by_name, K), values, G)
    for labels in ([0, 0, 1, 1, 2, 2, -1], [5] * 7, [-1] * 7, [3, 1, 4, 1, 5, 9, 2]):
        values = np.unique(np.array([l for l in labels if l >= 0], dtype=np.int64))
        ranks = np.where(np.array(labels) >= 0, np.searchsorted(values, labels), -1)
        want = SR.silhouette(matrix, ranks, max(len(values), 1))
        if len(values) == 0:
            want = want[:4] + (want[4][:0], want[5][:0]) + want[6:]
        _check_result(silhouette_conformers(item, labels, **kw), want, values.tolist(), G)


def test_families_with_masked_and_broken_conformers():
    from agdiff_amd.clusters import cluster_conformers
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.silhouette import silhouette_conformers
    n, K, G = 20, 4, 37
    item, label, gen, heavy = _families(n, K, G)
    matrix = self_rmsd_matrix(item).cpu().numpy()
    found = cluster_conformers(item, 0.5, align=False)
    ranks = found["cluster"].cpu().numpy()
    res = silhouette_conformers(item, ranks)
    _check_result(res, SR.silhouette(matrix, ranks, K), list(range(K)), G)
    assert float(res["s"].min()) > 0.8 and res["mean"] > 0.9 and res["count"].cpu().tolist() == [16, 11, 7, 3]   # tight families, far apart
    _check_result(silhouette_conformers(item, label), SR.silhouette(matrix, label, K), list(range(K)), G)       # the planted labels themselves
    valid = np.ones(G, dtype=bool)
    valid[label == 2] = False                                # one whole family: its rank stays, empty
    valid[[0, 5]] = False
    sel = np.nonzero(valid)[0]
    sub = self_rmsd_matrix(dict(item, pos_gen=gen[sel])).cpu().numpy()
    want = SR.silhouette(sub, label[sel], K)
    for mask in (valid, torch.from_numpy(valid).cuda()):
        res = silhouette_conformers(item, label, valid=mask)
        _check_result(res, want, list(range(K)), G, sel=sel)
        assert bool(torch.isnan(res["s"][~torch.from_numpy(valid)]).all()) and (res["other"][~torch.from_numpy(valid)] == -1).all()
        assert res["count"][2] == 0 and bool(torch.isnan(res["cluster_mean"][2])) and not (res["other"] == 2).any()
    broken = gen.copy()                                      # a coordinate that is not finite: left out like a masked one
    broken[0, 3, 1], broken[5, 0, 0] = np.nan, np.inf
    for c in np.nonzero(label == 2)[0]:
        broken[c, -1, 2] = -np.inf
    _check_result(silhouette_conformers(dict(item, pos_gen=broken), label), want, list(range(K)), G, sel=sel)
    none = silhouette_conformers(item, label, valid=np.zeros(G, dtype=bool))
    assert bool(torch.isnan(none["s"]).all()) and (none["other"] == -1).all() and none["count"].tolist() == [0] * K and np.isnan(none["mean"])
    assert none["s"].shape == (G,) and none["cluster_mean"].shape == (K,) and bool(torch.isnan(none["cluster_mean"]).all())


@functools.lru_cache(maxsize=None)
def _three_families():
    """(item, family [G], gen): three tight families (0.03 Angstrom of noise) of 14, 10 and 6 conformers of a 12-atom molecule, every
    member moved rigidly"""
    rng = np.random.default_rng(33)
    n, sizes = 12, [14, 10, 6]
    centres = rng.normal(size=(3, n, 3)) * 1.5
    family = rng.permutation(np.repeat(np.arange(3), sizes))
    gen = np.stack([_moved(rng, centres[c] + 0.03 * rng.normal(size=(n, 3))) for c in family]).astype(F32)
    return {"atom_type": np.full(n, 6), "pos_gen": gen}, family, gen


def test_sweep_finds_three_planted_families():
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.medoids import medoid_conformers
    from agdiff_amd.silhouette import sweep_medoids
    item, family, gen = _three_families()
    G = gen.shape[0]
    matrix = self_rmsd_matrix(item).cpu().numpy()
    for init in ("maxmin", "first"):
        res = sweep_medoids(item, 2, 6, init=init)
        assert res["k"].tolist() == [2, 3, 4, 5, 6] and res["k"].dtype == np.int32 and res["mean"].dtype == np.float64
        assert res["cost"].dtype == np.float64 and res["iters"].dtype == np.int32 and res["converged"].dtype == np.bool_
        seeds = KR.maxmin(matrix, 6)[0] if init == "maxmin" else np.arange(6)
        for j, K in enumerate(range(2, 7)):                  # every curve entry: restated k-medoids, then the restated silhouette
            walk = KR.kmedoids(matrix, seeds[:K].tolist())
            sil = SR.silhouette(matrix, walk[1], K)
            assert SR.same((res["mean"][j], res["cost"][j]), (sil[6], walk[5])), (init, K)
            assert res["iters"][j] == walk[6] and res["converged"][j] == (walk[7] == 0)
            if K == res["best_k"]:
                _check_result(res["silhouette"], sil, list(range(K)), G)
        best = int(np.argmax(res["mean"]))                   # (argmax: the first of equal maxima, i.e. the smallest K)
        assert res["best_k"] == res["k"][best]
        want = medoid_conformers(item, res["best_k"], init=init)
        assert set(want) == set(res["medoids"])
        for key, value in want.items():                      # tensor for tensor
            if torch.is_tensor(value):
                assert value.dtype == res["medoids"][key].dtype and torch.equal(value.view(torch.uint8), res["medoids"][key].view(torch.uint8)), key
            else:
                assert value == res["medoids"][key] and type(value) is type(res["medoids"][key]), key
        if init == "maxmin":                                 # MaxMin seeds put one medoid in each family
            assert res["best_k"] == 3 and res["mean"][1] > 0.9 and res["mean"][0] < res["mean"][1] - 0.1 and res["mean"][2] < res["mean"][1] - 0.1
            labels = res["medoids"]["labels"].cpu().numpy()
            assert np.array_equal(family[res["medoids"]["medoids"].cpu().numpy()][labels], family)
            med = res["medoids"]["medoids"].cpu().numpy()
            aligned = np.stack([_kabsch_align(gen[c], gen[med[0]], np.arange(gen.shape[1])) for c in med])
            assert np.abs(res["medoids"]["pos"].cpu().numpy() - aligned).max() <= ALIGN_ATOL
    # the range is clamped to the usable conformers; with fewer than k_min of them no K is run
    valid = np.zeros(G, dtype=bool)
    valid[:4] = True
    few = sweep_medoids(item, 3, 9, valid=valid, align=False)
    assert few["k"].tolist() == [3, 4] and few["medoids"]["labels"].shape == (G,) and few["silhouette"]["s"].shape == (G,)
    valid[2:] = False
    none = sweep_medoids(item, 3, 9, valid=valid)
    assert none["k"].shape == (0,) and none["best_k"] == 0 and none["medoids"] is None and none["silhouette"] is None


def test_command_line_round_trip(tmp_path, capsys):
    from agdiff_amd import clusters, driver, silhouette, synth
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
    found = clusters.main(base + ["--rms", str(thr), "--out", str(tmp_path / "clusters.npz")])
    capsys.readouterr()
    out = silhouette.main(base + ["--labels", str(tmp_path / "clusters.npz"), "--out", str(tmp_path / "sil.npz")])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and "silhouette of 19 conformers by RMSD" in line[0] and "mean over 3 molecules" in line[0]
    z = np.load(str(tmp_path / "sil.npz"))
    keys = ("sil", "sil_a", "sil_b", "sil_other", "sil_cluster", "sil_mean", "count", "name")
    assert set(z.files) == {"%s_%d" % (k, i) for k in keys for i in range(3)} == set(out)
    for i, g in enumerate(gens):
        G, K = g.shape[0], int(found["cluster_%d" % i].max()) + 1
        for k, dtype, shape in (("sil", np.float64, (G,)), ("sil_a", np.float64, (G,)), ("sil_b", np.float64, (G,)), ("sil_other", np.int32, (G,)),
                                ("sil_cluster", np.float64, (K,)), ("sil_mean", np.float64, ()), ("count", np.int32, (K,))):
            assert z["%s_%d" % (k, i)].dtype == dtype and z["%s_%d" % (k, i)].shape == shape, (k, i)
            assert np.array_equal(z["%s_%d" % (k, i)], out["%s_%d" % (k, i)], equal_nan=True)
        assert str(z["name_%d" % i]) == mols[i]["name"] and np.array_equal(z["count_%d" % i], found["count_%d" % i])
    for i in (1, 2):                                         # two tight families each, the even and the odd conformers
        assert z["sil_%d" % i].min() > 0.9 and z["sil_mean_%d" % i] > 0.9 and np.array_equal(z["sil_other_%d" % i], 1 - found["cluster_%d" % i])
    by_leader = silhouette.main(base + ["--labels", str(tmp_path / "clusters.npz"), "--label-key", "leader", "--out", str(tmp_path / "l.npz")])
    capsys.readouterr()
    assert all(np.array_equal(by_leader["sil_%d" % i], out["sil_%d" % i]) for i in (1, 2))
    sweep = silhouette.main(base + ["--sweep", "2", "6", "--align", "--out", str(tmp_path / "sweep.npz")])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and "k-medoids for K = 2 .. 6, maxmin seeds" in line[0] and "best K:" in line[0] and "x K = 2" in line[0]
    z = np.load(str(tmp_path / "sweep.npz"))
    more = ("sweep_k", "sweep_sil", "sweep_cost", "best_k", "medoid", "cluster", "dist", "population", "within", "cost", "iters", "converged",
            "pos")
    assert set(z.files) == {"%s_%d" % (k, i) for k in keys + more for i in range(3)} == set(sweep)
    for i, g in enumerate(gens):
        G, n, hi = g.shape[0], g.shape[1], min(6, g.shape[0])
        K = int(z["best_k_%d" % i])
        assert z["sweep_k_%d" % i].tolist() == list(range(2, hi + 1)) and z["sweep_k_%d" % i].dtype == np.int32
        assert z["best_k_%d" % i].dtype == np.int32 and z["best_k_%d" % i].shape == ()
        for k, dtype, shape in (("sweep_sil", np.float64, (hi - 1,)), ("sweep_cost", np.float64, (hi - 1,)), ("medoid", np.int32, (K,)),
                                ("cluster", np.int32, (G,)), ("dist", np.float32, (G,)), ("count", np.int32, (K,)),
                                ("population", np.float32, (K,)), ("within", np.float64, (K,)), ("cost", np.float64, ()),
                                ("iters", np.int32, ()), ("converged", np.int8, ()), ("pos", np.float32, (K, n, 3)),
                                ("sil", np.float64, (G,)), ("sil_a", np.float64, (G,)), ("sil_b", np.float64, (G,)),
                                ("sil_other", np.int32, (G,)), ("sil_cluster", np.float64, (K,)), ("sil_mean", np.float64, ())):
            assert z["%s_%d" % (k, i)].dtype == dtype and z["%s_%d" % (k, i)].shape == shape, (k, i)
        assert z["sil_mean_%d" % i] == z["sweep_sil_%d" % i][K - 2] == z["sweep_sil_%d" % i].max()
        assert z["cost_%d" % i] == z["sweep_cost_%d" % i][K - 2] and z["count_%d" % i].sum() == G
    assert z["best_k_1"] == 2 and z["best_k_2"] == 2 and np.array_equal(z["sil_1"], out["sil_1"][np.arange(7)])
    more = silhouette.main(base + ["--sweep", "2", "3", "--drop-invalid", "--out", str(tmp_path / "checked.npz")])
    capsys.readouterr()
    for i in range(3):
        assert more["valid_%d" % i].dtype == np.int8 and np.array_equal(np.isnan(more["sil_%d" % i]), more["valid_%d" % i] == 0)
    tfd = silhouette.main(base + ["--sweep", "2", "3", "--tfd", "--init", "first", "--out", str(tmp_path / "tfd.npz")])
    assert "by TFD (k-medoids for K = 2 .. 3, first seeds)" in capsys.readouterr().out and all(tfd["sil_%d" % i].shape == (gens[i].shape[0],) for i in range(3))
