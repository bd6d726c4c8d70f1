"""GPU (MI355X): agglomerative linkage and its cuts (agdiff_amd.linkage; csrc/eval.hip: k_link_*) against the numpy restatement of
the rule (tests/linkage_ref.py) on the same float32 matrix -- integers equal, doubles bit-equal, NaN at the same places -- and end
to end through linkage_conformers, sweep_linkage and the command line.

Every minimum, maximum and sum the tree makes is one of integers (the matrix entries on a 2^-28 grid), a mean is one correctly
rounded fp64 division of two exactly stated operands, and every float a cut writes is a copy of a matrix entry or such a sum divided
by 2^28, so every comparison with the restatement is exact.  The one tolerance is ALIGN_ATOL, for the superposed medoids against a
float64 Kabsch of the same fp32 inputs: the bar that tests/test_hip_clusters.py carries for agdiff_align_conformers, the same kernel
under the same bar; nothing new is measured here."""
import functools

import numpy as np
import pytest
import torch

import linkage_ref as LR
import tfd_ref as TR
from test_hip_clusters import ALIGN_ATOL, _families, _kabsch_align, _moved, seven_pattern_conformers

pytestmark = pytest.mark.gpu
F32 = np.float32
METHODS = ("single", "complete", "average")
SENTINEL, FSENTINEL, TAIL = -7, -777.0, 64           # (no output is negative but the -1 of the fills)


def _full(m, v, dtype):
    return torch.full((m + TAIL,), v, dtype=dtype, device="cuda")


def _checked(arrays):
    """the first m entries of each (tensor, m, sentinel): all written, the canary tail as it was"""
    out = []
    for a, m, s in arrays:
        a = a.cpu().numpy()
        assert (a[m:] == s).all() and not (a[:m] == s).any()
        out.append(a[:m])
    return out


def _tree(dev, G, method, anchor=0, fill=SENTINEL):
    """agdiff_linkage on a device tensor [G, G]: the outputs filled with a sentinel and followed by a canary tail, the scratch
    filled with `fill` and followed by one too.  The result in the restatement's form."""
    from agdiff_amd import _lib
    left, right, size, order, status = (_full(m, SENTINEL, torch.int32) for m in (G, G, G, G, 1))
    height = _full(G, FSENTINEL, torch.float64)
    words = G * G + _lib.DEFINES["AGDIFF_LINKAGE_WORK_FIXED_BYTES"] // 8
    work = _full(words, fill, torch.int64)
    _lib.call("agdiff_linkage", dev, G, METHODS.index(method), int(anchor), left, right, height, size, order, status, work)
    assert (work[words:] == fill).all()
    left, right, height, size, order, status = _checked(((left, G, SENTINEL), (right, G, SENTINEL), (height, G, FSENTINEL),
                                                         (size, G, SENTINEL), (order, G, SENTINEL), (status, 1, SENTINEL)))
    return left, right, height, size, order, int(status[0])


def _cut(dev, G, tree, count=1, stop=np.inf):
    """agdiff_linkage_cut of a tree in the restatement's form, its outputs sentinel-filled with canary tails"""
    from agdiff_amd import _lib
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    left, right, height, order = on(tree[0]), on(tree[1]), on(tree[2]), on(tree[4])
    medoids, labels, size, n, status = (_full(m, SENTINEL, torch.int32) for m in (G, G, G, 1, 1))
    near = _full(G, FSENTINEL, torch.float32)
    within, cost = _full(G, FSENTINEL, torch.float64), _full(1, FSENTINEL, torch.float64)
    words = _lib.DEFINES["AGDIFF_LINKAGE_CUT_WORK_BYTES"] // 8
    work = _full(words, SENTINEL, torch.int64)
    _lib.call("agdiff_linkage_cut", dev, G, left, right, height, order, int(count), float(stop), medoids, labels, near, size, within,
              cost, n, status, work)
    assert (work[words:] == SENTINEL).all()
    for a, b in ((left, tree[0]), (right, tree[1]), (order, tree[4])):               # the tree is read only
        assert np.array_equal(a.cpu().numpy(), b)
    medoids, labels, near, size, within, cost, n, status = _checked(
        ((medoids, G, SENTINEL), (labels, G, SENTINEL), (near, G, FSENTINEL), (size, G, SENTINEL), (within, G, FSENTINEL),
         (cost, 1, FSENTINEL), (n, 1, SENTINEL), (status, 1, SENTINEL)))
    return medoids, labels, near, size, within, cost[0], int(n[0]), int(status[0])


@functools.lru_cache(maxsize=None)
def _case(name, *args):
    """(matrix, its fixed-point image, the same matrix on the device) of a named matrix -- made once, left unchanged"""
    d = LR.random_metric(args[0], seed=args[0]) if name == "metric" else getattr(LR, name)(*args)
    d.setflags(write=False)
    q = LR.Q(d)
    q.setflags(write=False)
    return d, q, torch.from_numpy(np.array(d)).cuda()


def _fresh(d):
    d = np.ascontiguousarray(d, dtype=F32)
    return d, LR.Q(d), torch.from_numpy(d.copy()).cuda()


@functools.lru_cache(maxsize=None)
def _want(name, args, method):
    d, q, _ = _case(name, *args)
    return LR.linkage(d, method, q=q)


def _describe(t):
    n = int((t[0] >= 0).sum())
    return n, t[0][:6], t[1][:6], t[2][:6], t[5]


def _both_tree(case, method, anchor=0, want=None):
    d, q, dev = case
    want = LR.linkage(d, method, anchor, q=q) if want is None else want
    got = _tree(dev, d.shape[0], method, anchor)
    assert LR.same_tree(got, want), "G = %d, %s, anchor = %d: got %s, want %s" % (d.shape[0], method, anchor, _describe(got), _describe(want))
    return got


def _both_cut(case, tree, count=1, stop=np.inf):
    d, q, dev = case
    want = LR.cut(d, tree, count, stop, q=q)
    got = _cut(dev, d.shape[0], tree, count, stop)
    assert LR.same(got, want), "cut G = %d, count = %d, stop = %r: got %s, want %s" % (d.shape[0], count, stop, (got[0][:8], got[3][:8], got[5:]),
                                                                                 (want[0][:8], want[3][:8], want[5:]))
    return got


# ------------------------------------------------------------------------------------------------ 1. the kernels against the rule
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("G", [1, 2, 3, 63, 64, 65, 257, 1025])
def test_kernels_equal_the_restated_rule(G, method):
    """a wave, a row workgroup (4 rows), the choose workgroup's 1024, odd sizes; a few cuts of each tree"""
    case = _case("metric", G)
    tree = _both_tree(case, method, want=_want("metric", (G,), method))
    assert tree[5] == 0 and sorted(tree[4].tolist()) == list(range(G)) and (tree[0][:G - 1] >= 0).all() and tree[0][G - 1] == -1
    for count in sorted({1, min(2, G), min(7, G), G}):
        got = _both_cut(case, tree, count)
        assert got[6:] == (count, 0)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("G", [65, 257])
def test_small_values_both_tie_rules(G, method):
    """nearly every arg-min is a tie: between rows (the lowest a) and inside a row (the lowest b)"""
    for values in ((1.0, 2.0, 3.0), (1.0, 2.0)):
        case = _fresh(LR.small_values(G, seed=G + len(values), values=values))
        tree = _both_tree(case, method)
        for count, stop in ((1, 1.0), (1, 2.0), (5, np.inf), (G // 2, 2.5)):
            _both_cut(case, tree, count, stop)
    for value in (2.5, 0.0):                             # every key ties, always: (0, 1), (0, 2), ...
        case = _fresh(np.full((G, G), F32(value)))
        tree = _both_tree(case, method)
        assert tree[0][:G - 1].tolist() == [0] * (G - 1) and tree[1][:G - 1].tolist() == list(range(1, G))
        assert tree[4].tolist() == list(range(G)) and (tree[2][:G - 1] == value).all()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["line", "star"])
def test_rescan_heavy_trees(name, method):
    case = _case(name, 257)
    tree = _both_tree(case, method, want=_want(name, (257,), method))
    for count, stop in ((1, 1.0), (3, np.inf), (1, 2.0), (100, 64.0)):
        _both_cut(case, tree, count, stop)


@pytest.mark.parametrize("method", METHODS)
def test_ineligible_conformers_bad_entries_and_anchors(method):
    G = 65
    base = _case("metric", G)[0]
    bad = [1, 21, 64]
    case = _fresh(LR.with_inf(base, bad))
    ok = [j for j in range(G) if j not in bad]
    tree = _both_tree(case, method)
    assert (tree[4][bad] == -1).all() and sorted(tree[4][ok].tolist()) == list(range(len(ok))) and tree[0][len(ok) - 1] == -1
    for count in (1, 4, len(ok), G):
        got = _both_cut(case, tree, count)
        assert (got[1][bad] == -1).all() and np.isnan(got[2][bad]).all() and got[3].sum() == len(ok) and got[6] == min(count, len(ok))
    alone = _both_tree(case, method, anchor=21)          # an unusable anchor is alone with itself
    assert alone[5] == 0 and alone[4][21] == 0 and (alone[4] >= 0).sum() == 1 and (alone[0] == -1).all()
    assert _both_cut(case, alone)[6] == 1
    _both_tree(case, method, anchor=7)                   # a non-zero anchor: the same conformers
    for anchor in (-1, G, 1 << 30):                      # out of range: status 2, an empty tree
        empty = _both_tree(case, method, anchor=anchor)
        assert empty[5] == 2 and (empty[0] == -1).all() and (empty[1] == -1).all() and np.isnan(empty[2]).all()
        assert not empty[3].any() and (empty[4] == -1).all()
        assert _both_cut(case, empty)[6:] == (0, 0)
    for value in (np.nan, -1.0, 5000.0, np.inf, -np.inf):    # an invalid entry between two eligible conformers counts as 2^40
        e = np.array(base)
        e[5, 6] = e[6, 5] = e[ok[-2], ok[-1]] = e[9, 20] = value
        case_e = _fresh(e)
        tree = _both_tree(case_e, method)
        _both_cut(case_e, tree, 3)
        _both_cut(case_e, tree, 1)                       # (near copies the entry as it is stored)
    e = np.array(base)
    e[0, 3] = np.nextafter(F32(4096), F32(np.inf))       # just above the cap in the anchor's row: 3 is out
    e[5, 6] = 4096.0                                     # the cap itself is a distance
    tree = _both_tree(_fresh(e), method)
    assert tree[4][3] == -1 and (tree[4] >= 0).sum() == G - 1


@pytest.mark.parametrize("method", METHODS)
def test_only_the_strict_upper_triangle_is_read(method):
    G = 257
    d, q, dev = _case("metric", G)
    want = _want("metric", (G,), method)
    junk = LR.upper_only(d, seed=3)
    junk[0, 0] = np.nan
    got = _tree(torch.from_numpy(junk).cuda(), G, method)
    assert LR.same_tree(got, want)
    got = _tree(torch.from_numpy(LR.upper_only(d, seed=4)).cuda(), G, method, anchor=100)     # row 100 left of the diagonal: junk
    assert LR.same_tree(got, LR.linkage(LR.upper_only(d, seed=4), method, anchor=100))


def test_average_rounds_once_above_two_to_the_53():
    """every entry one of the eight float32 values up to and including 4096: the sums pass 2^53, so (double)W rounds and the
    division rounds once more -- the rule's, bit for bit"""
    G = 257
    values = [F32(4096)]
    for _ in range(7):
        values.append(np.nextafter(values[-1], F32(0)))
    case = _fresh(LR.small_values(G, seed=53, values=tuple(float(v) for v in values)))
    tree = _both_tree(case, "average")
    members, most = {j: 1 for j in range(G)}, 0
    for a, b in zip(tree[0][:G - 1].tolist(), tree[1][:G - 1].tolist()):
        most = max(most, members[a] * members[b])
        members[a] += members.pop(b)
    assert most * int(case[1][0, 1:].min()) > 2 ** 53    # a pair weight that is no fp64: the conversion rounded
    for count in (1, 2, 9):
        _both_cut(case, tree, count)
    for method in ("single", "complete"):
        _both_tree(case, method)


# ------------------------------------------------------------------------------------------------ 2. the cut
@pytest.mark.parametrize("method", METHODS)
def test_cut_at_every_count(method):
    G = 65
    case = _case("metric", G)
    tree = _want("metric", (G,), method)
    for count in range(1, G + 1):
        assert _both_cut(case, tree, count)[6] == count
    for count in (G + 1, 1000, 1 << 30):                 # count >= M applies nothing
        got = _both_cut(case, tree, count)
        assert got[6] == G and got[0].tolist() == list(range(G)) and got[1].tolist() == list(range(G)) and got[5] == 0


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name, G", [("line", 65), ("metric", 65), ("small_values", 64)])
def test_cut_at_thresholds_taken_from_the_heights(name, G, method):
    """<= is inclusive: at the float32 that equals a height the merge is applied, one float32 below it is not"""
    case = _case(name, G) if name != "small_values" else _case(name, G, 5)
    tree = LR.linkage(case[0], method, q=case[1])
    seen = 0
    for h in sorted(set(tree[2][:G - 1].tolist()))[:12]:
        T = F32(h)
        if not LR.valid(T):
            continue
        for stop in (T, np.nextafter(T, F32(0)), np.nextafter(T, F32(np.inf))):
            if LR.valid(stop):
                _both_cut(case, tree, 1, float(stop))
                _both_cut(case, tree, 3, float(stop))
        seen += float(T) == h
    assert seen > 0 or name == "metric"                  # (integer distances: the thresholds hit the heights exactly)
    _both_cut(case, tree, 1, 0.0)
    _both_cut(case, tree, 1, 4096.0)


def test_cut_of_something_that_is_no_tree_gives_status_two():
    G = 65
    case = _case("metric", G)
    tree = _want("metric", (G,), "average")
    for t, (a, b) in ((0, (5, 5)), (3, (7, 2)), (10, (0, G)), (20, (0, 1 << 20))):
        left, right = tree[0].copy(), tree[1].copy()
        left[t], right[t] = a, b
        broken = (left, right) + tuple(tree[2:])
        got = _both_cut(case, broken, 1)
        assert got[6:] == (0, 2) and (got[0] == -1).all() and (got[1] == -1).all() and np.isnan(got[2]).all() and got[5] == 0
        assert _both_cut(case, broken, G - t)[7] == 0    # (the broken record is never applied)


@pytest.mark.parametrize("method", METHODS)
def test_two_calls_into_scratch_filled_differently_are_bit_identical(method):
    from agdiff_amd.linkage import cut_tree, linkage
    G = 300
    d, q, dev = _case("metric", G)
    a = _tree(dev, G, method, fill=0)
    b = _tree(dev, G, method, fill=-1)
    c = _tree(dev, G, method, fill=0x7ff8000000000000)
    assert LR.same_tree(a, b) and LR.same_tree(a, c) and LR.same_tree(a, LR.linkage(d, method, q=q))
    x, y = linkage(dev, G, method), linkage(dev, G, method)          # ... and through the wrappers
    for u, v, dtype, m in zip(x, y, (torch.int32, torch.int32, torch.float64, torch.int32, torch.int32, torch.int32), (G,) * 5 + (1,)):
        assert u.dtype == dtype and tuple(u.shape) == (m,) and u.is_cuda and torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    assert LR.same_tree([t.cpu().numpy() for t in x[:5]] + [int(x[5])], a)
    for count, stop in ((4, np.inf), (1, 1.5)):
        p, r = cut_tree(dev, G, x, count, stop), cut_tree(dev, G, y, count, stop)
        for u, v in zip(p, r):
            assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
        assert LR.same([t.cpu().numpy() for t in p[:5]] + [p[5].item(), int(p[6]), int(p[7])], LR.cut(d, a, count, stop, q=q))


def test_size_limit_and_no_conformers():
    from agdiff_amd import _lib
    from agdiff_amd.linkage import cut_tree, linkage
    G = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1
    big = torch.zeros((G, G), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.AgdiffLimitError):
        linkage(big, G)
    status = _full(1, SENTINEL, torch.int32)
    ints, doubles, work = _full(0, SENTINEL, torch.int32), _full(0, FSENTINEL, torch.float64), _full(0, SENTINEL, torch.int64)
    dist = torch.zeros(1, dtype=torch.float32, device="cuda")
    _lib.call("agdiff_linkage", dist, 0, 2, 0, ints, ints, doubles, ints, ints, status, work)      # no launch: status = 0
    assert status.cpu().tolist() == [0] + [SENTINEL] * TAIL and (ints == SENTINEL).all() and (doubles == FSENTINEL).all()
    n, status, cost = _full(1, SENTINEL, torch.int32), _full(1, SENTINEL, torch.int32), _full(1, FSENTINEL, torch.float64)
    floats = _full(0, FSENTINEL, torch.float32)
    _lib.call("agdiff_linkage_cut", dist, 0, ints, ints, doubles, ints, 1, float("inf"), ints, ints, floats, ints, doubles, cost, n,
              status, work)
    assert n.cpu().tolist() == [0] + [SENTINEL] * TAIL and status.cpu().tolist() == [0] + [SENTINEL] * TAIL
    assert cost.cpu().tolist() == [0.0] + [FSENTINEL] * TAIL and (ints == SENTINEL).all() and (work == SENTINEL).all()
    small = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    tree = linkage(small, 4)
    for bad in (lambda: linkage(small, 4, "ward"), lambda: linkage(small.double(), 4), lambda: linkage(small, 5),
                lambda: cut_tree(small, 4, tree, 0), lambda: cut_tree(small, 4, tree, 1, -1.0), lambda: cut_tree(small, 4, tree, 1, 5000.0),
                lambda: cut_tree(small, 4, tree, 1, float("nan")), lambda: cut_tree(small, 4, tree[:3]),
                lambda: cut_tree(small, 4, [t.cpu() for t in tree])):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ 3. end to end
def _seven():
    at, bonds, gen, _ = seven_pattern_conformers(np.random.default_rng(9))
    _, bi, bt = TR.graph(at, bonds)
    return dict(atom_type=at, bond_index=bi, bond_type=bt, pos_gen=gen), gen


def _check_result(res, matrix, method, count, stop, G, n_atoms, sel=None):
    """a linkage_conformers result against the restatement run on the matrix of the usable conformers (`sel`: their indices)"""
    sel = np.arange(G) if sel is None else np.asarray(sel)
    tree = LR.linkage(matrix, method)
    med, labels, near, size, within, cost, K, status = LR.cut(matrix, tree, count, stop)
    M = int((tree[4] >= 0).sum())
    for key, dtype, shape in (("medoids", torch.int32, (K,)), ("labels", torch.int32, (G,)), ("near", torch.float32, (G,)),
                              ("count", torch.int32, (K,)), ("population", torch.float32, (K,)), ("within", torch.float64, (K,)),
                              ("pos", torch.float32, (K, n_atoms, 3)), ("merges", torch.int32, (M - 1, 2)),
                              ("heights", torch.float64, (M - 1,)), ("merge_sizes", torch.int32, (M - 1,)), ("order", torch.int32, (G,))):
        assert res[key].dtype == dtype and tuple(res[key].shape) == shape and res[key].is_cuda, key
    assert res["cost"] == cost and res["n_clusters"] == K and res["linkage"] == method and "iters" not in res and "converged" not in res
    full_labels, full_near, full_order = np.full(G, -1, np.int32), np.full(G, np.nan, F32), np.full(G, -1, np.int32)
    full_labels[sel], full_near[sel], full_order[sel] = labels, near, tree[4]
    assert LR.same((res["medoids"].cpu().numpy(), res["labels"].cpu().numpy(), res["near"].cpu().numpy(), res["count"].cpu().numpy(),
                    res["within"].cpu().numpy(), res["order"].cpu().numpy(), res["heights"].cpu().numpy(), res["merge_sizes"].cpu().numpy()),
                   (sel[med[:K]], full_labels, full_near, size[:K], within[:K], full_order, tree[2][:M - 1], tree[3][:M - 1]))
    assert np.array_equal(res["merges"].cpu().numpy(), np.stack([sel[tree[0][:M - 1]], sel[tree[1][:M - 1]]], axis=1))
    assert LR.same((res["population"].cpu().numpy(),), (size[:K].astype(F32) / F32(sel.size),))
    return tree


@pytest.mark.parametrize("metric, rings", [("rmsd", False), ("tfd", False), ("tfd", True)])
def test_seven_pattern_equals_the_restatement_on_the_devices_matrix(metric, rings):
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.linkage import linkage_conformers, sweep_linkage, to_scipy
    from agdiff_amd.silhouette import silhouette
    from agdiff_amd.torsions import tfd_self
    item, gen = _seven()
    G, n = gen.shape[0], gen.shape[1]
    dev = self_rmsd_matrix(item) if metric == "rmsd" else tfd_self(item, rings=rings)[0]
    matrix = dev.cpu().numpy()
    kw = dict(metric=metric, tfd_rings=rings, align=False)
    for method in METHODS:
        for count, stop in ((1, np.inf), (3, np.inf), (7, np.inf), (12, np.inf), (1, float(np.median(matrix))), (2, 0.0)):
            res = linkage_conformers(item, method=method, count=count, height=stop, **kw)
            tree = _check_result(res, matrix, method, count, stop, G, n)
            assert torch.equal(res["pos"].cpu(), torch.from_numpy(gen[res["medoids"].cpu().numpy()]))
        Z, leaves = to_scipy(*tree[:5])
        assert Z.shape == (G - 1, 4) and leaves.tolist() == list(range(G)) and (Z[:, 0] < Z[:, 1]).all() and Z[-1, 3] == G
        assert np.array_equal(Z[:, 2], tree[2][:G - 1]) and sorted(Z[:, :2].reshape(-1).tolist()) == list(range(2 * G - 2))
        sweep = sweep_linkage(item, 2, 6, method=method, **kw)
        assert sweep["k"].tolist() == [2, 3, 4, 5, 6] and set(sweep) == {"k", "mean", "cost", "best_k", "medoids", "silhouette"}
        means = []
        for K in range(2, 7):
            labels = LR.cut(matrix, tree, K)[1]
            means.append(silhouette(dev, G, torch.from_numpy(labels).cuda(), K)[6].item())
        assert sweep["mean"].tolist() == means
        best = max(range(5), key=lambda j: (means[j], -j))
        assert sweep["best_k"] == 2 + best and sweep["medoids"]["n_clusters"] == 2 + best
        _check_result(sweep["medoids"], matrix, method, 2 + best, np.inf, G, n)
        assert sweep["silhouette"]["mean"] == means[best]


@pytest.mark.parametrize("n,K,G", [(20, 4, 37)])
def test_families_are_recovered_by_count_height_and_sweep(n, K, G):
    """K tight families (0.03 Angstrom of noise) far apart: the cut at K, the cut at 0.5 Angstrom and the sweep's best K are the
    families, whatever the method; masked conformers keep the item's own indices"""
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.linkage import linkage_conformers, sweep_linkage
    item, label, gen, heavy = _families(n, K, G)
    matrix = self_rmsd_matrix(item).cpu().numpy()
    for method in METHODS:
        by_count = linkage_conformers(item, method=method, count=K)
        _check_result(by_count, matrix, method, K, np.inf, G, n)
        by_height = linkage_conformers(item, method=method, height=0.5, align=False)
        sweep = sweep_linkage(item, 2, 8, method=method, align=False)
        assert sweep["best_k"] == K
        for res in (by_count, by_height, sweep["medoids"]):
            labels, med = res["labels"].cpu().numpy(), res["medoids"].cpu().numpy()
            assert res["n_clusters"] == K and np.array_equal(label[med][labels], label) and float(res["near"].max()) < 0.5
            assert res["count"].cpu().tolist() == [int((label == label[m]).sum()) for m in med]
            assert float(res["heights"][G - K - 1]) < 0.5 < float(res["heights"][G - K])       # the gap in the heights
            order = res["order"].cpu().numpy()           # every family is one run of the leaf order
            assert all(np.ptp(order[label == c]) == (label == c).sum() - 1 for c in range(K))
    med = by_count["medoids"].cpu().numpy()              # align: rank 0 bit for bit, the others on it within the bar
    assert torch.equal(by_count["pos"][0].cpu(), torch.from_numpy(gen[med[0]]))
    aligned = np.stack([_kabsch_align(gen[m], gen[med[0]], heavy) for m in med])
    dev = np.abs(by_count["pos"].cpu().numpy() - aligned).max()
    print("aligned medoids n=%d: max |aligned - float64 Kabsch| = %.3e Angstrom" % (n, dev))
    assert dev <= ALIGN_ATOL
    valid = np.ones(G, dtype=bool)
    valid[label == 2] = False
    valid[[0, 5]] = False
    sel = np.nonzero(valid)[0]
    sub = self_rmsd_matrix(dict(item, pos_gen=gen[sel])).cpu().numpy()
    res = linkage_conformers(item, count=3, valid=valid, align=False)
    _check_result(res, sub, "average", 3, np.inf, G, n, sel=sel)
    assert np.array_equal(res["labels"].cpu().numpy() == -1, ~valid) and np.array_equal(res["order"].cpu().numpy() == -1, ~valid)
    none = linkage_conformers(item, count=3, valid=np.zeros(G, dtype=bool))
    assert none["n_clusters"] == 0 and tuple(none["merges"].shape) == (0, 2) and (none["order"] == -1).all() and none["cost"] == 0.0
    assert tuple(none["medoids"].shape) == (0,) and tuple(none["pos"].shape) == (0, n, 3) and (none["labels"] == -1).all()


def test_command_line_round_trip_and_silhouette_of_its_labels(tmp_path, capsys):
    from agdiff_amd import driver, linkage, silhouette, synth
    from agdiff_amd.ensemble import self_rmsd_matrix
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
    out = linkage.main(base + ["--count", "2", "--align", "--out", str(tmp_path / "tree.npz")])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and "6 clusters of 19 conformers" in line[0] and "RMSD" in line[0] and "average linkage, 2 per molecule" in line[0]
    z = np.load(str(tmp_path / "tree.npz"))
    keys = ("medoid", "cluster", "dist", "count", "population", "within", "cost", "pos", "name", "merge", "height", "merge_size",
            "order", "linkage", "leaves")
    assert set(z.files) == {"%s_%d" % (k, i) for k in keys for i in range(3)} == set(out)
    for i, g in enumerate(gens):
        G, n = g.shape[0], g.shape[1]
        for k, dtype, shape in (("medoid", np.int32, (2,)), ("cluster", np.int32, (G,)), ("dist", np.float32, (G,)),
                                ("count", np.int32, (2,)), ("population", np.float32, (2,)), ("within", np.float64, (2,)),
                                ("cost", np.float64, ()), ("pos", np.float32, (2, n, 3)), ("merge", np.int32, (G - 1, 2)),
                                ("height", np.float64, (G - 1,)), ("merge_size", np.int32, (G - 1,)), ("order", np.int32, (G,)),
                                ("leaves", np.int64, (G,))):
            assert z["%s_%d" % (k, i)].dtype == dtype and z["%s_%d" % (k, i)].shape == shape, (k, i)
            assert np.array_equal(z["%s_%d" % (k, i)], out["%s_%d" % (k, i)], equal_nan=True)
        assert str(z["name_%d" % i]) == mols[i]["name"] and str(z["linkage_%d" % i]) == "average"
        med = z["medoid_%d" % i]
        assert np.array_equal(z["cluster_%d" % i][med], np.arange(2)) and z["count_%d" % i].sum() == G
        assert np.array_equal(z["pos_%d" % i][0], g[med[0]]) and z["within_%d" % i].sum() == z["cost_%d" % i]
        assert sorted(z["order_%d" % i].tolist()) == list(range(G)) and z["merge_size_%d" % i][-1] == G
        item = dict(atom_type=mols[i]["atom_type"], edge_index=mols[i]["edge_index"], edge_type=mols[i]["edge_type"], pos_gen=g)
        matrix = self_rmsd_matrix(item).cpu().numpy()
        tree = LR.linkage(matrix, "average")
        assert np.array_equal(z["height_%d" % i], tree[2][:G - 1]) and np.array_equal(z["cluster_%d" % i], LR.cut(matrix, tree, 2)[1])
    for i in (1, 2):                                     # two tight families, the even and the odd conformers
        assert np.array_equal(z["cluster_%d" % i], np.arange(gens[i].shape[0]) % 2) and z["dist_%d" % i].max() < 0.2
    by_height = linkage.main(base + ["--height", "0.5", "--method", "complete", "--out", str(tmp_path / "h.npz")])
    assert "complete linkage, cut at 0.5" in capsys.readouterr().out
    swept = linkage.main(base + ["--sweep", "2", "4", "--method", "single", "--out", str(tmp_path / "s.npz")])
    assert "single linkage, the best of K = 2 .. 4 by silhouette" in capsys.readouterr().out
    for i in (1, 2):
        assert np.array_equal(by_height["cluster_%d" % i], z["cluster_%d" % i]) and str(by_height["linkage_%d" % i]) == "complete"
        assert np.array_equal(swept["cluster_%d" % i], z["cluster_%d" % i]) and swept["best_k_%d" % i] == 2
        assert swept["sweep_k_%d" % i].tolist() == [2, 3, 4] and swept["sweep_sil_%d" % i].shape == (3,)
    tfd = linkage.main(base + ["--count", "2", "--tfd", "--drop-invalid", "--out", str(tmp_path / "tfd.npz")])
    assert "TFD" in capsys.readouterr().out
    for i in range(3):
        assert np.array_equal(tfd["cluster_%d" % i] == -1, tfd["valid_%d" % i] == 0)
        assert np.array_equal(tfd["order_%d" % i] == -1, tfd["valid_%d" % i] == 0)
    # python -m agdiff_amd.silhouette scores the file as it is
    sil = silhouette.main(base + ["--labels", str(tmp_path / "tree.npz"), "--out", str(tmp_path / "sil.npz")])
    assert "labels cluster of" in capsys.readouterr().out
    for i in range(3):
        assert np.array_equal(sil["count_%d" % i], z["count_%d" % i]) and sil["sil_%d" % i].shape == (gens[i].shape[0],)
    for i in (1, 2):
        assert sil["sil_mean_%d" % i] > 0.8
