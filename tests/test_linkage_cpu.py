"""No GPU: the C ABI of agdiff_linkage and agdiff_linkage_cut as the header declares it, their host-side argument checks (every one
returns before any launch), the signatures and argument checks of agdiff_amd.linkage, to_scipy and the command line's parser."""
import ctypes
import inspect

import numpy as np
import pytest

from agdiff_amd import _lib

VP, I32, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
INF = float("inf")


def _buf():
    """a non-null, 8-byte aligned host address: the checks under test return before anything is read or launched"""
    b = (ctypes.c_uint64 * 8)()
    return b, ctypes.c_void_p(ctypes.addressof(b))


def _tree(lib, dist, outs, G=8, method=2, anchor=0):
    """outs: left, right, height, size, order, status, work"""
    return lib.agdiff_linkage(dist, G, method, anchor, *outs, ctypes.c_void_p(0))


def _cut(lib, dist, ptrs, G=8, count=1, stop=INF):
    """ptrs: left, right, height, order | medoids, labels, near, size, within, cost, n_clusters, status, work"""
    return lib.agdiff_linkage_cut(dist, G, *ptrs[:4], count, stop, *ptrs[4:], ctypes.c_void_p(0))


def test_exports_equal_the_headers_declarations():
    assert _lib.EXPORTS["agdiff_linkage"] == [VP, I32, I32, I32] + [VP] * 8
    assert _lib.EXPORTS["agdiff_linkage_cut"] == [VP, I32] + [VP] * 4 + [I32, F] + [VP] * 10
    lib = _lib.load()
    for name in ("agdiff_linkage", "agdiff_linkage_cut"):
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.EXPORTS[name]
    assert lib.agdiff_abi_version() == _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48            # the exports are additions only
    D = _lib.DEFINES
    assert (D["AGDIFF_LINKAGE_SINGLE"], D["AGDIFF_LINKAGE_COMPLETE"], D["AGDIFF_LINKAGE_AVERAGE"]) == (0, 1, 2)
    # control words + nn_key (64-bit) + nn_idx, size, live, next, tail (32-bit) per slot; then the square
    assert D["AGDIFF_LINKAGE_WORK_FIXED_BYTES"] >= 64 + D["AGDIFF_PRUNE_MAX_CONFS"] * (8 + 5 * 4) and D["AGDIFF_LINKAGE_WORK_FIXED_BYTES"] % 8 == 0
    assert D["AGDIFF_LINKAGE_CUT_WORK_BYTES"] >= 32 + D["AGDIFF_PRUNE_MAX_CONFS"] * 8 and D["AGDIFF_LINKAGE_CUT_WORK_BYTES"] % 8 == 0
    header = open(_lib.HEADER).read()
    assert ("int agdiff_linkage(const float* dist, int32_t G, int32_t method, int32_t anchor,\n"
            "                   int32_t* left, int32_t* right, double* height, int32_t* size, int32_t* order, int32_t* status,\n"
            "                   uint64_t* work, void* stream);") in header
    assert ("int agdiff_linkage_cut(const float* dist, int32_t G, const int32_t* left, const int32_t* right, const double* height,\n"
            "                       const int32_t* order, int32_t count, float stop_height,\n"
            "                       int32_t* medoids, int32_t* labels, float* near, int32_t* size, double* within,\n"
            "                       double* cost, int32_t* n_clusters, int32_t* status, uint64_t* work, void* stream);") in header
    for words in ("ONLY THE STRICT UPPER TRIANGLE IS READ", "j == anchor or", "TIES TO THE LOWEST a, THEN TO THE", "its SLOT",
                  "ONE\n *     correctly rounded division", "next[tail[a]] = b; tail[a] = tail[b]", "HEIGHTS ARE NOT PROMISED MONOTONE",
                  "whenever every sum stays below 2^53", "the first merge that fails either test ends it", "8 G G + AGDIFF_LINKAGE_WORK_FIXED_BYTES",
                  "No cooperative launch, no workgroup waits on another, no atomics on global memory", "Ward, centroid and median linkage",
                  "optimal leaf ordering", "on tie-free input only"):
        assert words in header, words


def test_linkage_checks_its_arguments_on_the_host():
    lib = _lib.load()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    ok = [p] * 7
    for k in range(7):
        a = list(ok)
        a[k] = null
        assert _tree(lib, p, a) == -1, k
        assert _tree(lib, p, a, G=0) == -1, k                              # (also with nothing to cluster)
    assert _tree(lib, null, ok) == -1 and _tree(lib, null, ok, G=0) == -1
    assert _tree(lib, p, ok, G=-1) == -1
    for method in (-1, 3, 7, 1 << 20):
        assert _tree(lib, p, ok, method=method) == -1 and _tree(lib, p, ok, G=0, method=method) == -1
    for off in (1, 2, 4):                                                  # a misaligned work
        a = list(ok)
        a[6] = ctypes.c_void_p(p.value + off)
        assert _tree(lib, p, a) == -1 and _tree(lib, p, a, G=0) == -1
    limit = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"]
    assert limit == 4096
    for method in (0, 1, 2):
        assert _tree(lib, p, ok, G=limit + 1, method=method) == -2
    assert _tree(lib, p, ok, G=limit + 1, anchor=-7) == -2                 # (the anchor is looked at on the device)
    assert _tree(lib, p, ok, G=limit + 1, method=3) == -1                  # (the argument errors come first)
    a = list(ok)
    a[6] = ctypes.c_void_p(p.value + 4)
    assert _tree(lib, p, a, G=limit + 1) == -1
    a = list(ok)
    a[2] = null
    assert _tree(lib, p, a, G=limit + 1) == -1
    assert _tree(lib, p, ok, G=0, anchor=-5) == 0                          # nothing to cluster: no launch, the anchor is not looked at
    assert _tree(lib, ctypes.c_void_p(p.value + 4), ok, G=limit + 1) == -2     # dist needs 4-byte alignment only
    with pytest.raises(_lib.AgdiffLimitError):
        _lib.check(_tree(lib, p, ok, G=limit + 1), "agdiff_linkage")
    with pytest.raises(_lib.AgdiffHipError):
        _lib.check(_tree(lib, p, ok, method=5), "agdiff_linkage")
    del keep


def test_cut_checks_its_arguments_on_the_host():
    lib = _lib.load()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    ok = [p] * 13
    for k in range(13):
        a = list(ok)
        a[k] = null
        assert _cut(lib, p, a) == -1, k
        assert _cut(lib, p, a, G=0) == -1, k
    assert _cut(lib, null, ok) == -1 and _cut(lib, p, ok, G=-1) == -1
    for count in (0, -1, -(1 << 31)):
        assert _cut(lib, p, ok, count=count) == -1 and _cut(lib, p, ok, G=0, count=count) == -1
    top = float(np.nextafter(np.float32(4096), np.float32(np.inf)))
    for stop in (float("nan"), -1.0, -1e-30, -INF, top, 5000.0, 3e38):    # NaN, negative, finite above the cap
        assert _cut(lib, p, ok, stop=stop) == -1, stop
        assert _cut(lib, p, ok, G=0, stop=stop) == -1, stop
    for off in (1, 2, 4):
        a = list(ok)
        a[12] = ctypes.c_void_p(p.value + off)
        assert _cut(lib, p, a) == -1 and _cut(lib, p, a, G=0) == -1
    limit = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"]
    for stop in (INF, 0.0, -0.0, 0.5, 4096.0):                             # +inf or valid(T)
        assert _cut(lib, p, ok, G=limit + 1, stop=stop) == -2, stop
    assert _cut(lib, p, ok, G=limit + 1, count=1 << 30) == -2              # any count >= 1
    assert _cut(lib, p, ok, G=limit + 1, count=0) == -1                    # (the argument errors come first)
    assert _cut(lib, p, ok, G=limit + 1, stop=-2.0) == -1
    a = list(ok)
    a[12] = ctypes.c_void_p(p.value + 4)
    assert _cut(lib, p, a, G=limit + 1) == -1
    assert _cut(lib, p, ok, G=0) == 0 and _cut(lib, p, ok, G=0, count=9, stop=1.5) == 0
    with pytest.raises(_lib.AgdiffLimitError):
        _lib.check(_cut(lib, p, ok, G=limit + 1), "agdiff_linkage_cut")
    del keep


def test_signatures_and_defaults():
    from agdiff_amd import ensemble, linkage, medoids, silhouette
    sig = inspect.signature(linkage.linkage)
    assert list(sig.parameters) == ["dist", "G", "method", "anchor"]
    assert sig.parameters["method"].default == "average" and sig.parameters["anchor"].default == 0
    sig = inspect.signature(linkage.cut_tree)
    assert list(sig.parameters) == ["dist", "G", "tree", "count", "height"]
    assert sig.parameters["count"].default == 1 and sig.parameters["height"].default == INF
    assert list(inspect.signature(linkage.to_scipy).parameters) == ["left", "right", "height", "size", "order"]
    sig = inspect.signature(linkage.linkage_conformers)
    assert list(sig.parameters) == ["item", "method", "count", "height", "metric", "align", "device", "valid", "fix_handedness",
                                    "fix_double_bonds", "tfd_rings"]
    want = dict(method="average", count=1, height=INF, metric="rmsd", align=True, device="cuda", valid=None, fix_handedness=False,
                fix_double_bonds=False, tfd_rings=False)
    assert {n: p.default for n, p in sig.parameters.items() if n != "item"} == want
    sig = inspect.signature(linkage.sweep_linkage)
    assert list(sig.parameters) == ["item", "k_min", "k_max", "method", "metric", "align", "device", "valid", "fix_handedness",
                                    "fix_double_bonds", "tfd_rings"]
    assert sig.parameters["method"].default == "average" and sig.parameters["k_min"].default is inspect.Parameter.empty
    assert linkage.METHODS == ("single", "complete", "average")
    assert linkage.WORK_FIXED_BYTES == _lib.DEFINES["AGDIFF_LINKAGE_WORK_FIXED_BYTES"]
    assert linkage.CUT_WORK_BYTES == _lib.DEFINES["AGDIFF_LINKAGE_CUT_WORK_BYTES"]
    # the shared prelude, medoids' result and the silhouette call, not copies
    assert linkage._usable_matrix is ensemble._usable_matrix and linkage._result is medoids._result
    assert linkage.silhouette is silhouette.silhouette and linkage._check_sweep is silhouette._check_sweep


def test_linkage_conformers_checks_its_arguments_before_any_device_work():
    from agdiff_amd import linkage
    item = {"atom_type": [6, 6], "pos_gen": [[0.0, 0, 0], [1, 0, 0], [0.0, 0, 0], [1.1, 0, 0]]}
    for method in ("ward", "centroid", "median", "upgma", 2, None):
        with pytest.raises(ValueError):
            linkage.linkage_conformers(item, method=method)
        with pytest.raises(ValueError):
            linkage.sweep_linkage(item, 2, 3, method=method)
    with pytest.raises(ValueError):
        linkage.linkage_conformers(item, metric="usr")
    with pytest.raises(ValueError):
        linkage.linkage_conformers(item, tfd_rings=True)                  # (the rings are terms of the TFD)
    for count in (0, -1, 1.5):
        with pytest.raises(ValueError):
            linkage.linkage_conformers(item, count=count)
    for height in (-1.0, float("nan"), 5000.0, -INF, "high"):
        with pytest.raises(ValueError):
            linkage.linkage_conformers(item, height=height)
    for lo, hi in ((1, 3), (3, 2), (2, 2.5), (2, 66)):
        with pytest.raises(ValueError):
            linkage.sweep_linkage(item, lo, hi)
    for valid in (np.ones(3, dtype=bool), np.ones(2, dtype=np.int32)):
        with pytest.raises(ValueError):
            linkage.linkage_conformers(item, valid=valid)
    with pytest.raises(ValueError):
        linkage.linkage_conformers({"atom_type": [6, 6], "pos_gen": np.zeros((0, 3), np.float32)})
    G = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1
    with pytest.raises(_lib.AgdiffLimitError):
        linkage.linkage_conformers({"atom_type": np.array([6, 6]), "pos_gen": np.zeros((G, 2, 3), np.float32)})


def test_wrappers_check_their_tensors():
    import torch
    from agdiff_amd import linkage
    d = torch.zeros((4, 4), dtype=torch.float32)                          # (on the host: refused before any launch)
    with pytest.raises(ValueError):
        linkage.linkage(d, 4)
    with pytest.raises(ValueError):
        linkage.linkage(np.zeros((4, 4), np.float32), 4)
    with pytest.raises(ValueError):
        linkage.linkage(d, 4, "ward")
    with pytest.raises(ValueError):
        linkage.linkage(d, 4, anchor=0.5)
    tree = (torch.zeros(4, dtype=torch.int32),) * 2 + (torch.zeros(4, dtype=torch.float64),) + (torch.zeros(4, dtype=torch.int32),) * 2
    for bad in (lambda: linkage.cut_tree(d, 4, tree), lambda: linkage.cut_tree(d, 4, tree, 0), lambda: linkage.cut_tree(d, 4, tree, 1, -0.5),
                lambda: linkage.cut_tree(d, 4, tree[:2])):
        with pytest.raises(ValueError):
            bad()


def test_to_scipy_by_hand():
    from agdiff_amd.linkage import to_scipy
    # conformers 1 and 4 left out; merges (2, 5) at 1, (0, 3) at 2, (0, 2) at 6: leaves 0, 2, 3, 5 are the ids 0, 1, 2, 3
    left, right = np.array([2, 0, 0, -1, -1, -1], np.int32), np.array([5, 3, 2, -1, -1, -1], np.int32)
    height = np.array([1.0, 2.0, 6.0, np.nan, np.nan, np.nan])
    size, order = np.array([2, 2, 4, 0, 0, 0], np.int32), np.array([0, -1, 2, 1, -1, 3], np.int32)
    Z, leaves = to_scipy(left, right, height, size, order)
    assert leaves.tolist() == [0, 2, 3, 5] and Z.dtype == np.float64
    assert Z.tolist() == [[1, 3, 1.0, 2], [0, 2, 2.0, 2], [4, 5, 6.0, 4]]            # the lower id first: {2, 5} is 4, {0, 3} is 5
    Z, leaves = to_scipy(left[:0], right[:0], height[:0], size[:0], order[:0])
    assert Z.shape == (0, 4) and leaves.shape == (0,)
    Z, leaves = to_scipy(*(np.full(3, v, t) for v, t in ((-1, np.int32), (-1, np.int32), (np.nan, np.float64), (0, np.int32))),
                         np.array([-1, 0, -1], np.int32))
    assert Z.shape == (0, 4) and leaves.tolist() == [1]
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    import linkage_ref as LR
    d = LR.random_metric(17, seed=17)
    for method in ("single", "complete", "average"):
        Z, leaves = to_scipy(*LR.linkage(d, method)[:5])
        assert hierarchy.is_valid_linkage(Z) and leaves.tolist() == list(range(17))
        got = hierarchy.fcluster(Z, 3, criterion="maxclust")
        want = LR.cut(d, LR.linkage(d, method), 3)[1]
        assert len(set(zip(got.tolist(), want.tolist()))) == 3               # the same partition, under its own numbering


def test_parser_flags_and_defaults(capsys):
    from agdiff_amd import linkage
    base = ["--samples", "s.npz", "--testset", "t.npz", "--out", "o.npz"]
    ap = linkage._parser()
    a = ap.parse_args(base + ["--count", "5"])
    assert a.count == 5 and a.height is None and a.sweep is None and a.method == "average" and a.tfd is False and a.tfd_rings is False
    assert a.align is False and a.device == "cuda" and not (a.fix_handedness or a.fix_double_bonds or a.drop_invalid or a.drop_bent)
    assert (a.samples, a.testset, a.out) == ("s.npz", "t.npz", "o.npz")
    a = ap.parse_args(base + ["--height", "0.75", "--method", "single", "--tfd", "--tfd-rings", "--align", "--drop-invalid", "--drop-bent",
                              "--fix-handedness", "--fix-double-bonds"])
    assert a.height == 0.75 and a.count is None and a.method == "single" and a.tfd and a.tfd_rings and a.align and a.drop_invalid
    assert a.drop_bent and a.fix_handedness and a.fix_double_bonds
    a = ap.parse_args(base + ["--sweep", "2", "12", "--method", "complete"])
    assert a.sweep == [2, 12] and a.method == "complete"
    assert ap.parse_args(base + ["--height", "inf"]).height == INF
    for bad in (base, base + ["--count", "3", "--height", "1"], base + ["--count", "3", "--sweep", "2", "4"], base + ["--count", "0"],
                base + ["--count", "1.5"], base + ["--height", "-1"], base + ["--height", "5000"], base + ["--height", "nan"],
                base + ["--sweep", "1", "4"], base + ["--sweep", "5", "4"], base + ["--sweep", "2", "70"], base + ["--sweep", "2"],
                base + ["--count", "3", "--method", "ward"], base + ["--count", "3", "--tfd-rings"], base[2:] + ["--count", "3"],
                base + ["--count", "3", "--init", "first"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    capsys.readouterr()


def test_main_hands_its_flags_on(monkeypatch, tmp_path):
    from agdiff_amd import linkage
    seen = []

    class Stop(Exception):
        pass

    def spy_tree(item, **kw):
        seen.append(("tree", kw["method"], kw["count"], kw["height"], kw["metric"], kw["align"], kw["tfd_rings"]))
        raise Stop()

    def spy_sweep(item, lo, hi, **kw):
        seen.append(("sweep", lo, hi, kw["method"], kw["metric"]))
        raise Stop()
    mol = {"index": 0, "name": "m0"}
    monkeypatch.setattr(linkage, "sampled_items", lambda testset, samples: iter([(mol, {"atom_type": [6], "pos_gen": [[0.0, 0, 0]]})]))
    monkeypatch.setattr(linkage, "linkage_conformers", spy_tree)
    monkeypatch.setattr(linkage, "sweep_linkage", spy_sweep)
    base = ["--samples", "s.npz", "--testset", "t.npz", "--out", str(tmp_path / "o.npz")]
    for extra, want in ((["--count", "10"], ("tree", "average", 10, INF, "rmsd", False, False)),
                        (["--height", "0.5", "--align", "--method", "complete"], ("tree", "complete", 1, 0.5, "rmsd", True, False)),
                        (["--count", "3", "--tfd", "--tfd-rings", "--method", "single"], ("tree", "single", 3, INF, "tfd", False, True)),
                        (["--sweep", "2", "8", "--tfd"], ("sweep", 2, 8, "average", "tfd"))):
        with pytest.raises(Stop):
            linkage.main(base + extra)
        assert seen[-1] == want
    with pytest.raises(SystemExit):
        linkage.main(base)
