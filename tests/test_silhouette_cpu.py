"""No GPU: the C ABI of agdiff_silhouette as the header declares it, its host-side argument checks (every one returns before any
launch), the signatures and argument checks of agdiff_amd.silhouette, the label-to-rank mapping and the command line's parser."""
import ctypes
import inspect

import numpy as np
import pytest

from agdiff_amd import _lib

VP, I32 = ctypes.c_void_p, ctypes.c_int32
NPTR = 11                                                    # dist, labels, the eight outputs, work


def _buf():
    """a non-null, 8-byte aligned host address: the checks under test return before anything is read or launched"""
    b = (ctypes.c_uint64 * 8)()
    return b, ctypes.c_void_p(ctypes.addressof(b))


def _call(lib, a, G=8, K=3):
    return lib.agdiff_silhouette(a[0], G, K, a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], ctypes.c_void_p(0))


def test_export_equals_the_headers_declaration():
    assert _lib.EXPORTS["agdiff_silhouette"] == [VP, I32, I32, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP]
    lib = _lib.load()
    assert hasattr(lib, "agdiff_silhouette") and lib.agdiff_silhouette.argtypes == _lib.EXPORTS["agdiff_silhouette"]
    assert lib.agdiff_abi_version() == _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    assert _lib.DEFINES["AGDIFF_SILHOUETTE_WORK_BYTES"] == 65536 >= 32 + 8 * _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"]
    header = open(_lib.HEADER).read()
    assert ("int agdiff_silhouette(const float* dist, int32_t G, int32_t K, const int32_t* labels,\n"
            "                      double* a, double* b, double* s, int32_t* other,\n"
            "                      int32_t* size, double* cluster_mean, double* mean, int32_t* status,\n"
            "                      uint64_t* work, void* stream);") in header
    for words in ("Rousseeuw 1987", "labels[j] == -1 means conformer j is LEFT OUT", "never read as a column", "EMPTY RANK IS NEVER",
                  "the diagonal is never read", "(double)S_own / (double)(size_own - 1)", "ties to the LOWEST rank",
                  "s(i) = (mb - ma) / max(ma, mb)", "T(i) = (int64)rint(s(i) * 2^40)", "status = 2", "every entry written in every case",
                  "not the simplified (medoid-based) one", "by definition only, not bit for bit"):
        assert words in header, words


def test_silhouette_checks_its_arguments_on_the_host():
    lib = _lib.load()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    for k in range(NPTR):
        a = [p] * NPTR
        a[k] = null
        assert _call(lib, a) == -1, k
        assert _call(lib, a, G=0) == -1, k                                 # (also with nothing to score)
    ok = [p] * NPTR
    assert _call(lib, ok, G=-1) == -1
    limit = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"]
    assert limit == 4096
    for K in (0, -1, limit + 1, 1 << 30):
        assert _call(lib, ok, K=K) == -1
        assert _call(lib, ok, G=0, K=K) == -1                              # (K sizes two outputs: it is looked at with G == 0 too)
    for off in (1, 2, 4):                                                  # a misaligned work
        a = [p] * NPTR
        a[10] = ctypes.c_void_p(p.value + off)
        assert _call(lib, a) == -1
        assert _call(lib, a, G=0) == -1
    assert _call(lib, ok, G=limit + 1, K=1) == -2
    assert _call(lib, ok, G=limit + 1, K=limit) == -2                      # (K may exceed the ranks used, and is bounded by the same limit)
    for kw in (dict(K=0), dict(K=limit + 1)):
        assert _call(lib, ok, **dict(dict(G=limit + 1), **kw)) == -1       # (the argument errors come first)
    a = [p] * NPTR
    a[10] = ctypes.c_void_p(p.value + 4)
    assert _call(lib, a, G=limit + 1, K=1) == -1
    a = [p] * NPTR
    a[5] = null
    assert _call(lib, a, G=limit + 1, K=1) == -1
    assert _call(lib, ok, G=0) == 0                                        # nothing to score: no launch
    assert _call(lib, ok, G=0, K=1) == 0
    with pytest.raises(_lib.AgdiffLimitError):
        _lib.check(_call(lib, ok, G=limit + 1, K=1), "agdiff_silhouette")
    with pytest.raises(_lib.AgdiffHipError):
        _lib.check(_call(lib, ok, K=0), "agdiff_silhouette")
    del keep


def test_unaligned_dist_is_not_an_argument_error():
    """dist needs 4-byte alignment only: an address one float into an allocation passes the checks (here: up to the limit check)"""
    lib = _lib.load()
    keep, p = _buf()
    a = [p] * NPTR
    a[0] = ctypes.c_void_p(p.value + 4)
    assert _call(lib, a, G=_lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1, K=1) == -2
    del keep


def test_signatures_and_defaults():
    from agdiff_amd import medoids, silhouette
    sig = inspect.signature(silhouette.silhouette)
    assert list(sig.parameters) == ["dist", "G", "labels", "K"]
    sig = inspect.signature(silhouette.silhouette_conformers)
    assert list(sig.parameters) == ["item", "labels", "metric", "device", "valid", "fix_handedness", "fix_double_bonds", "tfd_rings"]
    assert {n: p.default for n, p in sig.parameters.items() if n not in ("item", "labels")} == dict(
        metric="rmsd", device="cuda", valid=None, fix_handedness=False, fix_double_bonds=False, tfd_rings=False)
    sig = inspect.signature(silhouette.sweep_medoids)
    assert list(sig.parameters) == ["item", "k_min", "k_max", "metric", "init", "max_iter", "align", "device", "valid", "fix_handedness",
                                    "fix_double_bonds", "tfd_rings"]
    assert {n: p.default for n, p in sig.parameters.items() if n not in ("item", "k_min", "k_max")} == dict(
        metric="rmsd", init="maxmin", max_iter=32, align=True, device="cuda", valid=None, fix_handedness=False, fix_double_bonds=False,
        tfd_rings=False)
    assert silhouette.WORK_BYTES == 65536 and silhouette.MAX_SWEEP == 64 and silhouette.MAX_CONFS == 4096
    from agdiff_amd.ensemble import _usable_matrix                       # the prelude the other walks share
    assert silhouette._usable_matrix is _usable_matrix is medoids._usable_matrix
    assert silhouette._result is medoids._result                         # one body behind medoid_conformers and the sweep
    assert "_result(" in inspect.getsource(medoids._from_matrix) and "_from_matrix(" in inspect.getsource(medoids.medoid_conformers)


def test_silhouette_wrapper_checks_its_tensors():
    import torch
    from agdiff_amd import silhouette
    d = torch.zeros((4, 4), dtype=torch.float32)                          # (on the host: refused before any launch)
    labels = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError):
        silhouette.silhouette(d, 4, labels, 1)
    with pytest.raises(ValueError):
        silhouette.silhouette(np.zeros((4, 4), np.float32), 4, labels, 1)


ITEM = {"atom_type": [6, 6], "pos_gen": [[0.0, 0, 0], [1, 0, 0], [0.0, 0, 0], [1.1, 0, 0], [0.0, 0, 0], [1.2, 0, 0]]}     # three conformers


def test_silhouette_conformers_checks_its_arguments_before_any_device_work():
    from agdiff_amd import silhouette
    with pytest.raises(ValueError):
        silhouette.silhouette_conformers(ITEM, [0, 0, 1], metric="usr")
    with pytest.raises(ValueError):
        silhouette.silhouette_conformers(ITEM, [0, 0, 1], tfd_rings=True)     # (the rings are terms of the TFD)
    for labels in ([0, 0, -2], [0, 1], [0, 0, 1, 1], [[0, 0, 1]], [0.0, 0.0, 1.0], np.array([0, 0, 1 << 40]), [True, False, True], 3,
                   np.array([0, 0, -5], dtype=np.int64)):
        with pytest.raises(ValueError):
            silhouette.silhouette_conformers(ITEM, labels)
    for valid in (np.ones(4, dtype=bool), np.ones((3, 1), dtype=bool), np.ones(3, dtype=np.int32)):
        with pytest.raises(ValueError):
            silhouette.silhouette_conformers(ITEM, [0, 0, 1], valid=valid)
    with pytest.raises(ValueError):
        silhouette.silhouette_conformers({"atom_type": [6, 6], "pos_gen": np.zeros((0, 3), np.float32)}, [])
    G = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1
    with pytest.raises(_lib.AgdiffLimitError):
        silhouette.silhouette_conformers({"atom_type": np.array([6, 6]), "pos_gen": np.zeros((G, 2, 3), np.float32)}, np.zeros(G, np.int32))


def test_sweep_medoids_checks_its_arguments_before_any_device_work():
    from agdiff_amd import silhouette
    for lo, hi in ((1, 3), (0, 2), (3, 2), (2, 66), (2.5, 3), (2, 3.5), (-1, -1)):
        with pytest.raises(ValueError):
            silhouette.sweep_medoids(ITEM, lo, hi)
    for kw in (dict(init="pam"), dict(init=[0, 1]), dict(max_iter=0), dict(max_iter=129), dict(max_iter=1.5), dict(metric="usr"),
               dict(tfd_rings=True), dict(valid=np.ones(4, dtype=bool))):
        with pytest.raises(ValueError):
            silhouette.sweep_medoids(ITEM, 2, 3, **kw)
    G = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1
    with pytest.raises(_lib.AgdiffLimitError):
        silhouette.sweep_medoids({"atom_type": np.array([6, 6]), "pos_gen": np.zeros((G, 2, 3), np.float32)}, 2, 65)


def test_labels_map_to_ranks_in_ascending_order():
    import torch
    from agdiff_amd.silhouette import label_ranks
    values, ranks = label_ranks([0, 1, 1, 2, -1, 0])                      # ranks as clusters / medoids / picks write them
    assert values.tolist() == [0, 1, 2] and ranks.tolist() == [0, 1, 1, 2, -1, 0] and ranks.dtype == np.int32 and values.dtype == np.int64
    values, ranks = label_ranks(np.array([7, 7, 2, 2, 7, -1, 40, 2], dtype=np.int32))     # kept-conformer indices, as ensemble writes them
    assert values.tolist() == [2, 7, 40] and ranks.tolist() == [1, 1, 0, 0, 1, -1, 2, 0]
    values, ranks = label_ranks(torch.tensor([5, 5, 3], dtype=torch.int64))
    assert values.tolist() == [3, 5] and ranks.tolist() == [1, 1, 0]
    values, ranks = label_ranks(np.array([4, 0, 4], dtype=np.uint8))
    assert values.tolist() == [0, 4] and ranks.tolist() == [1, 0, 1]
    values, ranks = label_ranks(np.full(4, -1))
    assert values.shape == (0,) and ranks.tolist() == [-1] * 4
    values, ranks = label_ranks(np.zeros(0, np.int32))
    assert values.shape == (0,) and ranks.shape == (0,)
    for bad in ([0, -2], [0.0, 1.0], [[0, 1]], "ab", np.array([0, 1 << 31])):
        with pytest.raises(ValueError):
            label_ranks(bad)


def test_parser_flags_and_defaults(capsys):
    from agdiff_amd import silhouette
    base = ["--samples", "s.npz", "--testset", "t.npz", "--out", "o.npz"]
    ap = silhouette._parser()
    a = ap.parse_args(base + ["--labels", "c.npz"])
    assert a.labels == "c.npz" and a.label_key == "cluster" and a.sweep is None and a.tfd is False and a.tfd_rings is False
    assert a.init == "maxmin" and a.max_iter == 32 and a.align is False and a.device == "cuda"
    assert not (a.fix_handedness or a.fix_double_bonds or a.drop_invalid or a.drop_bent)
    assert (a.samples, a.testset, a.out) == ("s.npz", "t.npz", "o.npz")
    a = ap.parse_args(base + ["--labels", "p.npz", "--label-key", "owner", "--tfd", "--tfd-rings", "--drop-invalid"])
    assert a.label_key == "owner" and a.tfd and a.tfd_rings and a.drop_invalid
    a = ap.parse_args(base + ["--sweep", "2", "65", "--init", "first", "--max-iter", "128", "--align", "--drop-bent", "--fix-handedness",
                              "--fix-double-bonds"])
    assert a.sweep == [2, 65] and a.labels is None and a.init == "first" and a.max_iter == 128 and a.align and a.drop_bent
    assert a.fix_handedness and a.fix_double_bonds
    for bad in (base, base + ["--labels", "c.npz", "--sweep", "2", "5"], base + ["--labels", "c.npz", "--tfd-rings"],
                base + ["--sweep", "1", "5"], base + ["--sweep", "0", "0"], base + ["--sweep", "5", "4"], base + ["--sweep", "2", "66"],
                base + ["--sweep", "2"], base + ["--sweep", "2", "3.5"], base + ["--sweep", "2", "5", "--init", "pam"],
                base + ["--sweep", "2", "5", "--max-iter", "0"], base + ["--sweep", "2", "5", "--max-iter", "129"],
                base[2:] + ["--labels", "c.npz"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    capsys.readouterr()


def test_main_hands_its_flags_on(monkeypatch, tmp_path):
    from agdiff_amd import silhouette
    seen = []

    class Stop(Exception):
        pass

    def spy_labels(item, labels, **kw):
        seen.append(("labels", np.asarray(labels).tolist(), kw["metric"], kw["tfd_rings"]))
        raise Stop()

    def spy_sweep(item, lo, hi, **kw):
        seen.append(("sweep", lo, hi, kw["metric"], kw["init"], kw["max_iter"], kw["align"]))
        raise Stop()
    mol = {"index": 0, "name": "m0"}
    monkeypatch.setattr(silhouette, "sampled_items", lambda testset, samples: iter([(mol, {"atom_type": [6], "pos_gen": [[0.0, 0, 0]]})]))
    monkeypatch.setattr(silhouette, "silhouette_conformers", spy_labels)
    monkeypatch.setattr(silhouette, "sweep_medoids", spy_sweep)
    np.savez(str(tmp_path / "c.npz"), cluster_0=np.array([0], np.int32), owner_0=np.array([3], np.int32))
    base = ["--samples", "s.npz", "--testset", "t.npz", "--out", str(tmp_path / "o.npz")]
    for extra, want in ((["--labels", str(tmp_path / "c.npz")], ("labels", [0], "rmsd", False)),
                        (["--labels", str(tmp_path / "c.npz"), "--label-key", "owner", "--tfd", "--tfd-rings"], ("labels", [3], "tfd", True)),
                        (["--sweep", "2", "9"], ("sweep", 2, 9, "rmsd", "maxmin", 32, False)),
                        (["--sweep", "3", "4", "--init", "first", "--max-iter", "7", "--align", "--tfd"], ("sweep", 3, 4, "tfd", "first", 7, True))):
        with pytest.raises(Stop):
            silhouette.main(base + extra)
        assert seen[-1] == want
    with pytest.raises(ValueError):
        silhouette.main(base + ["--labels", str(tmp_path / "c.npz"), "--label-key", "leader"])     # no such key in the file
    with pytest.raises(SystemExit):
        silhouette.main(base)
