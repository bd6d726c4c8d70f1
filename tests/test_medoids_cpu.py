"""No GPU: the C ABI of agdiff_kmedoids as the header declares it, its host-side argument checks (every one returns before any
launch), the signatures and argument checks of agdiff_amd.medoids and the command line's parser."""
import ctypes
import inspect

import numpy as np
import pytest

from agdiff_amd import _lib

VP, I32 = ctypes.c_void_p, ctypes.c_int32
NPTR = 11                                                    # dist, init, the eight outputs, work


def _buf():
    """a non-null, 8-byte aligned host address: the checks under test return before anything is read or launched"""
    b = (ctypes.c_uint64 * 8)()
    return b, ctypes.c_void_p(ctypes.addressof(b))


def _call(lib, a, G=8, K=3, max_iter=32):
    return lib.agdiff_kmedoids(a[0], G, K, a[1], max_iter, a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], ctypes.c_void_p(0))


def test_export_equals_the_headers_declaration():
    assert _lib.EXPORTS["agdiff_kmedoids"] == [VP, I32, I32, VP, I32, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP]
    lib = _lib.load()
    assert hasattr(lib, "agdiff_kmedoids") and lib.agdiff_kmedoids.argtypes == _lib.EXPORTS["agdiff_kmedoids"]
    assert lib.agdiff_abi_version() == _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    assert _lib.DEFINES["AGDIFF_KMEDOIDS_MAX_DIST"] == 4096 and _lib.DEFINES["AGDIFF_KMEDOIDS_MAX_ITER"] == 128
    assert _lib.DEFINES["AGDIFF_KMEDOIDS_WORK_BYTES"] == 131072
    header = open(_lib.HEADER).read()
    assert ("int agdiff_kmedoids(const float* dist, int32_t G, int32_t K, const int32_t* init, int32_t max_iter,\n"
            "                    int32_t* medoids, int32_t* labels, float* near, int32_t* size, double* within,\n"
            "                    double* cost, int32_t* n_iter, int32_t* status, uint64_t* work, void* stream);") in header
    for words in ("x >= 0.0f && x <= 4096.0f", "rounding half to even", "Q(x) = 2^40", "j == init[0] or valid(dist[init[0]][j])",
                  "ties to the LOWEST rank", "ties to the LOWEST index", "THE INCUMBENT STAYS", "counting the one that changed nothing",
                  "after a status = 1 stop one more assign runs", "diagonal is never read","-0.0f written as +0.0f",
                  "not PAM's swap phase"):
        assert words in header, words


def test_kmedoids_checks_its_arguments_on_the_host():
    lib = _lib.load()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    for k in range(NPTR):
        a = [p] * NPTR
        a[k] = null
        assert _call(lib, a) == -1, k
        assert _call(lib, a, G=0) == -1, k                                 # (also with nothing to cluster)
    ok = [p] * NPTR
    assert _call(lib, ok, G=-1) == -1
    for K in (0, -1, 9):
        assert _call(lib, ok, K=K) == -1
    for it in (0, -1, 129, 1 << 20):
        assert _call(lib, ok, max_iter=it) == -1
    for off in (1, 2, 4):                                                  # a misaligned work
        a = [p] * NPTR
        a[10] = ctypes.c_void_p(p.value + off)
        assert _call(lib, a) == -1
        assert _call(lib, a, G=0) == -1
    limit = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"]
    assert limit == 4096
    assert _call(lib, ok, G=limit + 1, K=limit + 1) == -2
    assert _call(lib, ok, G=limit + 1, K=1, max_iter=128) == -2
    for kw in (dict(K=0), dict(K=limit + 2), dict(max_iter=0), dict(max_iter=129)):
        assert _call(lib, ok, **dict(dict(G=limit + 1, K=1), **kw)) == -1  # (the argument errors come first)
    a = [p] * NPTR
    a[10] = ctypes.c_void_p(p.value + 4)
    assert _call(lib, a, G=limit + 1, K=1) == -1
    a = [p] * NPTR
    a[5] = null
    assert _call(lib, a, G=limit + 1, K=1) == -1
    # nothing to cluster: no launch, and K and max_iter are not looked at
    assert _call(lib, ok, G=0, K=0, max_iter=-5) == 0
    assert _call(lib, ok, G=0) == 0
    with pytest.raises(_lib.AgdiffLimitError):
        _lib.check(_call(lib, ok, G=limit + 1, K=1), "agdiff_kmedoids")
    with pytest.raises(_lib.AgdiffHipError):
        _lib.check(_call(lib, ok, K=0), "agdiff_kmedoids")
    del keep


def test_unaligned_dist_is_not_an_argument_error():
    """dist needs 4-byte alignment only: an address one float into an allocation passes the checks (here: up to the limit check)"""
    lib = _lib.load()
    keep, p = _buf()
    a = [p] * NPTR
    a[0] = ctypes.c_void_p(p.value + 4)
    assert _call(lib, a, G=_lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1, K=1) == -2
    assert _call(lib, a, G=0) == 0
    del keep


def test_signatures_and_defaults():
    from agdiff_amd import medoids, picks
    sig = inspect.signature(medoids.medoid_conformers)
    assert list(sig.parameters) == ["item", "k", "metric", "init", "max_iter", "align", "device", "valid", "fix_handedness",
                                    "fix_double_bonds", "tfd_rings"]
    want = dict(metric="rmsd", init="maxmin", max_iter=32, align=True, device="cuda", valid=None, fix_handedness=False,
                fix_double_bonds=False, tfd_rings=False)
    assert {n: p.default for n, p in sig.parameters.items() if n not in ("item", "k")} == want
    assert sig.parameters["k"].default is inspect.Parameter.empty
    sig = inspect.signature(medoids.kmedoids)
    assert list(sig.parameters) == ["dist", "G", "init", "max_iter"] and sig.parameters["max_iter"].default == 32
    assert medoids.MAX_ITER == 128 and medoids.WORK_BYTES == 131072
    from agdiff_amd.ensemble import _usable_matrix                       # the prelude that picks shares
    assert picks._usable_matrix is _usable_matrix is medoids._usable_matrix


def test_medoid_conformers_checks_its_arguments_before_any_device_work():
    from agdiff_amd import medoids
    item = {"atom_type": [6, 6], "pos_gen": [[0.0, 0, 0], [1, 0, 0], [0.0, 0, 0], [1.1, 0, 0]]}
    with pytest.raises(ValueError):
        medoids.medoid_conformers(item, 1, metric="usr")
    with pytest.raises(ValueError):
        medoids.medoid_conformers(item, 1, tfd_rings=True)                # (the rings are terms of the TFD)
    for k in (0, -1, 1.5):
        with pytest.raises(ValueError):
            medoids.medoid_conformers(item, k)
    for it in (0, -1, 129, 2.5):
        with pytest.raises(ValueError):
            medoids.medoid_conformers(item, 1, max_iter=it)
    for init in ("random", "pam", [0, 0], [0], [0, 1, 1], [0.5, 1], [[0, 1], [1, 0]][:1] * 2):
        with pytest.raises(ValueError):
            medoids.medoid_conformers(item, 2, init=init)
    for init in ([-1], [2], np.array([5])):
        with pytest.raises(ValueError):
            medoids.medoid_conformers(item, 1, init=init)
    with pytest.raises(ValueError):
        medoids.medoid_conformers(item, 1, init=[0], valid=np.array([False, True]))      # a masked seed
    for valid in (np.ones(3, dtype=bool), np.ones((2, 1), dtype=bool), np.ones(2, dtype=np.int32), [1.0, 0.0]):
        with pytest.raises(ValueError):
            medoids.medoid_conformers(item, 1, valid=valid)
    with pytest.raises(ValueError):
        medoids.medoid_conformers({"atom_type": [6, 6], "pos_gen": np.zeros((0, 3), np.float32)}, 1)
    G = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1
    with pytest.raises(_lib.AgdiffLimitError):
        medoids.medoid_conformers({"atom_type": np.array([6, 6]), "pos_gen": np.zeros((G, 2, 3), np.float32)}, 1)


def test_kmedoids_wrapper_checks_its_tensors():
    import torch
    from agdiff_amd import medoids
    d = torch.zeros((4, 4), dtype=torch.float32)                          # (on the host: refused before any launch)
    with pytest.raises(ValueError):
        medoids.kmedoids(d, 4, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        medoids.kmedoids(np.zeros((4, 4), np.float32), 4, torch.zeros(1, dtype=torch.int32))


def test_parser_flags_and_defaults(capsys):
    from agdiff_amd import medoids
    base = ["--samples", "s.npz", "--testset", "t.npz", "--out", "o.npz"]
    ap = medoids._parser()
    a = ap.parse_args(base + ["--count", "5"])
    assert a.count == 5 and a.tfd is False and a.tfd_rings is False and a.init == "maxmin" and a.max_iter == 32 and a.align is False
    assert a.device == "cuda" and not (a.fix_handedness or a.fix_double_bonds or a.drop_invalid or a.drop_bent)
    assert (a.samples, a.testset, a.out) == ("s.npz", "t.npz", "o.npz")
    a = ap.parse_args(base + ["--count", "4", "--tfd", "--tfd-rings", "--init", "first", "--max-iter", "128", "--align", "--drop-invalid",
                              "--drop-bent", "--fix-handedness", "--fix-double-bonds"])
    assert a.count == 4 and a.tfd and a.tfd_rings and a.init == "first" and a.max_iter == 128 and a.align and a.drop_invalid
    assert a.drop_bent and a.fix_handedness and a.fix_double_bonds
    for bad in (base, base + ["--count", "3", "--tfd-rings"], base[2:] + ["--count", "3"], base + ["--count", "1.5"],
                base + ["--count", "0"], base + ["--count", "3", "--init", "pam"], base + ["--count", "3", "--max-iter", "0"],
                base + ["--count", "3", "--max-iter", "129"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    capsys.readouterr()


def test_main_hands_its_flags_to_medoid_conformers(monkeypatch, tmp_path):
    from agdiff_amd import medoids
    seen = []

    class Stop(Exception):
        pass

    def spy(item, k, **kw):
        seen.append((k, kw["metric"], kw["init"], kw["max_iter"], kw["align"], kw["tfd_rings"]))
        raise Stop()
    mol = {"index": 0, "name": "m0"}
    monkeypatch.setattr(medoids, "sampled_items", lambda testset, samples: iter([(mol, {"atom_type": [6], "pos_gen": [[0.0, 0, 0]]})]))
    monkeypatch.setattr(medoids, "medoid_conformers", spy)
    base = ["--samples", "s.npz", "--testset", "t.npz", "--out", str(tmp_path / "o.npz")]
    for extra, want in ((["--count", "10"], (10, "rmsd", "maxmin", 32, False, False)),
                        (["--count", "2", "--align", "--init", "first", "--max-iter", "7"], (2, "rmsd", "first", 7, True, False)),
                        (["--count", "3", "--tfd", "--tfd-rings"], (3, "tfd", "maxmin", 32, False, True))):
        with pytest.raises(Stop):
            medoids.main(base + extra)
        assert seen[-1] == want
    with pytest.raises(SystemExit):
        medoids.main(base)
