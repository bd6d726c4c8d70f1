"""No GPU: the C ABI of agdiff_pam_build and agdiff_pam_swap as the header declares it, their host-side argument checks (every one
returns before any launch), the signatures and argument checks of agdiff_amd.pam and the command line's parser."""
import ctypes
import inspect

import numpy as np
import pytest

from agdiff_amd import _lib

VP, I32 = ctypes.c_void_p, ctypes.c_int32
NOUT = 9                                                     # the eight outputs, work


def _buf():
    """a non-null, 8-byte aligned host address: the checks under test return before anything is read or launched"""
    b = (ctypes.c_uint64 * 8)()
    return b, ctypes.c_void_p(ctypes.addressof(b))


def _build(lib, dist, outs, G=8, K=3, anchor=0):
    return lib.agdiff_pam_build(dist, G, K, anchor, *outs, ctypes.c_void_p(0))


def _swap(lib, dist, outs, G=8, K=3, anchor=0, max_swaps=64, init=None):
    return lib.agdiff_pam_swap(dist, G, K, dist if init is None else init, anchor, max_swaps, *outs, ctypes.c_void_p(0))


CALLS = (_build, _swap)


def test_exports_equal_the_headers_declarations():
    assert _lib.EXPORTS["agdiff_pam_build"] == [VP, I32, I32, I32] + [VP] * 10
    assert _lib.EXPORTS["agdiff_pam_swap"] == [VP, I32, I32, VP, I32, I32] + [VP] * 10
    lib = _lib.load()
    for name in ("agdiff_pam_build", "agdiff_pam_swap"):
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.EXPORTS[name]
    assert lib.agdiff_abi_version() == _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    assert _lib.DEFINES["AGDIFF_PAM_MAX_SWAPS"] == 256
    # control words + dn, ds and the records' deltas (64-bit) + tag and the records' ranks (32-bit), one per conformer
    assert _lib.DEFINES["AGDIFF_PAM_WORK_BYTES"] >= 32 + _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] * (3 * 8 + 2 * 4)
    assert _lib.DEFINES["AGDIFF_PAM_WORK_BYTES"] % 8 == 0
    header = open(_lib.HEADER).read()
    assert ("int agdiff_pam_build(const float* dist, int32_t G, int32_t K, int32_t anchor,\n"
            "                     int32_t* medoids, int32_t* labels, float* near, int32_t* size, double* within,\n"
            "                     double* cost, int32_t* n_swaps, int32_t* status, uint64_t* work, void* stream);") in header
    assert ("int agdiff_pam_swap(const float* dist, int32_t G, int32_t K, const int32_t* init, int32_t anchor, int32_t max_swaps,\n"
            "                    int32_t* medoids, int32_t* labels, float* near, int32_t* size, double* within,\n"
            "                    double* cost, int32_t* n_swaps, int32_t* status, uint64_t* work, void* stream);") in header
    for words in ("j == anchor or valid(dist[anchor][j])", "ties to the LOWEST rank", "a gain of 0 still picks",
                  "delta(c, r) = corr(c, r) - gain(c)", "ties to the lowest candidate index, then to the lowest rank",
                  "is memoryless: calling again", "diagonal is never read", "FasterPAM's eager variant",
                  "(PAM is agdiff_pam_build + agdiff_pam_swap, below)"):
        assert words in header, words


@pytest.mark.parametrize("call", CALLS)
def test_entry_points_check_their_arguments_on_the_host(call):
    lib = _lib.load()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    ok = [p] * NOUT
    for k in range(NOUT):
        a = list(ok)
        a[k] = null
        assert call(lib, p, a) == -1, k
        assert call(lib, p, a, G=0) == -1, k                               # (also with nothing to cluster)
    assert call(lib, null, ok) == -1 and call(lib, null, ok, G=0) == -1
    assert call(lib, p, ok, G=-1) == -1
    for K in (0, -1, 9):
        assert call(lib, p, ok, K=K) == -1
    for off in (1, 2, 4):                                                  # a misaligned work
        a = list(ok)
        a[8] = ctypes.c_void_p(p.value + off)
        assert call(lib, p, a) == -1
        assert call(lib, p, a, G=0) == -1
    limit = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"]
    assert limit == 4096
    assert call(lib, p, ok, G=limit + 1, K=limit + 1) == -2
    assert call(lib, p, ok, G=limit + 1, K=1, anchor=-7) == -2             # (the anchor is looked at on the device)
    for K in (0, limit + 2):
        assert call(lib, p, ok, G=limit + 1, K=K) == -1                    # (the argument errors come first)
    a = list(ok)
    a[8] = ctypes.c_void_p(p.value + 4)
    assert call(lib, p, a, G=limit + 1, K=1) == -1
    a = list(ok)
    a[3] = null
    assert call(lib, p, a, G=limit + 1, K=1) == -1
    # nothing to cluster: no launch, and K and the anchor are not looked at
    assert call(lib, p, ok, G=0, K=0, anchor=-5) == 0
    assert call(lib, p, ok, G=0) == 0
    assert call(lib, ctypes.c_void_p(p.value + 4), ok, G=limit + 1, K=1) == -2     # dist needs 4-byte alignment only
    with pytest.raises(_lib.AgdiffLimitError):
        _lib.check(call(lib, p, ok, G=limit + 1, K=1), "agdiff_pam")
    with pytest.raises(_lib.AgdiffHipError):
        _lib.check(call(lib, p, ok, K=0), "agdiff_pam")
    del keep


def test_swap_checks_init_and_max_swaps_on_the_host():
    lib = _lib.load()
    keep, p = _buf()
    ok = [p] * NOUT
    limit = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"]
    assert lib.agdiff_pam_swap(p, 8, 3, ctypes.c_void_p(0), 0, 64, *ok, ctypes.c_void_p(0)) == -1
    assert lib.agdiff_pam_swap(p, 0, 3, ctypes.c_void_p(0), 0, 64, *ok, ctypes.c_void_p(0)) == -1
    for n in (-1, 257, 1 << 20):
        assert _swap(lib, p, ok, max_swaps=n) == -1
        assert _swap(lib, p, ok, G=limit + 1, K=1, max_swaps=n) == -1
    for n in (0, 1, 256):                                                  # 0 is a count: the seeds' assignment
        assert _swap(lib, p, ok, G=limit + 1, K=1, max_swaps=n) == -2
    assert _swap(lib, p, ok, G=0, max_swaps=-3) == 0
    del keep


def test_signatures_and_defaults():
    from agdiff_amd import medoids, pam
    sig = inspect.signature(pam.pam_conformers)
    assert list(sig.parameters) == ["item", "k", "metric", "init", "max_swaps", "chunk", "align", "device", "valid", "fix_handedness",
                                    "fix_double_bonds", "tfd_rings"]
    want = dict(metric="rmsd", init="build", max_swaps=4096, chunk=64, align=True, device="cuda", valid=None, fix_handedness=False,
                fix_double_bonds=False, tfd_rings=False)
    assert {n: p.default for n, p in sig.parameters.items() if n not in ("item", "k")} == want
    assert sig.parameters["k"].default is inspect.Parameter.empty
    sig = inspect.signature(pam.pam_build)
    assert list(sig.parameters) == ["dist", "G", "k", "anchor"] and sig.parameters["anchor"].default == 0
    sig = inspect.signature(pam.pam_swap)
    assert list(sig.parameters) == ["dist", "G", "init", "anchor", "max_swaps"]
    assert sig.parameters["anchor"].default is None and sig.parameters["max_swaps"].default == 64
    assert pam.MAX_SWAPS == 256 and pam.WORK_BYTES == _lib.DEFINES["AGDIFF_PAM_WORK_BYTES"]
    from agdiff_amd.ensemble import _usable_matrix                       # the shared prelude and medoids' result, not copies
    assert pam._usable_matrix is _usable_matrix and pam._result is medoids._result
    assert "agdiff_amd.pam" in medoids.__doc__ and "agdiff_amd.pam" in medoids.medoid_conformers.__doc__


def test_pam_conformers_checks_its_arguments_before_any_device_work():
    from agdiff_amd import pam
    item = {"atom_type": [6, 6], "pos_gen": [[0.0, 0, 0], [1, 0, 0], [0.0, 0, 0], [1.1, 0, 0]]}
    with pytest.raises(ValueError):
        pam.pam_conformers(item, 1, metric="usr")
    with pytest.raises(ValueError):
        pam.pam_conformers(item, 1, tfd_rings=True)                       # (the rings are terms of the TFD)
    for k in (0, -1, 1.5):
        with pytest.raises(ValueError):
            pam.pam_conformers(item, k)
    for n in (-1, 2.5):
        with pytest.raises(ValueError):
            pam.pam_conformers(item, 1, max_swaps=n)
    for c in (0, -1, 257, 2.5):
        with pytest.raises(ValueError):
            pam.pam_conformers(item, 1, chunk=c)
    for init in ("random", "pam", "kmeans++", [0, 0], [0], [0, 1, 1], [0.5, 1], [[0, 1], [1, 0]][:1] * 2):
        with pytest.raises(ValueError):
            pam.pam_conformers(item, 2, init=init)
    for init in ([-1], [2], np.array([5])):
        with pytest.raises(ValueError):
            pam.pam_conformers(item, 1, init=init)
    with pytest.raises(ValueError):
        pam.pam_conformers(item, 1, init=[0], valid=np.array([False, True]))             # a masked seed
    for valid in (np.ones(3, dtype=bool), np.ones((2, 1), dtype=bool), np.ones(2, dtype=np.int32), [1.0, 0.0]):
        with pytest.raises(ValueError):
            pam.pam_conformers(item, 1, valid=valid)
    with pytest.raises(ValueError):
        pam.pam_conformers({"atom_type": [6, 6], "pos_gen": np.zeros((0, 3), np.float32)}, 1)
    G = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1
    with pytest.raises(_lib.AgdiffLimitError):
        pam.pam_conformers({"atom_type": np.array([6, 6]), "pos_gen": np.zeros((G, 2, 3), np.float32)}, 1)


def test_wrappers_check_their_tensors():
    import torch
    from agdiff_amd import pam
    d = torch.zeros((4, 4), dtype=torch.float32)                          # (on the host: refused before any launch)
    with pytest.raises(ValueError):
        pam.pam_build(d, 4, 2)
    with pytest.raises(ValueError):
        pam.pam_build(np.zeros((4, 4), np.float32), 4, 2)
    for k in (0, 1.5):
        with pytest.raises(ValueError):
            pam.pam_build(d, 4, k)
    with pytest.raises(ValueError):
        pam.pam_build(d, 4, 1, anchor=0.5)
    with pytest.raises(ValueError):
        pam.pam_swap(d, 4, torch.zeros(1, dtype=torch.int32))            # init on the host
    with pytest.raises(ValueError):
        pam.pam_swap(d, 4, [0])
    for n in (-1, 257, 1.5):
        with pytest.raises(ValueError):
            pam.pam_swap(d, 4, torch.zeros(1, dtype=torch.int32), max_swaps=n)


def test_parser_flags_and_defaults(capsys):
    from agdiff_amd import pam
    base = ["--samples", "s.npz", "--testset", "t.npz", "--out", "o.npz"]
    ap = pam._parser()
    a = ap.parse_args(base + ["--count", "5"])
    assert a.count == 5 and a.tfd is False and a.tfd_rings is False and a.init == "build" and a.max_swaps == 4096 and a.align is False
    assert a.device == "cuda" and not (a.fix_handedness or a.fix_double_bonds or a.drop_invalid or a.drop_bent)
    assert (a.samples, a.testset, a.out) == ("s.npz", "t.npz", "o.npz")
    a = ap.parse_args(base + ["--count", "4", "--tfd", "--tfd-rings", "--init", "alternate", "--max-swaps", "0", "--align",
                              "--drop-invalid", "--drop-bent", "--fix-handedness", "--fix-double-bonds"])
    assert a.count == 4 and a.tfd and a.tfd_rings and a.init == "alternate" and a.max_swaps == 0 and a.align and a.drop_invalid
    assert a.drop_bent and a.fix_handedness and a.fix_double_bonds
    for init in ("build", "maxmin", "first", "alternate"):
        assert ap.parse_args(base + ["--count", "2", "--init", init]).init == init
    for bad in (base, base + ["--count", "3", "--tfd-rings"], base[2:] + ["--count", "3"], base + ["--count", "1.5"],
                base + ["--count", "0"], base + ["--count", "3", "--init", "pam"], base + ["--count", "3", "--max-swaps", "-1"],
                base + ["--count", "3", "--max-swaps", "1.5"], base + ["--count", "3", "--max-iter", "3"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    capsys.readouterr()


def test_main_hands_its_flags_to_pam_conformers(monkeypatch, tmp_path):
    from agdiff_amd import pam
    seen = []

    class Stop(Exception):
        pass

    def spy(item, k, **kw):
        seen.append((k, kw["metric"], kw["init"], kw["max_swaps"], kw["align"], kw["tfd_rings"]))
        raise Stop()
    mol = {"index": 0, "name": "m0"}
    monkeypatch.setattr(pam, "sampled_items", lambda testset, samples: iter([(mol, {"atom_type": [6], "pos_gen": [[0.0, 0, 0]]})]))
    monkeypatch.setattr(pam, "pam_conformers", spy)
    base = ["--samples", "s.npz", "--testset", "t.npz", "--out", str(tmp_path / "o.npz")]
    for extra, want in ((["--count", "10"], (10, "rmsd", "build", 4096, False, False)),
                        (["--count", "2", "--align", "--init", "first", "--max-swaps", "7"], (2, "rmsd", "first", 7, True, False)),
                        (["--count", "3", "--tfd", "--tfd-rings", "--init", "alternate"], (3, "tfd", "alternate", 4096, False, True))):
        with pytest.raises(Stop):
            pam.main(base + extra)
        assert seen[-1] == want
    with pytest.raises(SystemExit):
        pam.main(base)
