"""No GPU: the C ABI of agdiff_maxmin_pick as the header declares it, its host-side argument checks (every one returns before any
launch), the argument checks of agdiff_amd.picks.pick_conformers and the command line's parser."""
import ctypes
import inspect

import numpy as np
import pytest

from agdiff_amd import _lib

VP, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float


def _buf():
    """a non-null host address: the checks under test return before anything is read or launched"""
    b = (ctypes.c_uint64 * 8)()
    return b, ctypes.c_void_p(ctypes.addressof(b))


def test_export_equals_the_headers_declaration():
    assert _lib.EXPORTS["agdiff_maxmin_pick"] == [VP, I32, I32, I32, F32, VP, VP, VP, VP, VP, VP, VP]
    lib = _lib.load()
    assert hasattr(lib, "agdiff_maxmin_pick") and lib.agdiff_maxmin_pick.argtypes == _lib.EXPORTS["agdiff_maxmin_pick"]
    assert lib.agdiff_abi_version() == _lib.DEFINES["AGDIFF_ABI_VERSION"]
    header = open(_lib.HEADER).read()
    assert ("int agdiff_maxmin_pick(const float* dist, int32_t G, int32_t K, int32_t first, float stop, int32_t* picks, "
            "float* radius,\n                       int32_t* owner, float* near, int32_t* n_picked, float* cover, void* stream);") in header
    for words in ("ties to the LOWEST index", "a strict <", "near[candidate] > stop (strict)", "INELIGIBLE FOR GOOD",
                  "-0.0f counts as 0", "stays with\n *     the EARLIER pick"):
        assert words in header, words


def test_maxmin_pick_checks_its_arguments_on_the_host():
    lib = _lib.load()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    call = lambda a, G=8, K=3, first=0, stop=-1.0: lib.agdiff_maxmin_pick(a[0], G, K, first, stop, a[1], a[2], a[3], a[4], a[5], a[6], null)
    for k in range(7):
        a = [p] * 7
        a[k] = null
        assert call(a) == -1, k
        assert call(a, G=0) == -1, k                                     # (also with nothing to pick from)
    ok = [p] * 7
    assert call(ok, G=-1) == -1
    for K in (0, -1, 9):
        assert call(ok, K=K) == -1
    for first in (-1, 8, 1 << 20):
        assert call(ok, first=first) == -1
    assert call(ok, stop=float("nan")) == -1
    limit = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"]
    assert limit == 4096
    assert call(ok, G=limit + 1, K=limit + 1, first=limit) == -2
    assert call(ok, G=limit + 1, K=1) == -2
    for kw in (dict(K=0), dict(K=limit + 2), dict(first=limit + 1), dict(first=-1), dict(stop=float("nan"))):
        assert call(ok, **dict(dict(G=limit + 1, K=1), **kw)) == -1       # (the argument errors come first)
    a = [p] * 7
    a[3] = null
    assert call(a, G=limit + 1, K=1) == -1
    # nothing to pick from: no launch, and K, first and stop are not looked at
    assert call(ok, G=0, K=0, first=-5, stop=float("nan")) == 0
    assert call(ok, G=0) == 0
    with pytest.raises(_lib.AgdiffLimitError):
        _lib.check(call(ok, G=limit + 1, K=1), "agdiff_maxmin_pick")
    with pytest.raises(_lib.AgdiffHipError):
        _lib.check(call(ok, K=0), "agdiff_maxmin_pick")
    del keep


def test_unaligned_dist_is_not_an_argument_error():
    """dist needs 4-byte alignment only: an address one float into an allocation passes the checks (here: up to the limit check)"""
    lib = _lib.load()
    keep, p = _buf()
    limit = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"]
    off = ctypes.c_void_p(p.value + 4)
    assert lib.agdiff_maxmin_pick(off, limit + 1, 1, 0, -1.0, p, p, p, p, p, p, ctypes.c_void_p(0)) == -2
    assert lib.agdiff_maxmin_pick(off, 0, 1, 0, -1.0, p, p, p, p, p, p, ctypes.c_void_p(0)) == 0
    del keep


def test_pick_conformers_signature():
    from agdiff_amd import picks
    sig = inspect.signature(picks.pick_conformers)
    assert list(sig.parameters) == ["item", "k", "radius", "metric", "first", "align", "device", "valid", "fix_handedness",
                                    "fix_double_bonds", "tfd_rings"]
    want = dict(k=None, radius=None, metric="rmsd", first=None, align=True, device="cuda", valid=None, fix_handedness=False,
                fix_double_bonds=False, tfd_rings=False)
    assert {n: p.default for n, p in sig.parameters.items() if n != "item"} == want
    sig = inspect.signature(picks.maxmin_pick)
    assert list(sig.parameters) == ["dist", "G", "k", "stop", "first"]
    assert sig.parameters["stop"].default == -1.0 and sig.parameters["first"].default == 0


def test_pick_conformers_checks_its_arguments_before_any_device_work():
    from agdiff_amd import picks
    item = {"atom_type": [6, 6], "pos_gen": [[0.0, 0, 0], [1, 0, 0], [0.0, 0, 0], [1.1, 0, 0]]}
    with pytest.raises(ValueError):
        picks.pick_conformers(item, k=1, metric="usr")
    with pytest.raises(ValueError):
        picks.pick_conformers(item, k=1, tfd_rings=True)                  # (the rings are terms of the TFD)
    with pytest.raises(ValueError):
        picks.pick_conformers(item)                                       # neither k nor radius
    for k in (0, -1, 1.5):
        with pytest.raises(ValueError):
            picks.pick_conformers(item, k=k)
    for radius in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            picks.pick_conformers(item, radius=radius)
    for valid in (np.ones(3, dtype=bool), np.ones((2, 1), dtype=bool), np.ones(2, dtype=np.int32), [1.0, 0.0]):
        with pytest.raises(ValueError):
            picks.pick_conformers(item, k=1, valid=valid)
    with pytest.raises(ValueError):
        picks.pick_conformers(item, k=1, first=0, valid=np.array([False, True]))      # a masked first
    for first in (-1, 2, 0.5):
        with pytest.raises(ValueError):
            picks.pick_conformers(item, k=1, first=first)
    with pytest.raises(ValueError):
        picks.pick_conformers({"atom_type": [6, 6], "pos_gen": np.zeros((0, 3), np.float32)}, k=1)
    G = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1
    with pytest.raises(_lib.AgdiffLimitError):
        picks.pick_conformers({"atom_type": np.array([6, 6]), "pos_gen": np.zeros((G, 2, 3), np.float32)}, k=1)


def test_parser_flags_and_defaults(capsys):
    from agdiff_amd import picks
    base = ["--samples", "s.npz", "--testset", "t.npz", "--out", "o.npz"]
    ap = picks._parser()
    a = ap.parse_args(base + ["--count", "10"])
    assert a.count == 10 and a.radius is None and a.tfd is False and a.tfd_rings is False and a.first is None and a.align is False
    assert a.device == "cuda" and not (a.fix_handedness or a.fix_double_bonds or a.drop_invalid or a.drop_bent)
    assert (a.samples, a.testset, a.out) == ("s.npz", "t.npz", "o.npz")
    a = ap.parse_args(base + ["--radius", "0.5"])
    assert a.count is None and a.radius == 0.5
    a = ap.parse_args(base + ["--count", "4", "--radius", "0.2", "--tfd", "--tfd-rings", "--first", "3", "--align", "--drop-invalid",
                              "--drop-bent", "--fix-handedness", "--fix-double-bonds"])
    assert a.count == 4 and a.radius == 0.2 and a.tfd and a.tfd_rings and a.first == 3 and a.align and a.drop_invalid and a.drop_bent
    assert a.fix_handedness and a.fix_double_bonds
    for bad in (base, base + ["--count", "3", "--tfd-rings"], base[2:] + ["--count", "3"], base + ["--count", "1.5"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    capsys.readouterr()


def test_main_hands_its_flags_to_pick_conformers(monkeypatch, tmp_path):
    from agdiff_amd import picks
    seen = []

    class Stop(Exception):
        pass

    def spy(item, **kw):
        seen.append((kw["k"], kw["radius"], kw["metric"], kw["first"], kw["align"], kw["tfd_rings"]))
        raise Stop()
    mol = {"index": 0, "name": "m0"}
    monkeypatch.setattr(picks, "sampled_items", lambda testset, samples: iter([(mol, {"atom_type": [6], "pos_gen": [[0.0, 0, 0]]})]))
    monkeypatch.setattr(picks, "pick_conformers", spy)
    base = ["--samples", "s.npz", "--testset", "t.npz", "--out", str(tmp_path / "o.npz")]
    for extra, want in ((["--count", "10"], (10, None, "rmsd", None, False, False)),
                        (["--radius", "0.5", "--align", "--first", "2"], (None, 0.5, "rmsd", 2, True, False)),
                        (["--count", "3", "--radius", "0.1", "--tfd", "--tfd-rings"], (3, 0.1, "tfd", None, False, True))):
        with pytest.raises(Stop):
            picks.main(base + extra)
        assert seen[-1] == want
    with pytest.raises(ValueError):
        picks.main(base + ["--radius", "-1"])
    with pytest.raises(SystemExit):
        picks.main(base)
