"""No GPU: the C ABI of the conformer-ensemble entry points (agdiff_rmsd_self, agdiff_leader_prune, agdiff_align_conformers)
as the header declares it, their host-side argument checks (every one returns before any launch), and the driver's switch."""
import ctypes

import pytest

from agdiff_amd import _lib

VP, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float


def _buf():
    """a non-null, 8-byte aligned host address: the checks under test return before anything is read or launched"""
    b = (ctypes.c_uint64 * 8)()
    return b, ctypes.c_void_p(ctypes.addressof(b))


def test_exports_and_abi_version():
    assert _lib.EXPORTS["agdiff_rmsd_self"] == [VP, VP, VP, I32, I32, I32, I32, F32, VP, VP, VP, VP]
    assert _lib.EXPORTS["agdiff_leader_prune"] == [VP, I32, VP, VP, VP, VP, VP]
    assert _lib.EXPORTS["agdiff_align_conformers"] == [VP, VP, VP, I32, I32, I32, VP, VP, VP]
    assert _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    assert _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] == 4096 == 64 * 64
    lib = _lib.load()
    assert lib.agdiff_abi_version() == 48
    for name in ("agdiff_rmsd_self", "agdiff_leader_prune", "agdiff_align_conformers"):
        assert hasattr(lib, name)


def test_rmsd_self_checks_its_arguments_on_the_host():
    lib = _lib.load()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    ok = dict(pos=p, idx=p, perms=null, G=4, n=5, m=3, P=0, thresh=0.5, scratch=p, out=p, bits=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.agdiff_rmsd_self(a["pos"], a["idx"], a["perms"], a["G"], a["n"], a["m"], a["P"], a["thresh"], a["scratch"],
                                    a["out"], a["bits"], null)
    for bad in (dict(pos=null), dict(idx=null), dict(scratch=null), dict(out=null, bits=null), dict(G=-1), dict(n=0), dict(m=0),
                dict(m=6), dict(perms=p, P=0), dict(thresh=-0.1), dict(thresh=float("nan")),
                dict(bits=ctypes.c_void_p(p.value + 2))):
        assert call(**bad) == -1, bad
    big = _lib.DEFINES["AGDIFF_RMSD_MAX_ATOMS"] + 1
    assert call(n=big + 10, m=big) == -2
    assert call(G=0) == 0                     # nothing to do: no launch
    del keep


def test_leader_prune_checks_its_arguments_on_the_host():
    lib = _lib.load()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    for k in range(5):
        a = [p, p, p, p, p]
        a[k] = null
        assert lib.agdiff_leader_prune(a[0], 8, a[1], a[2], a[3], a[4], null) == -1
    assert lib.agdiff_leader_prune(p, -1, p, p, p, p, null) == -1
    assert lib.agdiff_leader_prune(ctypes.c_void_p(p.value + 4), 8, p, p, p, p, null) == -1
    assert lib.agdiff_leader_prune(p, _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1, p, p, p, p, null) == -2
    with pytest.raises(_lib.AgdiffLimitError):
        _lib.check(lib.agdiff_leader_prune(p, _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1, p, p, p, p, null), "agdiff_leader_prune")
    del keep


def test_align_conformers_checks_its_arguments_on_the_host():
    lib = _lib.load()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    call = lambda pos=p, idx=p, tgt=p, G=2, n=5, m=3, out=p, rmsd=null: lib.agdiff_align_conformers(pos, idx, tgt, G, n, m, out, rmsd, null)
    for bad in (dict(pos=null), dict(idx=null), dict(tgt=null), dict(out=null), dict(G=-1), dict(n=0), dict(m=0), dict(m=6)):
        assert call(**bad) == -1, bad
    assert call(G=0) == 0
    del keep


def test_bit_matrix_pitch():
    from agdiff_amd.ensemble import bits_pitch
    assert [bits_pitch(g) for g in (1, 16, 17, 64, 65, 1000, 4096)] == [8, 8, 8, 8, 16, 128, 512]


def test_thresholds_are_checked_before_any_work():
    from agdiff_amd import ensemble
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            ensemble.prune_conformers({"atom_type": [6, 6], "pos_gen": [[0.0, 0, 0], [1, 0, 0]]}, bad)


def test_driver_takes_the_prune_switch(monkeypatch):
    from agdiff_amd import driver
    with pytest.raises(ValueError):
        driver.run_job(object(), [], "unused", driver.num_confs("1"), 10, {}, "cpu", prune_rms=-1)
    with pytest.raises(ValueError):
        driver.run_job(object(), [], "unused", driver.num_confs("1"), 10, {}, "cpu", prune_rms=float("nan"))
    # the parser: stop main() as soon as it has parsed
    seen = {}

    class Stop(Exception):
        pass

    import argparse
    real = argparse.ArgumentParser.parse_args

    def spy(self, argv=None, *a, **kw):
        seen["args"] = real(self, argv, *a, **kw)
        raise Stop("parsed")
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", spy)
    with pytest.raises(Stop):
        driver.main(["--ckpt", "c.pt", "--testset", "t.npz", "--out", "o", "--prune-rms", "0.5"])
    assert seen["args"].prune_rms == 0.5
    with pytest.raises(Stop):
        driver.main(["--ckpt", "c.pt", "--testset", "t.npz", "--out", "o"])
    assert seen["args"].prune_rms is None
