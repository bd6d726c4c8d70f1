"""No GPU: the C ABI of agdiff_butina_cluster as the header declares it, its host-side argument checks (every one returns before any
launch), the argument checks of agdiff_amd.clusters.cluster_conformers and the command line's parser."""
import ctypes

import numpy as np
import pytest

from agdiff_amd import _lib

VP, I32 = ctypes.c_void_p, ctypes.c_int32


def _buf():
    """a non-null, 8-byte aligned host address: the checks under test return before anything is read or launched"""
    b = (ctypes.c_uint64 * 8)()
    return b, ctypes.c_void_p(ctypes.addressof(b))


def test_export_and_abi_version():
    assert _lib.EXPORTS["agdiff_butina_cluster"] == [VP, I32, I32, VP, VP, VP, VP, VP]
    assert _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    lib = _lib.load()
    assert lib.agdiff_abi_version() == 48
    assert hasattr(lib, "agdiff_butina_cluster")


def test_butina_cluster_checks_its_arguments_on_the_host():
    lib = _lib.load()
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    for k in range(5):
        a = [p, p, p, p, p]
        a[k] = null
        assert lib.agdiff_butina_cluster(a[0], 8, 1, a[1], a[2], a[3], a[4], null) == -1, k
    assert lib.agdiff_butina_cluster(p, -1, 1, p, p, p, p, null) == -1
    for misaligned in (1, 2, 4):
        assert lib.agdiff_butina_cluster(ctypes.c_void_p(p.value + misaligned), 8, 1, p, p, p, p, null) == -1
    for reorder in (-1, 2, 7):
        assert lib.agdiff_butina_cluster(p, 8, reorder, p, p, p, p, null) == -1
    limit = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"]
    for reorder in (0, 1):
        assert lib.agdiff_butina_cluster(p, limit + 1, reorder, p, p, p, p, null) == -2
        assert lib.agdiff_butina_cluster(p, 0, reorder, p, p, p, p, null) == 0          # nothing to cluster: no launch
    assert lib.agdiff_butina_cluster(p, limit + 1, 2, p, p, p, p, null) == -1           # (the argument errors come first)
    with pytest.raises(_lib.AgdiffLimitError):
        _lib.check(lib.agdiff_butina_cluster(p, limit + 1, 1, p, p, p, p, null), "agdiff_butina_cluster")
    del keep


def test_cluster_conformers_checks_its_arguments_before_any_device_work():
    from agdiff_amd import clusters
    item = {"atom_type": [6, 6], "pos_gen": [[0.0, 0, 0], [1, 0, 0], [0.0, 0, 0], [1.1, 0, 0]]}
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            clusters.cluster_conformers(item, bad)
    with pytest.raises(ValueError):
        clusters.cluster_conformers(item, 0.5, metric="usr")
    for valid in (np.ones(3, dtype=bool), np.ones((2, 1), dtype=bool), np.ones(2, dtype=np.int32), [1.0, 0.0]):
        with pytest.raises(ValueError):
            clusters.cluster_conformers(item, 0.5, valid=valid)
    with pytest.raises(ValueError):
        clusters.cluster_conformers({"atom_type": [6, 6], "pos_gen": np.zeros((0, 3), np.float32)}, 0.5)


def test_parser_takes_exactly_one_threshold_and_passes_static_through(capsys):
    from agdiff_amd import clusters
    base = ["--samples", "s.npz", "--testset", "t.npz", "--out", "o.npz"]
    ap = clusters._parser()
    a = ap.parse_args(base + ["--rms", "0.5"])
    assert a.rms == 0.5 and a.tfd is None and a.static is False and a.align is False and a.device == "cuda"
    a = ap.parse_args(base + ["--tfd", "0.2", "--static", "--align", "--drop-invalid", "--drop-bent", "--fix-handedness",
                              "--fix-double-bonds"])
    assert a.tfd == 0.2 and a.rms is None and a.static is True and a.align and a.drop_invalid and a.drop_bent
    assert a.fix_handedness and a.fix_double_bonds
    for bad in (base, base + ["--rms", "0.5", "--tfd", "0.2"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    capsys.readouterr()


def test_main_hands_static_to_cluster_conformers_as_reorder_false(monkeypatch, tmp_path):
    from agdiff_amd import clusters
    seen = []

    class Stop(Exception):
        pass

    def spy(item, threshold, **kw):
        seen.append((threshold, kw["metric"], kw["reorder"]))
        raise Stop()
    mol = {"index": 0, "name": "m0"}
    monkeypatch.setattr(clusters, "sampled_items", lambda testset, samples: iter([(mol, {"atom_type": [6], "pos_gen": [[0.0, 0, 0]]})]))
    monkeypatch.setattr(clusters, "cluster_conformers", spy)
    base = ["--samples", "s.npz", "--testset", "t.npz", "--out", str(tmp_path / "o.npz")]
    for extra, want in ((["--rms", "0.5"], (0.5, "rmsd", True)), (["--rms", "0.5", "--static"], (0.5, "rmsd", False)),
                        (["--tfd", "0.2", "--static"], (0.2, "tfd", False))):
        with pytest.raises(Stop):
            clusters.main(base + extra)
        assert seen[-1] == want
    with pytest.raises(ValueError):
        clusters.main(base + ["--rms", "-1"])
