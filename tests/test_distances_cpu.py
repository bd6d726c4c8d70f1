"""No GPU: the float64 reference of the distance-distribution MMD (tests/mmd_ref.py) against closed values and its own symmetries,
the host side of agdiff_amd.distances (pair lists, nan-aware summaries, the command line with the kernel calls stubbed by the
reference), and the C ABI's two new entry points as the built library exports them."""
import ctypes

import numpy as np
import pytest
import torch

import mmd_ref as MR
from agdiff_amd import _lib, distances

VP, I32 = ctypes.c_void_p, ctypes.c_int32


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("d", [0.5, 1.0, 3.25])
def test_reference_closed_value_of_two_points(d):
    x, y = np.zeros((1, 1), np.float32), np.full((1, 1), d, np.float32)
    m, b = MR.mmd_all(x, y)
    assert abs(b - d * d) <= 1e-15 * d * d
    assert abs(m - MR.CLOSED_K) <= 1e-14
    ms, bs = MR.mmd_single(x, y)
    assert ms.shape == (1,) and abs(ms[0] - MR.CLOSED_K) <= 1e-14 and abs(bs[0] - d * d) <= 1e-15 * d * d
    assert 6.18 < MR.CLOSED_K < 6.20


@pytest.mark.parametrize("R,G,K", [(1, 1, 1), (3, 5, 3), (17, 33, 65), (40, 70, 300)])
def test_reference_bandwidth_equals_the_closed_form(R, G, K):
    x, y = MR.tables(R, G, K, seed=R + G + K)
    z = np.concatenate([x, y]).astype(np.float64)
    direct, closed = MR.bandwidth_direct(MR.sq_dists(z)), MR.bandwidth_closed(z)
    assert direct > 0 and abs(direct - closed) <= 1e-12 * direct
    for k in (0, K - 1):
        zk = z[:, k:k + 1]
        assert abs(MR.bandwidth_direct(MR.sq_dists(zk)) - MR.bandwidth_closed(zk)) <= 1e-12 * MR.bandwidth_closed(zk)


def test_reference_is_zero_on_equal_sets_and_symmetric_under_the_swap():
    x, y = MR.tables(7, 12, 9, seed=5)
    assert abs(MR.mmd_all(x, x)[0]) <= 1e-14
    assert np.abs(MR.mmd_single(x, x)[0]).max() <= 1e-14
    (a, ba), (b, bb) = MR.mmd_all(x, y), MR.mmd_all(y, x)
    assert a > 1e-3 and abs(a - b) <= 1e-13 and abs(ba - bb) <= 1e-13 * ba
    sa, sb = MR.mmd_single(x, y)[0], MR.mmd_single(y, x)[0]
    assert np.abs(sa - sb).max() <= 1e-13


def test_reference_degenerate_and_non_finite_inputs():
    same = np.full((3, 4), 1.5, np.float32)
    assert MR.mmd_all(same, same[:2]) == (0.0, 0.0)
    x, y = MR.tables(4, 6, 5, seed=2)
    y = y.copy()
    y[3, 2] = np.nan
    assert np.isnan(MR.mmd_all(x, y)[0])
    s, b = MR.mmd_single(x, y)
    assert np.isnan(s[2]) and np.isnan(b[2]) and np.isfinite(np.delete(s, 2)).all()
    x2 = x.copy()
    x2[:, 1] = 2.0
    y2 = y.copy()
    y2[:, 1] = 2.0
    assert MR.mmd_single(x2, y2)[0][1] == 0.0
    assert MR.within_gate([1.0, np.nan], [1.0 + 1e-7, np.nan]) and not MR.within_gate([1.0], [1.0 + 3e-7])
    assert not MR.within_gate([np.nan], [1.0]) and not MR.within_gate([1.0], [np.nan])


# ------------------------------------------------------------------------------------------------ host side of the module
def test_pair_list_order_and_ignore_h():
    at = np.array([6, 1, 8, 1, 7])
    assert distances.pair_list(at).tolist() == [[0, 2], [0, 4], [2, 4]]
    assert distances.pair_list(at).dtype == np.int32
    full = distances.pair_list(at, ignore_h=False)
    assert full.tolist() == [[i, j] for i in range(5) for j in range(i + 1, 5)]
    assert distances.pair_list(np.array([6, 1, 1])).shape == (0, 2)
    assert distances.pair_list(np.array([1, 1]), ignore_h=False).tolist() == [[0, 1]]
    n = 25
    assert distances.pair_list(np.full(n, 6)).shape == (n * (n - 1) // 2, 2)


def test_nan_aware_summaries():
    assert distances.summarise([0.1, 0.4, 0.2]) == (pytest.approx(0.7 / 3), pytest.approx(0.2), 0)
    mean, median, n_nan = distances.summarise(np.array([0.1, np.nan, 0.5, np.nan], dtype=np.float32))
    assert mean == pytest.approx(0.3, rel=1e-6) and median == pytest.approx(0.3, rel=1e-6) and n_nan == 2
    mean, median, n_nan = distances.summarise([np.nan])
    assert np.isnan(mean) and np.isnan(median) and n_nan == 1
    mean, median, n_nan = distances.summarise([])
    assert np.isnan(mean) and np.isnan(median) and n_nan == 0


def _stub_kernels(monkeypatch):
    """the three GPU calls of distance_mmd replaced by the float64 reference on CPU tensors"""
    def table(pos, pairs):
        p = pos.numpy().astype(np.float64)
        q = np.asarray(pairs).reshape(-1, 2)
        return torch.from_numpy(np.sqrt(((p[:, q[:, 0]] - p[:, q[:, 1]]) ** 2).sum(-1)).astype(np.float32))

    def m_all(tr, tg):
        m, b = MR.mmd_all(tr.numpy(), tg.numpy())
        return torch.tensor([m], dtype=torch.float32), torch.tensor([b], dtype=torch.float32)

    def m_single(tr, tg):
        m, b = MR.mmd_single(tr.numpy(), tg.numpy())
        return torch.from_numpy(m.astype(np.float32)), torch.from_numpy(b.astype(np.float32))

    monkeypatch.setattr(distances, "distance_table", table)
    monkeypatch.setattr(distances, "mmd_all", m_all)
    monkeypatch.setattr(distances, "mmd_single", m_single)


def _molecules(seed=0):
    rng = np.random.default_rng(seed)
    mols = []
    for n, R, G in ((6, 3, 5), (4, 2, 4)):
        at = np.array([6, 1, 8, 7, 1, 6][:n])
        base = rng.normal(size=(1, n, 3)) * 1.5
        ref = (base + 0.1 * rng.normal(size=(R, n, 3))).astype(np.float32)
        gen = (1.1 * base + 0.1 * rng.normal(size=(G, n, 3))).astype(np.float32)
        mols.append((at, ref, gen))
    return mols


def test_distance_mmd_puts_the_pieces_together(monkeypatch):
    _stub_kernels(monkeypatch)
    at, ref, gen = _molecules()[0]
    gen = gen.copy()
    res = distances.distance_mmd({"atom_type": at, "pos_ref": ref.reshape(-1, 3), "pos_gen": gen}, device="cpu", want_tables=True)
    K = 4 * 3 // 2
    assert set(res) >= {"all", "single", "single_mean", "single_median", "bandwidth_all", "pairs", "n_nan_columns"}
    assert res["pairs"].tolist() == distances.pair_list(at).tolist() and res["single"].shape == (K,) and res["n_nan_columns"] == 0
    assert res["table_ref"].shape == (3, K) and res["table_gen"].shape == (5, K)
    want_all, want_b = MR.mmd_all(res["table_ref"], res["table_gen"])
    assert res["all"] == pytest.approx(want_all, rel=1e-6) and res["bandwidth_all"] == pytest.approx(want_b, rel=1e-6)
    assert res["single_mean"] == pytest.approx(float(res["single"].astype(np.float64).mean()))
    assert res["single_median"] == pytest.approx(float(np.median(res["single"].astype(np.float64))))
    gen[2, 0] = np.nan                                # heavy atom 0: the pairs (0, 2), (0, 3), (0, 5)
    bad = distances.distance_mmd({"atom_type": at, "pos_ref": ref, "pos_gen": gen}, device="cpu")
    assert "table_ref" not in bad and "table_gen" not in bad
    assert bad["n_nan_columns"] == 3 and np.isnan(bad["all"]) and np.isfinite(bad["single_mean"])
    assert np.isnan(bad["single"][:3]).all() and np.array_equal(bad["single"][3:], res["single"][3:])
    with_h = distances.distance_mmd({"atom_type": at, "pos_ref": ref, "pos_gen": gen}, ignore_h=False, device="cpu")
    assert with_h["single"].shape == (15,)
    lone = distances.distance_mmd({"atom_type": np.array([8, 1, 1]), "pos_ref": np.zeros((2, 3, 3)), "pos_gen": np.ones((1, 3, 3))},
                                  device="cpu")
    assert np.isnan(lone["all"]) and lone["single"].shape == (0,) and lone["pairs"].shape == (0, 2)
    with pytest.raises(ValueError):
        distances.distance_mmd({"atom_type": at, "pos_ref": ref, "pos_gen": gen[:0]}, device="cpu")


def test_command_line_parsing_and_npz_round_trip(monkeypatch, tmp_path, capsys):
    _stub_kernels(monkeypatch)
    samples, refs = {}, {}
    for i, (at, ref, gen) in enumerate(_molecules(3)):
        refs["pos_ref_%d" % i], refs["atom_type_%d" % i], samples["pos_gen_%d" % i] = ref, at, gen
    refs["pos_ref_7"], refs["atom_type_7"] = refs["pos_ref_0"], refs["atom_type_0"]          # (no samples for it: left out)
    np.savez(tmp_path / "samples.npz", **samples)
    np.savez(tmp_path / "refs.npz", **refs)
    base = ["--samples", str(tmp_path / "samples.npz"), "--refs", str(tmp_path / "refs.npz"), "--device", "cpu"]
    out = distances.main(base + ["--out", str(tmp_path / "mmd.npz")])
    text = capsys.readouterr().out
    assert "2 molecules" in text and "heavy atoms" in text
    assert all(name in text for name in ("single_mean", "single_median", "all"))
    z = np.load(tmp_path / "mmd.npz")
    assert sorted(z.files) == sorted(out) and not any(k.endswith("_7") for k in z.files)
    for i, (at, ref, gen) in enumerate(_molecules(3)):
        res = distances.distance_mmd({"atom_type": at, "pos_ref": ref, "pos_gen": gen}, device="cpu")
        assert np.array_equal(z["single_%d" % i], res["single"]) and z["single_%d" % i].dtype == np.float32
        assert np.array_equal(z["pairs_%d" % i], res["pairs"]) and z["pairs_%d" % i].dtype == np.int32
        assert float(z["all_%d" % i]) == np.float32(res["all"]) and int(z["n_nan_columns_%d" % i]) == 0
        assert float(z["single_mean_%d" % i]) == res["single_mean"] and float(z["single_median_%d" % i]) == res["single_median"]
    rows = np.array([[float(z["single_mean_%d" % i]), float(z["single_median_%d" % i]), float(z["all_%d" % i])] for i in range(2)])
    for line, col in zip(text.strip().splitlines()[-3:], rows.T):
        mean, median = (float(v) for v in line.split()[1:3])
        assert mean == pytest.approx(col.mean(), abs=1e-6) and median == pytest.approx(np.median(col), abs=1e-6)
    with_h = distances.main(base + ["--with-h"])
    assert "all atoms" in capsys.readouterr().out and not (tmp_path / "mmd2.npz").exists()
    assert with_h["pairs_0"].shape[0] == 15 and out["pairs_0"].shape[0] == 6
    with pytest.raises(SystemExit):
        distances.main(["--samples", "x.npz"])


def test_tables_are_checked_before_any_launch():
    t = torch.zeros((2, 3), dtype=torch.float32)
    with pytest.raises(ValueError):
        distances.mmd_all(t, t)                       # (not on the GPU)
    with pytest.raises(ValueError):
        distances.mmd_single(t, t)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_exports_and_the_conformer_cap():
    sig = [VP, VP, I32, I32, I32, VP, VP, VP, VP]
    assert _lib.EXPORTS["agdiff_mmd_all"] == sig and _lib.EXPORTS["agdiff_mmd_single"] == sig
    assert _lib.DEFINES["AGDIFF_MMD_MAX_CONFS"] == 8192 == distances.MAX_CONFS
    lib = _lib.load()
    assert lib.agdiff_abi_version() == _lib.DEFINES["AGDIFF_ABI_VERSION"]
    for name in ("agdiff_mmd_all", "agdiff_mmd_single"):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == sig


def test_the_two_entry_points_check_their_arguments_on_the_host():
    lib = _lib.load()
    keep = (ctypes.c_uint64 * 8)()
    p, null = ctypes.c_void_p(ctypes.addressof(keep)), ctypes.c_void_p(0)
    for fn in (lib.agdiff_mmd_all, lib.agdiff_mmd_single):
        def call(**kw):
            a = dict(x=p, y=p, R=2, G=3, K=4, scratch=p, mmd2=p, bw=p)
            a.update(kw)
            return fn(a["x"], a["y"], a["R"], a["G"], a["K"], a["scratch"], a["mmd2"], a["bw"], null)
        for bad in (dict(x=null), dict(y=null), dict(scratch=null), dict(mmd2=null), dict(bw=null), dict(R=0), dict(G=0), dict(R=-1),
                    dict(K=0), dict(R=0, G=9000), dict(scratch=ctypes.c_void_p(ctypes.addressof(keep) + 4))):
            assert call(**bad) == -1, bad
    cap = _lib.DEFINES["AGDIFF_MMD_MAX_CONFS"]
    assert lib.agdiff_mmd_single(p, p, cap, 1, 1, p, p, p, null) == -2          # (M = cap + 1: refused before any launch)
    assert lib.agdiff_mmd_all(p, p, 2 ** 31 - 2, 1, 1, p, p, p, null) == -2
    assert lib.agdiff_mmd_all(p, p, 92672, 1, 1, p, p, p, null) == -2           # (5793 tile rows: 2^24 tiles or more)
    del keep
