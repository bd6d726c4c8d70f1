"""Plain-numpy float64 restatement of the distance-distribution MMD as include/agdiff_hip.h defines it (agdiff_mmd_all,
agdiff_mmd_single).  The bandwidth is the DIRECT double sum over pairs, not the closed form the kernels use; the kernel matrix is five
direct exponentials, not one and four squarings.  Test infrastructure only.

  GATE   |got - want| <= 1e-9 + 2^-23 |want|.  2^-23 is twice the half-ulp of the final fp32 store.  1e-9 covers fp64 reordering:
         kernel and reference sum the same M^2 terms <= 5, each with a few ulps of its own (the exponential's argument is good to
         a few 2^-53 relative and the argument is at most a few tens where the term matters), in different orders; the worst-case
         summation error 20 M^2 2^-53 is 3.6e-11 at M = 128 and the argument error of the exponentials stays below 6e-11 for
         K <= 512, in all < 1e-10: a factor of 10 of room.  Derived, not measured."""
import numpy as np

ATOL = 1e-9
RTOL = 2.0 ** -23


def within_gate(got, want):
    """every entry within the gate; NaNs in the same places"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    nan = np.isnan(want)
    if got.shape != want.shape or not np.array_equal(nan, np.isnan(got)):
        return False
    return bool((np.abs(got[~nan] - want[~nan]) <= ATOL + RTOL * np.abs(want[~nan])).all())


def worst(got, want):
    """the largest |got - want| / (ATOL + RTOL |want|) over the entries that are not NaN in the reference (<= 1 passes)"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    ok = ~np.isnan(want)
    return float((np.abs(got[ok] - want[ok]) / (ATOL + RTOL * np.abs(want[ok]))).max()) if ok.any() else 0.0


def _z(tab_x, tab_y):
    x = np.asarray(tab_x, dtype=np.float32).astype(np.float64)
    y = np.asarray(tab_y, dtype=np.float32).astype(np.float64)
    if x.ndim != 2 or y.ndim != 2 or x.shape[1] != y.shape[1] or x.shape[0] < 1 or y.shape[0] < 1:
        raise ValueError("tables must be [R >= 1, K] and [G >= 1, K]")
    return np.concatenate([x, y], axis=0), x.shape[0], y.shape[0]


def sq_dists(z):
    """D2 [M, M] = sum_k (Z[a][k] - Z[b][k])^2"""
    d = z[:, None, :] - z[None, :, :]
    return (d * d).sum(-1)


def bandwidth_direct(d2):
    m = d2.shape[0]
    return d2.sum() / (m * m - m)


def bandwidth_closed(z):
    """2 M sum_a |Z[a] - mu|^2 / (M^2 - M)"""
    m = z.shape[0]
    c = z - z.mean(0, keepdims=True)
    return 2.0 * m * (c * c).sum() / (m * m - m)


def _mmd2(z, R, G):
    """(mmd2, b) of one problem over the rows of z, float64"""
    with np.errstate(all="ignore"):
        if not np.isfinite(z).all():
            return np.nan, np.nan
        d2 = sq_dists(z)
        b = bandwidth_direct(d2)
        if b == 0.0:
            return 0.0, 0.0
        k = np.zeros_like(d2)
        for i in range(5):
            k += np.exp(-d2 / (b * 2.0 ** (i - 2)))
        return k[:R, :R].mean() + k[R:, R:].mean() - 2.0 * k[:R, R:].mean(), b


def mmd_all(tab_x, tab_y):
    """(mmd2, b) float64 scalars"""
    z, R, G = _z(tab_x, tab_y)
    return _mmd2(z, R, G)


def mmd_single(tab_x, tab_y):
    """(mmd2 float64 [K], b float64 [K]): column k alone"""
    z, R, G = _z(tab_x, tab_y)
    res = [_mmd2(z[:, k:k + 1], R, G) for k in range(z.shape[1])]
    return np.array([r[0] for r in res], dtype=np.float64), np.array([r[1] for r in res], dtype=np.float64)


CLOSED_K = 10.0 - 2.0 * (np.exp(-4.0) + np.exp(-2.0) + np.exp(-1.0) + np.exp(-0.5) + np.exp(-0.25))   # R = G = K = 1, x = 0, y = d


def tables(R, G, K, seed, scale_y=1.15):
    """fp32 tables of visibly different distributions: X ~ |N(2, 0.3)| per entry, Y the same law scaled by scale_y"""
    rng = np.random.default_rng(seed)
    x = np.abs(rng.normal(2.0, 0.3, size=(R, K))).astype(np.float32)
    y = (scale_y * np.abs(rng.normal(2.0, 0.3, size=(G, K)))).astype(np.float32)
    return x, y
