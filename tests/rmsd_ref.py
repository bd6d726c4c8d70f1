"""The RMSD recipe of the header of csrc/eval.hip (k_center_selected, ag_cov_add, ag_horn_key, ag_jacobi4, ag_pair_msd) restated in
float64 numpy, the interval a stored fp32 RMSD must lie in, the dynamic-LDS sizes of the matrix launchers, and the conformer sets
the tests of them share.  Test infrastructure only; anchored on the CPU in tests/test_rmsd_ref_cpu.py before
tests/test_hip_rmsd_kernels.py holds the kernels to it.

The kernels centre in fp64, round the centred coordinates to fp32 ONCE, and do everything after that in fp64 from those fp32
values.  So the comparison has two stages with nothing free in either:
  centring   every stored centred coordinate lies between the fp32 roundings of v - t and v + t (`centre`);
  pair       from the centred coordinates AS STORED the mean-square deviation is known to delta (`pair_msd`), and the stored RMSD
             lies between the fp32 roundings of the square roots of msd - delta and msd + delta (`in_gate`)."""
import math

import numpy as np

U = 2.0 ** -53                              # unit roundoff of fp64
OLD_BAR = 2e-5                              # the absolute bar of tests/test_hip_eval.py, test_hip_ensemble.py (Angstrom)
KINDS = ("noise", "identical", "moved", "unrelated", "planar", "collinear")

def GROUP6(m):
    """The abelian group of order six on the first five heavy atoms (in heavy-atom order), int32 [6, m]: c = the 3-cycle with
    c[0], c[1], c[2] = 1, 2, 0 and s = the swap of atoms 3 and 4, listed as (id, c, c c, s, c s, c c s).  A group, so that the self
    matrix's mirrored entries are the true [j][i] values; and c is NOT its own inverse, so that a kernel which applied a mapping to
    the wrong conformer, or applied its inverse, is told apart (the groups of tests/test_hip_ensemble.py hold involutions only)."""
    e = np.arange(m)
    c, s = e.copy(), e.copy()
    c[:3] = [1, 2, 0]
    s[3:5] = [4, 3]
    return np.stack([e, c, c[c], s, c[s], c[c][s]]).astype(np.int32)


ONE_WAY = (0, 1, 3, 4)                      # (id, c, s, c s) of GROUP6: holds c and c s WITHOUT their inverses -- see molecule

# sizes on either side of 48 KiB and of 64 KiB of dynamic LDS, and the limit (lds_bytes; tests/test_rmsd_ref_cpu.py checks the sides)
SHAPES = {"matrix": (127, 128, 170, 171, 256), "self": (122, 123, 164, 165, 256), "tfd": (383, 384, 511, 512)}


def lds_bytes(kernel, m_or_Q, T=0):
    """Dynamic LDS of one launch in bytes, as the launchers of csrc/eval.hip compute it: `matrix` (k_rmsd_matrix<false|true>: two
    tiles of 16 conformers of 3 m + 1 floats), `self` (k_rmsd_self: the same plus two [16][17] arrays), `tfd` (k_tfd_matrix: two
    tiles of 16 rows at the odd pitch Q | 1), `tfd_terms` (k_tfd_matrix_terms: the same behind T pairs of fp64)."""
    if kernel == "matrix":
        return 2 * 16 * (3 * m_or_Q + 1) * 4
    if kernel == "self":
        return (2 * 16 * (3 * m_or_Q + 1) + 2 * 16 * 17) * 4
    if kernel == "tfd":
        return 2 * 16 * (m_or_Q | 1) * 4
    if kernel == "tfd_terms":
        return 2 * 16 * (m_or_Q | 1) * 4 + 16 * T
    raise ValueError(kernel)


# ------------------------------------------------------------------------------------------------ the recipe
def _exact_sum(a, axis):
    """Sum of float64 values accumulated in the widest float numpy has (a 64-bit significand where long double is x87's): the
    products of two fp32 values are exact in fp64, so with it the reference's own summation error is 2^-11 of the kernels'."""
    return np.asarray(a, dtype=np.float64).sum(axis=axis, dtype=np.longdouble).astype(np.float64)


def centre(pos32, idx):
    """k_center_selected: (v, t) for conformers pos32 [C, n, 3] (or one, [n, 3]) and the selected atoms idx [m] -- v float64
    [C, m, 3] the selected coordinates minus their centroid BEFORE the rounding to fp32, t [C] = (m + 1) 2^-53 max |coordinate|
    the bound on what any order of summation can make of the centroid: m - 1 additions of at most m max|x| in all, each off by
    2^-53 relative, one division by m, one subtraction.  The kernel's stored value lies in [float32(v - t), float32(v + t)]."""
    p = np.asarray(pos32, dtype=np.float32).astype(np.float64)
    single = p.ndim == 2
    p = p.reshape(-1, p.shape[-2], 3)[:, np.asarray(idx, dtype=np.int64)]
    m = p.shape[1]
    with np.errstate(invalid="ignore"):
        c = _exact_sum(p, 1) / m
        v = p - c[:, None, :]
        t = (m + 1) * U * np.abs(p).max(axis=(1, 2))
    return (v[0], t[0]) if single else (v, t)


def horn_key(S):
    """ag_horn_key: Horn's symmetric 4x4 key matrix [..., 4, 4] of the cross-covariance S [..., 3, 3], S[a][b] = sum_k x_ka y_kb."""
    S = np.asarray(S, dtype=np.float64)
    Sxx, Sxy, Sxz = S[..., 0, 0], S[..., 0, 1], S[..., 0, 2]
    Syx, Syy, Syz = S[..., 1, 0], S[..., 1, 1], S[..., 1, 2]
    Szx, Szy, Szz = S[..., 2, 0], S[..., 2, 1], S[..., 2, 2]
    K = np.empty(S.shape[:-2] + (4, 4))
    K[..., 0, 0] = Sxx + Syy + Szz
    K[..., 0, 1] = K[..., 1, 0] = Syz - Szy
    K[..., 0, 2] = K[..., 2, 0] = Szx - Sxz
    K[..., 0, 3] = K[..., 3, 0] = Sxy - Syx
    K[..., 1, 1] = Sxx - Syy - Szz
    K[..., 1, 2] = K[..., 2, 1] = Sxy + Syx
    K[..., 1, 3] = K[..., 3, 1] = Szx + Sxz
    K[..., 2, 2] = -Sxx + Syy - Szz
    K[..., 2, 3] = K[..., 3, 2] = Syz + Szy
    K[..., 3, 3] = -Sxx - Syy + Szz
    return K


def jacobi4(K, sweeps=12):
    """ag_jacobi4<false>, statement for statement, on one symmetric 4x4 matrix: the diagonal left after at most `sweeps` cyclic
    Jacobi sweeps (ended early once the off-diagonal mass is below 1e-30), the eigenvalues in no particular order.  Used by the
    CPU tests only: it shows what the solver costs (test 2) and what a solver cut short would cost (test 3)."""
    A = [[float(K[r][c]) for c in range(4)] for r in range(4)]
    for _ in range(sweeps):
        off = 0.0
        for p in range(3):
            for q in range(p + 1, 4):
                off += A[p][q] * A[p][q]
        if off < 1e-30:
            break
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for r in range(4):                   # columns p, q
                    arp, arq = A[r][p], A[r][q]
                    A[r][p] = c * arp - s * arq
                    A[r][q] = s * arp + c * arq
                for r in range(4):                   # rows p, q
                    apr, aqr = A[p][r], A[q][r]
                    A[p][r] = c * apr - s * aqr
                    A[q][r] = s * apr + c * aqr
    return np.array([A[r][r] for r in range(4)])


def jacobi_eig(sweeps=None):
    """`eig` for pair_msd: jacobi4 with that many sweeps (None: its default) over a stack of matrices [..., 4, 4], sorted ascending
    like eigvalsh."""
    def eig(K):
        K = np.asarray(K)
        flat = K.reshape(-1, 4, 4)
        return np.stack([np.sort(jacobi4(k) if sweeps is None else jacobi4(k, sweeps)) for k in flat]).reshape(K.shape[:-1])
    return eig


def pair_msd(xc32, yc32, perms=None, eig=np.linalg.eigvalsh):
    """ag_pair_msd from centred FP32 coordinates: x = the probe (generated) conformer(s) [..., m, 3], y = the reference one(s)
    [..., m, 3] (leading axes broadcast), perms [P, m] or None (mapping p pairs atom k of x with atom perms[p][k] of y).  Returns
    (msd, msd_mirror, delta) in float64:
        gsum = |x|^2 + |y|^2,  S_p = sum_k x_k y_perm[p][k]^T,  K_p = horn_key(S_p),  lambda = eigvalsh(K_p)
        msd        = min_p (gsum - 2 lambda_max) / m          best proper rotation
        msd_mirror = min_p (gsum + 2 lambda_min) / m          the same for x inverted through its centroid (S -> -S)
        delta      = (4 m + 64) 2^-53 gsum / m
    Where delta comes from.  Every product of two fp32 values is exact in fp64, so all error is summation.  Recursive summation
    of m terms a_k, in ANY order, is off by at most m u sum |a_k| (u = 2^-53, first order).
      * An element of S is such a sum of x_ka y_kb, and |x y| <= (x^2 + y^2) / 2: |dS_ab| <= m u (|x_a|^2 + |y_b|^2) / 2, and the
        nine of them add up to 3 m u gsum / 2.
      * Every row of K holds each of the nine elements of S exactly once (three in the entry on the diagonal, two in each of the
        others), so the largest absolute row sum of dK, which bounds its 2-norm, is at most 3 m u gsum / 2; an eigenvalue of a
        symmetric matrix moves by at most the 2-norm of the perturbation (Weyl).  2 |d lambda| / m <= 3 m  units of u gsum / m.
      * gsum itself is a sum of 6 m squares accumulated atom by atom: m + 5 additions on the path of any term, m + 5 units.
      * The solver, the subtraction, the division and the rounding of S to fp64 here: 64 units cover them -- the twelve-sweep
        Jacobi is within 19 units of eigvalsh over the cases of this file, which tests/test_rmsd_ref_cpu.py asserts at 64.
    The sums here are accumulated in long double (_exact_sum), so delta is spent on the kernel alone."""
    x = np.asarray(xc32, dtype=np.float32).astype(np.float64)
    y = np.asarray(yc32, dtype=np.float32).astype(np.float64)
    m = x.shape[-2]
    assert y.shape[-2] == m and x.shape[-1] == 3 and y.shape[-1] == 3
    gsum = _exact_sum(x * x, (-2, -1)) + _exact_sum(y * y, (-2, -1))
    maps = [np.arange(m)] if perms is None else [np.asarray(p, dtype=np.int64) for p in perms]
    best = best_mirror = None
    with np.errstate(invalid="ignore"):
        for pm in maps:
            S = _exact_sum(x[..., :, :, None] * y[..., pm, None, :], -3)
            lam = eig(horn_key(S))
            a, b = (gsum - 2.0 * lam[..., -1]) / m, (gsum + 2.0 * lam[..., 0]) / m
            best = a if best is None else np.minimum(best, a)
            best_mirror = b if best_mirror is None else np.minimum(best_mirror, b)
    return best, best_mirror, (4 * m + 64) * U * gsum / m


def gate(msd, delta):
    """(lo, hi) as float32: the roundings of sqrt(max(msd - delta, 0)) and sqrt(msd + delta)."""
    msd, delta = np.asarray(msd, dtype=np.float64), np.asarray(delta, dtype=np.float64)
    return np.sqrt(np.maximum(msd - delta, 0.0)).astype(np.float32), np.sqrt(msd + delta).astype(np.float32)


def in_gate(got32, msd, delta):
    """True where float32(sqrt(max(msd - delta, 0))) <= got <= float32(sqrt(msd + delta)): an interval with no free tolerance.
    Rounding is monotone, so a kernel whose fp64 msd is within delta stores a value inside.  Above 1e-3 Angstrom the interval is
    the correctly rounded fp32 RMSD, or that and its neighbour when it straddles a rounding point; near zero it widens to about
    1e-6 Angstrom (sqrt(delta)), which is what the cancellation in gsum - 2 lambda allows."""
    got = np.asarray(got32)
    assert got.dtype == np.float32
    lo, hi = gate(msd, delta)
    return (lo <= got) & (got <= hi)


def gate_fraction(got32, msd, delta):
    """Information, not a gate: the largest |got^2 - msd| / delta over the entries whose interval holds more than one fp32 value on
    either side of got -- elsewhere the fp32 rounding of the stored value hides the kernel's msd.  None when there is no such entry."""
    got = np.asarray(got32, dtype=np.float32).astype(np.float64)
    msd, delta = np.broadcast_to(np.asarray(msd, dtype=np.float64), got.shape), np.broadcast_to(np.asarray(delta), got.shape)
    room = 4.0 * got * np.spacing(got.astype(np.float32)).astype(np.float64)        # what two fp32 steps of got are in msd
    ok = (delta > room) & np.isfinite(got)
    if not ok.any():
        return None
    return float((np.abs(got[ok] ** 2 - msd[ok]) / delta[ok]).max())


# ------------------------------------------------------------------------------------------------ the cases
def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def moved(rng, x):
    return x @ rotation(rng).T + rng.normal(size=3) * 5.0


def relabel(x, heavy, perm):
    """the same structure with heavy atom k sitting where heavy atom perm[k] sat"""
    y = x.copy()
    y[heavy] = x[heavy][perm]
    return y


def molecule(m, seed=0, R=5, G=18):
    """One molecule of exactly m heavy atoms with 0 to 2 hydrogens interleaved irregularly in front of each and 0 to 3 behind the
    last (the layout of tests/test_hip_trajectory.py::_case), and two conformer sets of it as fp32: ref [R, n, 3], gen [G, n, 3],
    from base * 1.5 + noise, every conformer then moved rigidly into a frame of its own, as the sampler leaves them (in a common
    frame Horn's matrix starts out nearly diagonal and the solver has nothing to do).  R >= 5, G >= 10.
    `pairs` names the (reference j, generated i) pairs of each kind:
        noise      ref j = base + 0.3 N, gen i = base + 0.5 N                     every pair not named below
        identical  gen 1 = ref 0 bit for bit                                      RMSD 0
        moved      gen 2 = ref 1 rigidly moved                                    ~0
        unrelated  gen 3 = another structure
        planar     ref 2 and gen 4 both in the plane z = 0                        rank-2 S
        collinear  ref 3 on the x axis, gen 5 on the y axis at another spacing    rank-1 S
        twin       gen 6 = ref 4 relabelled by c, moved                           ~0 under the mapping c alone
        mirror     gen 7 = ref 4 relabelled by c s, inverted, moved               mirror RMSD ~0 under the mapping c s alone
    and `self_twin` = (0, 9): gen 9 = gen 0 relabelled by c c, moved: with x = conformer 0 it matches under c alone.
    perms = GROUP6(m), what a self matrix needs; maps = perms[ONE_WAY], the set for a reference x generated matrix: it holds c and
    c s but not their inverses c c and c c s, so the twins are found only by a kernel that pairs atom k of the GENERATED conformer
    with atom perms[p][k] of the REFERENCE, as include/agdiff_hip.h says.  Both None for m < 5 (no twins then: gen 6, 7 and 9 stay
    noise).  Read-only arrays."""
    assert R >= 5 and G >= 10
    rng = np.random.default_rng(100 * m + seed)
    ty = []
    for _ in range(m):
        ty.extend([1] * int(rng.integers(0, 3)))
        ty.append(int(rng.choice([6, 7, 8])))
    ty.extend([1] * int(rng.integers(0, 4)))
    atom_type = np.asarray(ty, dtype=np.int64)
    heavy = np.nonzero(atom_type != 1)[0].astype(np.int32)
    n = atom_type.shape[0]
    assert heavy.shape[0] == m
    perms = GROUP6(m) if m >= 5 else None
    maps = perms[list(ONE_WAY)] if perms is not None else None
    base = rng.normal(size=(n, 3)) * 1.5
    ref = np.stack([moved(rng, base + 0.3 * rng.normal(size=(n, 3))) for _ in range(R)])
    gen = np.stack([moved(rng, base + 0.5 * rng.normal(size=(n, 3))) for _ in range(G)])
    ref[2, :, 2] = 0.0
    ref[3] = 0.0
    ref[3, :, 0] = 0.5 * np.arange(n)
    ref = ref.astype(np.float32)                   # (the copies below are taken from the fp32 references)
    ref64 = ref.astype(np.float64)
    gen[1] = ref64[0]
    gen[2] = moved(rng, ref64[1])
    gen[3] = rng.normal(size=(n, 3)) * 1.5
    gen[4] = ref64[2] + 0.2 * rng.normal(size=(n, 3))
    gen[4, :, 2] = 0.0
    gen[5] = 0.0
    gen[5, :, 1] = 0.55 * np.arange(n)
    pairs = {"identical": [(0, 1)], "moved": [(1, 2)], "unrelated": [(j, 3) for j in range(R)], "planar": [(2, 4)], "collinear": [(3, 5)]}
    if perms is not None:
        gen[6] = moved(rng, relabel(ref64[4], heavy, perms[1]))
        c = ref64[4][heavy].mean(0)
        gen[7] = moved(rng, relabel(2.0 * c - ref64[4], heavy, perms[4]))
        pairs["twin"], pairs["mirror"] = [(4, 6)], [(4, 7)]
    gen = gen.astype(np.float32)
    if perms is not None:
        gen[9] = moved(rng, relabel(gen[0].astype(np.float64), heavy, perms[2])).astype(np.float32)
    named = {p for v in pairs.values() for p in v}
    special = set(range(1, 8)) | {9}
    pairs["noise"] = [(j, i) for j in (0, 1, 4) for i in range(G) if i not in special and (j, i) not in named]
    out = dict(m=m, n=n, R=R, G=G, atom_type=atom_type, heavy=heavy, perms=perms, maps=maps, ref=ref, gen=gen, pairs=pairs,
               self_twin=(0, 9) if perms is not None else None)
    for k in ("atom_type", "heavy", "perms", "maps", "ref", "gen"):
        if out[k] is not None:
            out[k].setflags(write=False)
    return out


def kinds_of(mol):
    """(kind, j, i) for every named pair of `mol`: all the special pairs and the noise pairs"""
    return [(kind, j, i) for kind, lst in mol["pairs"].items() for j, i in lst]


def stored_centres(pos32, idx):
    """The centred coordinates as fp32 [C, m, 3]: `centre` rounded once, what the kernel stores up to the bound t."""
    v, _ = centre(pos32, idx)
    return v.astype(np.float32)
