"""GPU (MI355X): the RMSD family of csrc/eval.hip -- k_center_selected, k_rmsd_matrix<false|true>, k_rmsd_self, k_matrix_minima,
k_align_conformers -- and the TFD matrices k_tfd_matrix / k_tfd_matrix_terms, at their size limits and on both launch paths (at
most 48 KiB of dynamic LDS, and past it through hipFuncSetAttribute; past 64 KiB HIP refuses the launch without the attribute),
against the float64 restatement tests/rmsd_ref.py (anchored on the CPU in tests/test_rmsd_ref_cpu.py).

Gates (none is a measured figure):
  centred coordinates   [float32(v - t), float32(v + t)], t = (m + 1) 2^-53 max|coordinate|                       rmsd_ref.centre
  RMSD entries          [float32(sqrt(max(msd - d, 0))), float32(sqrt(msd + d))], d = (4 m + 64) 2^-53 gsum / m,
                        msd from the kernel's OWN centred coordinates (read back from `scratch`)                   rmsd_ref.in_gate
  self vs full matrix   bit for bit (the claim of the header of csrc/eval.hip); minima bit for bit against torch.min
  aligned coordinates   one fp32 ulp of the float64 SVD Kabsch value: one fp32 store of an fp64 value
  TFD                   2e-7, the TFD_ATOL of tests/test_hip_torsions.py and tests/test_hip_rings.py
The reference x generated matrices run over a mapping set that holds a 3-cycle without its inverse (rmsd_ref.molecule), so the
planted twins are found only if atom k of the generated conformer is paired with atom perms[p][k] of the reference; the self matrix
takes the whole group.

Largest observed fraction of each gate on the MI355X (information: `pytest -s` prints them):
  k_center_selected     every stored coordinate of every shape was float32(v) itself: none at the interval's other value
  k_rmsd_matrix<false>  0.015 of delta (m = 256), where the stored value lets the kernel's msd be inferred: the entries near zero
  k_rmsd_matrix<true>   0.015 of delta for `out` (bit for bit the other instantiation's), 0.009 for `out_mirror` (m = 170)
  k_rmsd_self           0.016 of delta (m = 164); bit for bit k_rmsd_matrix(pos, pos) transposed, at every shape
  k_matrix_minima       bit for bit (no gate to take a fraction of)
  k_align_conformers    0.500 ulp at all four shapes: the stored value is the float64 reference correctly rounded
  k_tfd_matrix          2.98e-8 = 0.149 of TFD_ATOL at every Q;  k_tfd_matrix_terms  2.98e-8 = 0.149 at Q = T = 512
No launcher returned anything but AGDIFF_OK on either path, and a non-finite conformer behaved as include/agdiff_hip.h now says."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rings_ref as RR
import rmsd_ref as RM
import tfd_ref as TR

pytestmark = pytest.mark.gpu

AGDIFF_OK = 0
TFD_ATOL = 2e-7
MATRIX_M, SELF_M = RM.SHAPES["matrix"], RM.SHAPES["self"]
LIMIT = 256


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                       # (a writable copy: the cached cases are read-only)


def _bits(x):
    """int32 view of a float32 array: equality of these is equality bit for bit"""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _mol(m, G=None):
    """(R, G) = (5, 18), at the limit (17, 33); G given: the conformer set of a self matrix"""
    if G is not None:
        return RM.molecule(m, R=5, G=G)
    return RM.molecule(m, R=17, G=33) if m == LIMIT else RM.molecule(m)


def _rmsd_matrix(ref, gen, heavy, perms, hands):
    """One call of agdiff_rmsd_matrix (hands: agdiff_rmsd_matrix_hands) through _lib with the test's own scratch:
    (rc, out [R, G], mirror or None, centred ref [R, 3 m + 1], centred gen [G, 3 m + 1]) on the host; every output pre-filled with NaN."""
    from agdiff_amd import _lib
    lib = _lib.load()
    R, G, n, m = ref.shape[0], gen.shape[0], ref.shape[1], int(heavy.shape[0])
    ref_d, gen_d, idx_d = _dev(ref), _dev(gen), _dev(heavy)
    pm_d = None if perms is None else _dev(perms)
    P = 0 if perms is None else perms.shape[0]
    scratch = torch.full(((R + G) * (3 * m + 1),), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.full((R, G), float("nan"), dtype=torch.float32, device="cuda")
    mirror = torch.full((R, G), float("nan"), dtype=torch.float32, device="cuda") if hands else None
    common = (_lib.ptr(ref_d), _lib.ptr(gen_d), _lib.ptr(idx_d), _lib.ptr(pm_d), R, G, n, m, P, _lib.ptr(scratch), _lib.ptr(out))
    if hands:
        rc = lib.agdiff_rmsd_matrix_hands(*common, _lib.ptr(mirror), _lib.stream_ptr())
    else:
        rc = lib.agdiff_rmsd_matrix(*common, _lib.stream_ptr())
    torch.cuda.synchronize()
    c = scratch.cpu().numpy().reshape(R + G, 3 * m + 1)
    return rc, out.cpu().numpy(), None if mirror is None else mirror.cpu().numpy(), c[:R], c[R:]


def _rmsd_self(gen, heavy, perms, thresh, want_out=True, want_bits=True):
    """One call of agdiff_rmsd_self through _lib: (rc, out [G, G] or None, adjacency bool [G, 8 pitch] or None, centred [G, 3 m + 1])"""
    from agdiff_amd import _lib
    from agdiff_amd.ensemble import bits_pitch, unpack_bits
    lib = _lib.load()
    G, n, m = gen.shape[0], gen.shape[1], int(heavy.shape[0])
    gen_d, idx_d = _dev(gen), _dev(heavy)
    pm_d = None if perms is None else _dev(perms)
    P = 0 if perms is None else perms.shape[0]
    scratch = torch.full((G * (3 * m + 1),), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.full((G, G), float("nan"), dtype=torch.float32, device="cuda") if want_out else None
    bits = torch.full((G, bits_pitch(G) // 8), -1, dtype=torch.int64, device="cuda") if want_bits else None
    rc = lib.agdiff_rmsd_self(_lib.ptr(gen_d), _lib.ptr(idx_d), _lib.ptr(pm_d), G, n, m, P, ctypes.c_float(thresh), _lib.ptr(scratch),
                              _lib.ptr(out), _lib.ptr(bits), _lib.stream_ptr())
    torch.cuda.synchronize()
    adj = None if bits is None else unpack_bits(bits, G).cpu().numpy()
    return rc, None if out is None else out.cpu().numpy(), adj, scratch.cpu().numpy().reshape(G, 3 * m + 1)


def _xyz(c):
    """[C, 3 m + 1] rows of scratch -> centred coordinates [C, m, 3]"""
    return c[:, :-1].reshape(c.shape[0], -1, 3)


@functools.lru_cache(maxsize=None)
def _matrix_run(m, with_perms):
    """Both entry points on the molecule of m heavy atoms, and the float64 reference of the kernel's own centred coordinates --
    computed once, shared by the tests below, never modified"""
    mol = _mol(m)
    perms = mol["maps"] if with_perms else None            # (c and c s without their inverses: rmsd_ref.molecule)
    rc, out, _, cref, cgen = _rmsd_matrix(mol["ref"], mol["gen"], mol["heavy"], perms, hands=False)
    rc_h, out_h, mirror, cref_h, cgen_h = _rmsd_matrix(mol["ref"], mol["gen"], mol["heavy"], perms, hands=True)
    msd, msd_mirror, delta = RM.pair_msd(_xyz(cgen)[None, :], _xyz(cref)[:, None], perms)
    return dict(mol=mol, rc=rc, rc_hands=rc_h, out=out, out_hands=out_h, mirror=mirror, cref=cref, cgen=cgen,
                same_scratch=np.array_equal(_bits(cref), _bits(cref_h)) and np.array_equal(_bits(cgen), _bits(cgen_h)),
                msd=msd, msd_mirror=msd_mirror, delta=delta)


def _fraction(name, got, msd, delta):
    f = RM.gate_fraction(got, msd, delta)
    print("%s: largest inferable |msd_kernel - msd_ref| / delta = %s" % (name, "none inferable" if f is None else "%.3f" % f))


# ------------------------------------------------------------------------------------------------ 1. centring
@pytest.mark.parametrize("m", sorted(set(MATRIX_M + SELF_M)))
def test_centred_coordinates_are_the_float64_values_rounded_once(m):
    mol = _mol(m)
    if m in MATRIX_M:
        run = _matrix_run(m, True)
        rc, rows, pos = run["rc"], np.concatenate([run["cref"], run["cgen"]]), np.concatenate([mol["ref"], mol["gen"]])
    else:
        rc, _, _, rows = _rmsd_self(mol["gen"], mol["heavy"], mol["perms"], 0.5)
        pos = mol["gen"]
    assert rc == AGDIFF_OK
    v, t = RM.centre(pos, mol["heavy"])
    lo, hi = (v - t[:, None, None]).astype(np.float32), (v + t[:, None, None]).astype(np.float32)
    got = _xyz(rows)
    assert got.shape == v.shape and ((lo <= got) & (got <= hi)).all()
    assert not rows[:, -1].any() and not np.signbit(rows[:, -1]).any()           # the pad float of each conformer is +0
    exact = got == v.astype(np.float32)
    print("centring m = %d: %d conformers, %.4f %% of the coordinates are float32(v) itself, the others its neighbour inside the interval"
          % (m, pos.shape[0], 100.0 * exact.mean()))


# ------------------------------------------------------------------------------------------------ 2. the matrix, both instantiations
@pytest.mark.parametrize("with_perms", [True, False])
@pytest.mark.parametrize("m", MATRIX_M)
def test_matrix_entries_lie_in_the_derived_interval(m, with_perms):
    run = _matrix_run(m, with_perms)
    mol = run["mol"]
    assert run["rc"] == AGDIFF_OK and run["rc_hands"] == AGDIFF_OK               # (also on the first launch past 48 KiB of the process)
    assert RM.lds_bytes("matrix", m) > 48 * 1024 or m == 127
    assert run["same_scratch"] and np.array_equal(_bits(run["out"]), _bits(run["out_hands"]))
    assert np.isfinite(run["out"]).all() and np.isfinite(run["mirror"]).all()
    ok = RM.in_gate(run["out"], run["msd"], run["delta"])
    ok_m = RM.in_gate(run["mirror"], run["msd_mirror"], run["delta"])
    _fraction("k_rmsd_matrix m = %d perms %s proper" % (m, with_perms), run["out"], run["msd"], run["delta"])
    _fraction("k_rmsd_matrix m = %d perms %s mirror" % (m, with_perms), run["mirror"], run["msd_mirror"], run["delta"])
    assert ok.all(), np.argwhere(~ok)[:5]
    assert ok_m.all(), np.argwhere(~ok_m)[:5]
    # the planted pairs are what they were planted as
    out, mirror, pairs = run["out"], run["mirror"], mol["pairs"]
    assert out[pairs["identical"][0]] < 2e-6 and out[pairs["moved"][0]] < 5e-6 and out[pairs["unrelated"][0]] > 1.0
    if with_perms:                                         # found only if atom k of the GENERATED conformer goes with perms[p][k] of the reference
        assert out[pairs["twin"][0]] < 5e-6 and mirror[pairs["mirror"][0]] < 5e-6 and out[pairs["mirror"][0]] > 1e-2
    else:
        assert out[pairs["twin"][0]] > 1e-2 and mirror[pairs["mirror"][0]] > 1e-2


def test_the_wrappers_at_the_limit_are_the_entry_points_bit_for_bit():
    from agdiff_amd.ensemble import self_rmsd_matrix, threshold_bits
    from agdiff_amd.evaluation import get_rmsd_confusion_matrix
    run = _matrix_run(LIMIT, True)
    mol = run["mol"]
    assert mol["m"] == LIMIT and (mol["R"], mol["G"]) == (17, 33)
    item = {"atom_type": mol["atom_type"].copy(), "pos_ref": mol["ref"].reshape(-1, 3).copy(), "pos_gen": mol["gen"].reshape(-1, 3).copy(),
            "perms": mol["maps"].copy()}                                          # (writable copies: the cached case is read-only)
    proper, mirror = get_rmsd_confusion_matrix(item, hands=True)
    item["perms"] = mol["perms"].copy()                                          # the self matrix takes the whole group
    assert np.array_equal(_bits(proper.cpu().numpy()), _bits(run["out"])) and np.array_equal(_bits(mirror.cpu().numpy()), _bits(run["mirror"]))
    rc, out, adj, _ = _rmsd_self(mol["gen"], mol["heavy"], mol["perms"], 0.5)
    assert rc == AGDIFF_OK
    assert np.array_equal(_bits(self_rmsd_matrix(item).cpu().numpy()), _bits(out))
    w_out, w_adj = threshold_bits(item, 0.5)
    assert np.array_equal(_bits(w_out.cpu().numpy()), _bits(out)) and np.array_equal(w_adj.cpu().numpy(), adj)


# ------------------------------------------------------------------------------------------------ 3. the self matrix
@pytest.mark.parametrize("G", [17, 37])
@pytest.mark.parametrize("m", SELF_M)
def test_self_matrix_entries_bits_and_the_full_matrix_bit_for_bit(m, G):
    """G = 17: a diagonal tile, a ragged diagonal tile and the ragged off-diagonal tile between them; G = 37: six tiles, three of
    them off the diagonal, the last column of tiles ragged"""
    from agdiff_amd.ensemble import bits_pitch
    mol = _mol(m, 37)
    gen, heavy, perms = mol["gen"][:G], mol["heavy"], mol["perms"]
    assert RM.lds_bytes("self", m) > 48 * 1024 or m == 122
    outs, adjs = [], []
    for thr in (0.0, 1.2, 1e9):
        rc, out, adj, cen = _rmsd_self(gen, heavy, perms, thr)
        assert rc == AGDIFF_OK
        assert adj.shape == (G, 8 * bits_pitch(G))
        assert np.array_equal(adj[:, :G], out <= np.float32(thr)) and not adj[:, G:].any() and adj[:, :G].diagonal().all()
        outs.append(out)
        adjs.append(adj)
    out = outs[0]
    assert all(np.array_equal(_bits(o), _bits(out)) for o in outs)
    assert len({int(a.sum()) for a in adjs}) == 3                                # the thresholds cut differently: the diagonal, a mix, all
    rc, no_out, adj_only, _ = _rmsd_self(gen, heavy, perms, 1.2, want_out=False)   # each output alone is the same output
    assert rc == AGDIFF_OK and no_out is None and np.array_equal(adj_only, adjs[1])
    rc, out_only, no_adj, _ = _rmsd_self(gen, heavy, perms, 1.2, want_bits=False)
    assert rc == AGDIFF_OK and no_adj is None and np.array_equal(_bits(out_only), _bits(out))
    assert np.array_equal(_bits(out), _bits(out.T)) and not _bits(out).diagonal().any()      # exactly symmetric, diagonal +0
    c = _xyz(cen)
    msd, _, delta = RM.pair_msd(c[:, None], c[None, :], perms)                   # [i][j]: x = conformer i, y = conformer j
    iu = np.triu_indices(G, 1)
    ok = RM.in_gate(out[iu], msd[iu], delta[iu])
    _fraction("k_rmsd_self m = %d G = %d" % (m, G), out[iu], msd[iu], delta[iu])
    assert ok.all(), [(iu[0][k], iu[1][k]) for k in np.nonzero(~ok)[0][:5]]
    a, b = mol["self_twin"]
    assert out[a, b] < 5e-6
    # csrc/eval.hip, header: k_rmsd_self and k_rmsd_matrix "agree bit for bit because they call that one routine".  The self kernel
    # computes (i, j), i < j, with x = conformer i; the matrix kernel's x is the GENERATED conformer, its column: entry [j][i]
    rc, full, _, _, _ = _rmsd_matrix(gen, gen, heavy, perms, hands=False)
    assert rc == AGDIFF_OK
    assert np.array_equal(_bits(out[iu]), _bits(full.T[iu]))


# ------------------------------------------------------------------------------------------------ 4. minima
@pytest.mark.parametrize("G", [1, 64, 65, 130])
@pytest.mark.parametrize("R", [1, 64, 65, 130])
def test_minima_are_torch_min_bit_for_bit_past_one_stride(R, G):
    from agdiff_amd.evaluation import matrix_minima
    rng = np.random.default_rng(1000 * R + G)
    mat = rng.uniform(0.01, 3.0, size=(R, G)).astype(np.float32)
    mat[rng.random((R, G)) < 0.1] = np.inf
    mat[R // 2, :] = np.inf                                                      # a row with nothing finite
    mat[:, 0] = np.inf                                                           # and such a column
    r2, c2 = R - 1, G - 1
    if R > 64 and G > 64:                                                        # minima that only the second trip of the stride sees
        mat[r2, :64], mat[:64, c2] = np.inf, np.inf
        mat[r2, 64:], mat[64:, c2] = np.maximum(mat[r2, 64:], 2.0), np.maximum(mat[64:, c2], 2.0)
        mat[r2, c2] = np.float32(0.001)
    d = _dev(mat)
    rmin, gmin = matrix_minima(d)
    assert np.array_equal(_bits(rmin.cpu().numpy()), _bits(d.min(dim=1).values.cpu().numpy()))
    assert np.array_equal(_bits(gmin.cpu().numpy()), _bits(d.min(dim=0).values.cpu().numpy()))
    assert np.array_equal(rmin.cpu().numpy(), mat.min(1)) and np.array_equal(gmin.cpu().numpy(), mat.min(0))
    assert np.isinf(rmin[R // 2].item()) and np.isinf(gmin[0].item())
    assert not (R > 64 and G > 64) or (rmin[r2].item() == gmin[c2].item() == np.float32(0.001))


# ------------------------------------------------------------------------------------------------ 5. non-finite input
def test_a_non_finite_conformer_is_plus_infinity_in_its_row_or_column_and_nothing_else_changes():
    """include/agdiff_hip.h: a conformer with a non-finite SELECTED coordinate is +inf away from everything, in both matrices (and
    keeps its zero diagonal in the self matrix); every other entry keeps its bits; unselected atoms are never read."""
    m = 128
    run = _matrix_run(m, True)
    mol = run["mol"]
    heavy, perms, maps, R, G = mol["heavy"], mol["perms"], mol["maps"], mol["R"], mol["G"]
    ref, gen = mol["ref"].copy(), mol["gen"].copy()
    ref[1, heavy[3], 1] = np.nan
    gen[4, heavy[70], 0] = np.inf                                                # past atom 64 of the selection
    gen[11, heavy[100], 2] = -np.inf
    hit = np.zeros((R, G), dtype=bool)
    hit[1, :] = hit[:, 4] = hit[:, 11] = True
    rc, out, mirror, _, _ = _rmsd_matrix(ref, gen, heavy, maps, hands=True)
    assert rc == AGDIFF_OK
    rc, plain, _, _, _ = _rmsd_matrix(ref, gen, heavy, maps, hands=False)
    assert rc == AGDIFF_OK and np.array_equal(_bits(plain), _bits(out))
    for got, clean in ((out, run["out"]), (mirror, run["mirror"])):
        assert (got[hit] == np.inf).all()
        assert np.array_equal(_bits(got[~hit]), _bits(clean[~hit]))
    # the self matrix: conformers 2 (NaN), 4 (+inf), 11 (-inf) of the generated set
    thr = 1.2
    rc, clean, clean_adj, _ = _rmsd_self(mol["gen"], heavy, perms, thr)
    assert rc == AGDIFF_OK
    gen[2, heavy[3], 1] = np.nan
    rc, got, adj, _ = _rmsd_self(gen, heavy, perms, thr)
    assert rc == AGDIFF_OK
    bad = np.zeros(G, dtype=bool)
    bad[[2, 4, 11]] = True
    cross = (bad[:, None] | bad[None, :]) & ~np.eye(G, dtype=bool)
    assert (got[cross] == np.inf).all() and not _bits(got).diagonal().any()
    assert np.array_equal(_bits(got[~cross]), _bits(clean[~cross]))
    assert not adj[:, :G][cross].any() and adj[:, :G].diagonal().all() and not adj[:, G:].any()
    assert np.array_equal(adj[:, :G][~cross], clean_adj[:, :G][~cross])
    rc, _, adj_inf, _ = _rmsd_self(gen, heavy, perms, float("inf"))            # the bits follow out <= thresh: +inf <= +inf
    assert rc == AGDIFF_OK and adj_inf[:, :G].all() and not adj_inf[:, G:].any()
    # a NaN in an unselected atom changes no bit
    hyd = np.nonzero(mol["atom_type"] == 1)[0]
    assert hyd.size > 10
    ref, gen = mol["ref"].copy(), mol["gen"].copy()
    ref[0, hyd[0]] = np.nan
    gen[:, hyd[5], 2] = np.nan
    gen[3, hyd[-1]] = np.inf
    rc, out, mirror, cref, cgen = _rmsd_matrix(ref, gen, heavy, maps, hands=True)
    assert rc == AGDIFF_OK
    assert np.array_equal(_bits(out), _bits(run["out"])) and np.array_equal(_bits(mirror), _bits(run["mirror"]))
    assert np.array_equal(_bits(cref), _bits(run["cref"])) and np.array_equal(_bits(cgen), _bits(run["cgen"]))
    rc, got, adj, _ = _rmsd_self(gen, heavy, perms, thr)
    assert rc == AGDIFF_OK and np.array_equal(_bits(got), _bits(clean)) and np.array_equal(adj, clean_adj)


# ------------------------------------------------------------------------------------------------ 6. alignment past one stride
@pytest.mark.parametrize("n,m", [(64, 64), (65, 65), (130, 70), (300, 256)])
def test_alignment_past_one_stride_is_the_float64_kabsch_to_one_ulp(n, m):
    """(64, 64): every loop makes exactly one full trip; (65, 65): one atom in the second; (130, 70): the selection loops make two
    trips and the loop over all atoms three; (300, 256): four and five."""
    from agdiff_amd.ensemble import align_conformers
    from test_hip_ensemble import _direct_rmsd, _kabsch_align, _pair_distances
    rng = np.random.default_rng(1000 * n + m)
    at = np.ones(n, dtype=np.int64)
    heavy = np.sort(rng.permutation(n)[:m])
    at[heavy] = rng.choice([6, 7, 8], size=m)
    G = 6
    target = (rng.normal(size=(n, 3)) * 1.5).astype(np.float32)
    pos = np.stack([RM.moved(rng, target + 0.3 * rng.normal(size=(n, 3))) for _ in range(G)]).astype(np.float32)
    top = max(np.abs(pos).max(), np.abs(target).max())
    assert top < 32.0
    got_d, rmsd_d = align_conformers(pos, at, target)
    got, rmsd = got_d.cpu().numpy(), rmsd_d.cpu().numpy()
    assert got.shape == (G, n, 3) and rmsd.shape == (G,) and got.dtype == rmsd.dtype == np.float32
    want = np.stack([_kabsch_align(p, target, heavy) for p in pos])
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    frac = np.abs(got.astype(np.float64) - want) / ulp
    print("alignment n = %d m = %d: largest |aligned - float64 Kabsch| = %.3e Angstrom = %.3f ulp of the element"
          % (n, m, np.abs(got - want).max(), frac.max()))
    assert (frac <= 1.0).all()
    for g in range(G):
        direct = _direct_rmsd(got[g], target, heavy)
        assert abs(float(rmsd[g]) - direct) <= np.spacing(np.float32(direct)), (g, rmsd[g], direct)
        assert np.abs(_pair_distances(got[g]) - _pair_distances(pos[g])).max() <= 4.0 * 2.0 ** -24 * top * np.sqrt(3.0)
    # a NaN in a selected atom of one conformer leaves the others bit for bit what they were
    broken = pos.copy()
    broken[2, heavy[m - 1], 1] = np.nan
    got2, rmsd2 = (x.cpu().numpy() for x in align_conformers(broken, at, target))
    keep = np.arange(G) != 2
    assert np.array_equal(_bits(got2[keep]), _bits(got[keep])) and np.array_equal(_bits(rmsd2[keep]), _bits(rmsd[keep]))
    assert not np.isfinite(rmsd2[2])


# ------------------------------------------------------------------------------------------------ 7. TFD at the limit
@functools.lru_cache(maxsize=None)
def _tfd_case(Q, P):
    """(x [17, Q], y [33, Q] fp32 uniform in (-pi, pi], tmap [P, Q] with row 0 a permutation of the columns, weights [Q]); T = Q"""
    rng = np.random.default_rng(10 * Q + P)
    x = (-rng.uniform(-np.pi, np.pi, size=(17, Q))).astype(np.float32)           # uniform on [-pi, pi), negated: (-pi, pi]
    y = (-rng.uniform(-np.pi, np.pi, size=(33, Q))).astype(np.float32)
    tmap = rng.integers(0, Q, size=(P, Q)).astype(np.int32)
    tmap[0] = rng.permutation(Q)
    w = rng.uniform(0.2, 3.0, size=Q).astype(np.float32)
    for a in (x, y, tmap, w):
        a.setflags(write=False)
    return x, y, tmap, w


@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("Q", RM.SHAPES["tfd"])
def test_tfd_matrix_on_both_sides_of_48_kib_and_at_the_column_limit(Q, P):
    from agdiff_amd.ensemble import unpack_bits
    from agdiff_amd.torsions import tfd_from_angles
    x, y, tmap, w = _tfd_case(Q, P)
    tmap, w = tmap.copy(), w.copy()                                              # (writable copies: the cached case is read-only)
    assert (RM.lds_bytes("tfd", Q) > 48 * 1024) == (Q >= 384) and (RM.lds_bytes("tfd", Q) > 64 * 1024) == (Q == 512)
    xd, yd = _dev(x), _dev(y)
    worst = 0.0
    for weights in (None, w):
        out, mirror, bits = tfd_from_angles(xd, yd, tmap, weights=weights, want_mirror=True, threshold=0.5)     # (raises unless AGDIFF_OK)
        for got, want in ((out, TR.tfd(x, y, tmap, weights)), (mirror, TR.tfd(x, y, tmap, weights, mirror=True))):
            g = got.cpu().numpy()
            assert g.dtype == np.float32 and g.shape == (17, 33) and (g > 0).all() and (g <= 1).all()
            err = np.abs(g.astype(np.float64) - want).max()
            worst = max(worst, err)
            assert err <= TFD_ATOL, (weights is not None, err)
        adj = unpack_bits(bits, 17)
        assert torch.equal(adj[:, :33], out <= 0.5) and not adj[:, 33:].any()
    print("k_tfd_matrix Q = T = %d P = %d: largest difference to the reference %.3e = %.3f of the gate" % (Q, P, worst, worst / TFD_ATOL))


@pytest.mark.parametrize("P", [1, 4])
def test_tfd_with_terms_at_the_column_limit(P):
    """Q = T = 512: 73,856 bytes of dynamic LDS, the most any launch of csrc/eval.hip's matrix kernels asks for besides the RMSD ones;
    the reference and the gate of tests/test_hip_rings.py::test_tfd_with_terms_matches_the_float64_reference"""
    from agdiff_amd.ensemble import unpack_bits
    from agdiff_amd.torsions import tfd_from_angles
    Q = 512
    assert RM.lds_bytes("tfd_terms", Q, Q) == 73856
    x, y, tmap, w = _tfd_case(Q, P)
    tmap, w = tmap.copy(), w.copy()                                              # (writable copies: the cached case is read-only)
    rng = np.random.default_rng(P)
    even = rng.integers(0, 2, size=Q).astype(np.int32)
    even[0], even[-1] = 0, 1
    scale = np.where(even != 0, [RR.ring_scale(N) for N in rng.integers(4, 13, size=Q)], np.pi).astype(np.float32)
    x, y = x.copy(), y.copy()
    ringcol = np.zeros(Q, dtype=bool)
    ringcol[tmap[0][even != 0]] = True                                           # ring-like values in [0, pi / 2] where an even term reads
    x[:, ringcol], y[:, ringcol] = np.abs(x[:, ringcol]) * 0.5, np.abs(y[:, ringcol]) * 0.5
    xd, yd = _dev(x), _dev(y)
    worst = 0.0
    for weights in (None, w):
        out, mirror, bits = tfd_from_angles(xd, yd, tmap, weights=weights, want_mirror=True, threshold=0.5, rings=(scale, even))
        for got, want in ((out, RR.tfd_terms(x, y, tmap, scale, even, weights)),
                          (mirror, RR.tfd_terms(x, y, tmap, scale, even, weights, mirror=True))):
            g = got.cpu().numpy()
            assert g.dtype == np.float32 and g.shape == (17, 33) and (g > 0).all() and (g <= 1).all()
            err = np.abs(g.astype(np.float64) - want).max()
            worst = max(worst, err)
            assert err <= TFD_ATOL, (weights is not None, err)
        adj = unpack_bits(bits, 17)
        assert torch.equal(adj[:, :33], out <= 0.5) and not adj[:, 33:].any()
    print("k_tfd_matrix_terms Q = T = 512 P = %d: largest difference to the reference %.3e = %.3f of the gate" % (P, worst, worst / TFD_ATOL))
