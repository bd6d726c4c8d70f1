"""GPU (MI355X): ring conformations (agdiff_amd.rings, the ring terms of agdiff_amd.torsions; csrc/eval.hip: k_ring_coords,
k_tfd_matrix_terms) against the float64 numpy restatement of their definitions (tests/rings_ref.py), against the rings the
restatement's inverse constructs, and through prune, clustering and the command lines.

Gates, none taken from what the kernels give:
  ANGLE_ATOL 1e-6 rad  tau and the phases: kernel and reference both compute in fp64 from the same fp32 coordinates, so the difference
                       is the fp32 store; half an ulp at <= 2 pi is 2.4e-7, with a margin of 4
  AMP_ATOL   1e-6 A    the amplitudes, likewise: half an ulp below 4 Angstrom is 2.4e-7
  TFD_ATOL   2e-7      as in test_hip_torsions.py: a pure fp64 function of the fp32 value table, only the fp32 store differs (2 ulp at 1)
  MOVE_ATOL  1e-5      against the construction: the ring is built and moved in fp64 and rounded to fp32, each coordinate (|x| < 8 here)
                       by up to 2^-22 = 2.4e-7, a height z_j by sqrt(3) times that; an amplitude is sqrt(2 / N) times a sum of N heights
                       with |cos| <= 1, so it moves by at most sqrt(2 N) sqrt(3) 2.4e-7 = 3.3e-6 A at N = 32; tau as MOVE_ATOL of
                       test_hip_torsions.py (atoms >= 0.28 A apart here)
  PHASE_MOVE 2e-4 rad  a phase moves by the amplitude's shift over the amplitude: MOVE_ATOL / 0.05, the smallest amplitude drawn
Phases are compared where the REFERENCE's q_m >= 1e-3 only (below that the phase of a vanishing mode is noise on both sides): a
condition, not a measurement.  The constructed cases draw amplitudes from [0.05, 0.6] A, so none is skipped there; the skipped
share of the random cases is asserted <= 5 % and printed."""
import functools

import numpy as np
import pytest
import torch

import rings_ref as RR
import tfd_ref as TR

pytestmark = pytest.mark.gpu
ANGLE_ATOL, AMP_ATOL, TFD_ATOL, MOVE_ATOL, PHASE_MOVE, Q_MIN = 1e-6, 1e-6, 2e-7, 1e-5, 2e-4, 1e-3


def _dev(pos):
    return torch.from_numpy(np.array(pos, dtype=np.float32, order="C")).cuda()          # (a writable copy: the cached cases are read-only)


def _coords(pos, ptr, idx):
    from agdiff_amd.rings import ring_coordinates
    tau, amp, pucker = ring_coordinates(_dev(pos), np.asarray(ptr, dtype=np.int32), np.asarray(idx, dtype=np.int32))
    assert tau.dtype == amp.dtype == pucker.dtype == torch.float32
    return tau.cpu().numpy(), amp.cpu().numpy(), pucker.cpu().numpy()


def _circ(a, b):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) % (2.0 * np.pi)
    return np.minimum(d, 2.0 * np.pi - d)


def _compare(got, want, ptr, label):
    """the kernel's (tau, amp, pucker) against float64 ones at the three gates; returns (phases compared, phases skipped)"""
    is_phase, amp_of = RR.phase_columns(ptr)
    tau, amp, pk = (g.astype(np.float64) for g in got)
    wtau, wamp, wpk = want
    for g, w in zip((tau, amp, pk), want):
        assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), label
    e_tau = np.nanmax(np.abs(tau - wtau), initial=0.0)
    e_amp = max(np.nanmax(np.abs(amp - wamp), initial=0.0), np.nanmax(np.abs(pk - wpk)[:, ~is_phase], initial=0.0))
    with np.errstate(invalid="ignore"):
        use = wpk[:, amp_of[is_phase]] >= Q_MIN
    e_phi = np.max(_circ(pk[:, is_phase], wpk[:, is_phase])[use], initial=0.0)
    finite = ~np.isnan(wpk[:, is_phase])
    print("%s: tau %.2e rad, amplitudes %.2e A, phases %.2e rad (%d compared, %d skipped)"
          % (label, e_tau, e_amp, e_phi, int(use.sum()), int((finite & ~use).sum())))
    assert e_tau <= ANGLE_ATOL and e_amp <= AMP_ATOL and e_phi <= ANGLE_ATOL, label
    assert ((pk[:, is_phase] >= 0.0) & (pk[:, is_phase] < np.float32(2.0 * np.pi)))[finite].all() and (pk[:, amp_of[is_phase]][finite] >= 0).all()
    assert (tau[~np.isnan(tau)] >= 0).all() and (tau[~np.isnan(tau)] <= np.float32(np.pi)).all()
    return int(use.sum()), int((finite & ~use).sum())


# ------------------------------------------------------------------------------------------------ 1. constructed rings
@functools.lru_cache(maxsize=None)
def _constructed(N, G):
    """(pos fp32 [G, N, 3], the numbers each ring was built from float64 [G, N - 3]) -- moved by a random rigid motion"""
    rng = np.random.default_rng(1000 * N + G)
    M = len(RR.modes(N))
    pos, rows = [], []
    for _ in range(G):
        q, phi = rng.uniform(0.05, 0.6, size=M), rng.uniform(0.0, 2.0 * np.pi, size=M)
        qh = rng.uniform(0.05, 0.6) * rng.choice([-1.0, 1.0]) if N % 2 == 0 else 0.0
        rot, shift = RR.random_motion(rng)
        pos.append(RR.construct(N, q, phi, qh) @ rot.T + 0.5 * shift)
        rows.append(RR.pucker_row(N, q, phi, qh))
    pos = np.stack(pos).astype(np.float32)
    assert np.abs(pos).max() < 8.0
    pos.setflags(write=False)
    return pos, np.stack(rows)


@pytest.mark.parametrize("N", [4, 5, 6, 7, 8, 12, 32])
def test_constructed_rings_come_back(N):
    ptr, idx = [0, N], list(range(N))
    is_phase, _ = RR.phase_columns(ptr)
    for G in (1, 3, 33):
        pos, built = _constructed(N, G)
        got = _coords(pos, ptr, idx)
        compared, skipped = _compare(got, RR.ring_coords(pos, ptr, idx), ptr, "N = %d, G = %d" % (N, G))
        assert skipped == 0 and compared == G * len(RR.modes(N))
        pk = got[2].astype(np.float64)
        assert np.abs(pk - built)[:, ~is_phase].max(initial=0.0) <= MOVE_ATOL
        assert _circ(pk, built)[:, is_phase].max(initial=0.0) <= PHASE_MOVE
        assert np.abs(got[1].astype(np.float64) - np.sqrt((built[:, ~is_phase] ** 2).sum(1, keepdims=True))).max() <= MOVE_ATOL     # Parseval


def test_chair_boat_and_twist_boat():
    from agdiff_amd.rings import CLASS_NAMES, ring_classes
    pos = np.stack([RR.chair(), RR.boat(), RR.twist_boat(), RR.chair(q3=-0.63)])
    tau, amp, pk = _coords(pos, [0, 6], list(range(6)))
    assert np.abs(np.degrees(tau[:, 0].astype(np.float64)) - [60.15, 30.87, 35.37, 60.15]).max() <= 0.01
    assert pk[0, 0] <= 1e-6 and pk[3, 0] <= 1e-6                 # the perfect chair: q_2 vanishes and its phase means nothing
    # (against the construction, whose coordinates were rounded to fp32: the MOVE gates)
    assert abs(pk[0, 2] - 0.63) <= MOVE_ATOL and abs(pk[3, 2] + 0.63) <= MOVE_ATOL           # only the sign of q_3 tells the ring flip:
    assert abs(float(tau[0, 0]) - float(tau[3, 0])) <= ANGLE_ATOL                             # tau does not
    assert np.abs(pk[1:3, 0] - 0.7).max() <= MOVE_ATOL and np.abs(pk[1:3, 2]).max() <= MOVE_ATOL
    assert _circ(pk[1, 1], 0.0) <= PHASE_MOVE and _circ(pk[2, 1], np.pi / 6) <= PHASE_MOVE
    assert np.abs(amp[:, 0] - [0.63, 0.7, 0.7, 0.63]).max() <= MOVE_ATOL
    assert [CLASS_NAMES[c] for c in ring_classes([0, 6], pk)[:, 0]] == ["chair", "boat", "twist-boat", "chair"]


# ------------------------------------------------------------------------------------------------ 2. random coordinates, ring tables
def _random_table(rng, n, sizes):
    idx = np.concatenate([rng.permutation(n)[:N] for N in sizes]).astype(np.int32)
    return np.cumsum([0] + list(sizes)).astype(np.int32), idx


@functools.lru_cache(maxsize=None)
def _random_case(n, Rg):
    """(pos fp32 [G, n, 3], ring_ptr, ring_idx, the reference's numbers, the kernel's) -- computed once"""
    rng = np.random.default_rng(100 * n + Rg)
    G = 5
    if (n, Rg) == (61, 7):
        sizes = [30, 30, 32, 4, 5, 6, 7]             # 114 slots: more than a wave's 64, and ring 2 starts at slot 60 and straddles 64
    elif (n, Rg) == (200, 20):
        sizes = [32] * 20                            # 640 slots: a second pass of the kernel (512 slots each), whole rings only
    else:
        sizes = [int(s) for s in rng.integers(4, min(n, 32) + 1, size=Rg)]
    ptr, idx = _random_table(rng, n, sizes)
    pos = (rng.normal(size=(G, n, 3)) * 0.5).astype(np.float32)
    want = RR.ring_coords(pos, ptr, idx)
    assert want[1].max() < 4.0                       # (AMP_ATOL's premise: every amplitude below 4 Angstrom)
    got = _coords(pos, ptr, idx)
    for a in (pos, ptr, idx) + want + got:
        a.setflags(write=False)
    return pos, ptr, idx, want, got


CASES = [(n, Rg) for n in (9, 61, 200) for Rg in (1, 7, 20)]


def test_random_rings_match_the_float64_reference():
    compared = skipped = 0
    for n, Rg in CASES:
        pos, ptr, idx, want, got = _random_case(n, Rg)
        assert got[0].shape == (5, Rg) and got[2].shape == (5, int(ptr[-1]) - 3 * Rg) and np.isfinite(got[2]).all()
        c, s = _compare(got, want, ptr, "n = %d, Rg = %d" % (n, Rg))
        compared, skipped = compared + c, skipped + s
        # Parseval on what the kernel stored
        is_phase, _ = RR.phase_columns(ptr)
        col = ptr.astype(np.int64) - 3 * np.arange(Rg + 1)
        pk = got[2].astype(np.float64)
        for r in range(Rg):
            sq = (np.where(is_phase[col[r]:col[r + 1]], 0.0, pk[:, col[r]:col[r + 1]]) ** 2).sum(1)
            # (up to 16 stored amplitudes, each half an ulp off: their root sum of squares moves by at most sqrt(16) half ulps)
            assert np.abs(np.sqrt(sq) - got[1][:, r]).max() <= 4 * AMP_ATOL
    print("phases skipped because the reference's q_m < %g: %d of %d (%.2f %%)" % (Q_MIN, skipped, compared + skipped, 100.0 * skipped / (compared + skipped)))
    assert skipped <= 0.05 * (compared + skipped)


def test_two_launches_are_bitwise_equal_and_tau_alone_is_the_same_tau():
    from agdiff_amd.rings import ring_torsion_values
    for n, Rg in ((61, 7), (200, 20)):
        pos, ptr, idx, _, got = _random_case(n, Rg)
        again = _coords(pos, ptr, idx)
        for a, b in zip(got, again):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
        alone = ring_torsion_values(_dev(pos), ptr, idx).cpu().numpy()
        assert np.array_equal(alone.view(np.int32), got[0].view(np.int32))


def test_a_rings_numbers_do_not_depend_on_the_rest_of_the_table():
    pos, ptr, idx, _, got = _random_case(200, 20)
    col = ptr.astype(np.int64) - 3 * np.arange(21)
    for r in (0, 7, 15, 16, 19):                                 # (ring 16 opens the kernel's second pass in the full table)
        one = _coords(pos, [0, 32], idx[ptr[r]:ptr[r + 1]])
        assert np.array_equal(one[0][:, 0].view(np.int32), got[0][:, r].view(np.int32))
        assert np.array_equal(one[1][:, 0].view(np.int32), got[1][:, r].view(np.int32))
        assert np.array_equal(one[2].view(np.int32), got[2][:, col[r]:col[r + 1]].view(np.int32))
    pos, ptr, idx, _, got = _random_case(61, 7)                  # the straddling ring, moved to the front of a shorter table
    col = ptr.astype(np.int64) - 3 * np.arange(8)
    sub = _coords(pos, [0, 32, 36], np.concatenate([idx[ptr[2]:ptr[3]], idx[ptr[3]:ptr[4]]]))
    assert np.array_equal(sub[0].view(np.int32), got[0][:, 2:4].view(np.int32))
    assert np.array_equal(sub[2].view(np.int32), got[2][:, col[2]:col[4]].view(np.int32))


def test_broken_rings_are_nan_in_their_own_numbers_only():
    pos, ptr, idx, want, got = _random_case(61, 7)
    n = pos.shape[1]
    col = ptr.astype(np.int64) - 3 * np.arange(8)
    # an index outside [0, n) in rings 2 (n) and 4 (-1): NaN there in every conformer, every other number bit for bit as before
    bad = idx.copy()
    bad[ptr[2] + 5], bad[ptr[4] + 1] = n, -1
    b = _coords(pos, ptr, bad)
    ring_bad = np.zeros(7, dtype=bool)
    ring_bad[[2, 4]] = True
    col_bad = np.zeros(col[-1], dtype=bool)
    col_bad[col[2]:col[3]], col_bad[col[4]:col[5]] = True, True
    for k, mask in ((0, ring_bad), (1, ring_bad), (2, col_bad)):
        assert np.isnan(b[k][:, mask]).all() and np.array_equal(b[k][:, ~mask].view(np.int32), got[k][:, ~mask].view(np.int32))
    ref = RR.ring_coords(pos, ptr, bad)
    assert all(np.array_equal(np.isnan(x), np.isnan(y)) for x, y in zip(b, ref))
    # a coordinate that is not finite: NaN in the rings that hold the atom, in that conformer only
    atom = int(idx[ptr[3] + 2])
    holds = np.array([atom in idx[ptr[r]:ptr[r + 1]] for r in range(7)])
    for value in (np.nan, np.inf):
        broken = pos.copy()
        broken[1, atom, 2] = value
        c = _coords(broken, ptr, idx)
        assert np.isnan(c[0][1, holds]).all() and np.isnan(c[1][1, holds]).all() and not np.isnan(c[0][1, ~holds]).any()
        assert np.array_equal(np.delete(c[0], 1, axis=0).view(np.int32), np.delete(got[0], 1, axis=0).view(np.int32))
        assert np.array_equal(c[0][1, ~holds].view(np.int32), got[0][1, ~holds].view(np.int32))
        ref = RR.ring_coords(broken, ptr, idx)
        assert all(np.array_equal(np.isnan(x), np.isnan(y)) for x, y in zip(c, ref))


def test_empty_tables_and_the_size_limits():
    from agdiff_amd import _lib
    from agdiff_amd.rings import ring_coordinates
    pos = _dev(np.zeros((3, 40, 3)))
    tau, amp, pucker = ring_coordinates(pos, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert tau.shape == (3, 0) and amp.shape == (3, 0) and pucker.shape == (3, 0)
    tau, amp, pucker = ring_coordinates(pos[:0].contiguous(), [0, 6], list(range(6)))
    assert tau.shape == (0, 1) and amp.shape == (0, 1) and pucker.shape == (0, 3)
    ring_coordinates(pos, [0, 4, 36], list(range(36)))                               # 4 and 32 atoms: the two ends of the range
    for sizes in ([3], [33], [6, 3], [6, 33, 6]):
        ptr = np.cumsum([0] + sizes).astype(np.int32)
        with pytest.raises(_lib.AgdiffLimitError):
            ring_coordinates(pos, ptr, np.arange(ptr[-1], dtype=np.int32) % 40)
    # the launcher itself: the status, and nothing asked for is an argument error
    lib = _lib.load()
    ptr, idx, out = torch.tensor([0, 33], dtype=torch.int32).cuda(), torch.arange(33, dtype=torch.int32).cuda(), torch.zeros(3, dtype=torch.float32).cuda()
    call = lambda p, o: lib.agdiff_ring_coords(_lib.ptr(pos), _lib.ptr(p), _lib.ptr(idx), 3, 40, 1, _lib.ptr(o), _lib.ptr(None), _lib.ptr(None),
                                               _lib.stream_ptr())
    assert call(ptr, out) == -2 and call(torch.tensor([0, 3], dtype=torch.int32).cuda(), out) == -2
    assert call(torch.tensor([0, 6], dtype=torch.int32).cuda(), None) == -1 and call(torch.tensor([1, 7], dtype=torch.int32).cuda(), out) == -1
    assert call(torch.tensor([0, 6], dtype=torch.int32).cuda(), out) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. the TFD over terms
@functools.lru_cache(maxsize=None)
def _value_case(R, G, Q, T, P):
    """(x [R, Q], y [G, Q] fp32 numpy, tmap, scale, even, weights): dihedral-like columns in [-pi, pi], ring-like ones in [0, pi]
    for the columns that an even term names in row 0; NaNs in both tables"""
    rng = np.random.default_rng(R + 10 * G + 100 * Q + T)
    tmap = rng.integers(0, Q, size=(P, T)).astype(np.int32)
    tmap[0] = rng.permutation(Q)[:T]
    even = rng.integers(0, 2, size=T).astype(np.int32)
    even[0], even[-1] = 0, 1
    scale = np.where(even != 0, [RR.ring_scale(N) for N in rng.integers(4, 13, size=T)], np.pi).astype(np.float32)
    x = rng.uniform(-np.pi, np.pi, size=(R, Q)).astype(np.float32)
    y = rng.uniform(-np.pi, np.pi, size=(G, Q)).astype(np.float32)
    ringcol = np.zeros(Q, dtype=bool)
    ringcol[tmap[0][even != 0]] = True
    x[:, ringcol], y[:, ringcol] = np.abs(x[:, ringcol]) * 0.5, np.abs(y[:, ringcol]) * 0.5
    x[R // 2, int(tmap[0, 0])] = np.nan
    y[G // 3, int(tmap[P - 1, T - 1])] = np.nan
    w = rng.uniform(0.2, 3.0, size=T).astype(np.float32)
    return x, y, tmap, scale, even, w


SHAPES = [(1, 1, 2, 2, 1), (17, 33, 20, 9, 4), (40, 40, 70, 30, 2)]


@pytest.mark.parametrize("R,G,Q,T,P", SHAPES)
def test_tfd_with_terms_matches_the_float64_reference(R, G, Q, T, P):
    from agdiff_amd.ensemble import unpack_bits
    from agdiff_amd.torsions import tfd_from_angles
    x, y, tmap, scale, even, w = _value_case(R, G, Q, T, P)
    xd, yd = _dev(x), _dev(y)
    for weights in (None, w):
        out, mirror, bits = tfd_from_angles(xd, yd, tmap, weights=weights, want_mirror=True, threshold=0.5, rings=(scale, even))
        for got, want in ((out, RR.tfd_terms(x, y, tmap, scale, even, weights)), (mirror, RR.tfd_terms(x, y, tmap, scale, even, weights, mirror=True))):
            g = got.cpu().numpy()
            assert g.dtype == np.float32 and g.shape == (R, G) and (g >= 0).all() and (g <= 1).all()
            err = np.abs(g.astype(np.float64) - want).max()
            print("R, G, Q, T, P = %r, weights %s: largest difference to the reference %.3e" % ((R, G, Q, T, P), weights is not None, err))
            assert err <= TFD_ATOL
        adj = unpack_bits(bits, R)
        assert torch.equal(adj[:, :G], out <= 0.5) and not adj[:, G:].any()              # bits == (out <= thresh) exactly
        only_bits = tfd_from_angles(xd, yd, tmap, weights=weights, want_out=False, threshold=0.5, rings=(scale, even))
        assert only_bits[0] is None and torch.equal(only_bits[2], bits)
    # the NaN of x's row R // 2 sits in term 0's own column: that term counts 1 against every y
    out = tfd_from_angles(xd, yd, tmap[:1], rings=(scale, even))[0]
    assert float(out[R // 2].min()) >= 1.0 / T - TFD_ATOL


@pytest.mark.parametrize("R,G,Q,T,P", SHAPES)
def test_with_scales_pi_and_no_even_term_it_is_the_plain_tfd(R, G, Q, T, P):
    from agdiff_amd.torsions import tfd_from_angles
    x, y, tmap, _, _, w = _value_case(R, G, Q, T, P)
    xd, yd = _dev(x), _dev(y)
    for weights in (None, w):
        plain = tfd_from_angles(xd, yd, tmap, weights=weights, want_mirror=True)
        terms = tfd_from_angles(xd, yd, tmap, weights=weights, want_mirror=True, rings=(np.full(T, np.pi), np.zeros(T)))
        for a, b in zip(plain[:2], terms[:2]):
            assert (a - b).abs().max().item() <= TFD_ATOL


@pytest.mark.parametrize("G", [1, 17, 40])
def test_self_matrix_is_bitwise_symmetric_with_a_zero_diagonal(G):
    from agdiff_amd.ensemble import unpack_bits
    from agdiff_amd.torsions import tfd_from_angles
    rng = np.random.default_rng(G)
    for T in (1, 9, 30):
        Q = T + 3
        val = _dev(rng.uniform(-np.pi, np.pi, size=(G, Q)))
        tmap = rng.integers(0, Q, size=(4, T)).astype(np.int32)
        tmap[0] = np.arange(T)
        even = rng.integers(0, 2, size=T)
        scale = np.where(even != 0, RR.ring_scale(6), np.pi)
        w = rng.uniform(0.2, 3.0, size=T).astype(np.float32)
        for weights in (None, w):
            out, mirror, bits = tfd_from_angles(val, val, tmap, weights=weights, want_mirror=True, threshold=0.3, rings=(scale, even))
            assert torch.equal(out, out.T) and torch.equal(mirror, mirror.T) and not out.diagonal().any()
            assert torch.equal(unpack_bits(bits, G)[:, :G], out <= 0.3)


def test_the_mirror_image_negates_the_torsion_and_leaves_the_ring():
    from agdiff_amd.torsions import tfd_from_angles
    s6 = RR.ring_scale(6)
    x = np.array([[1.0, 0.5], [-2.0, 0.2]], dtype=np.float32)
    y = np.array([[-1.0, 0.5], [2.0, 0.3], [0.4, 1.0]], dtype=np.float32)
    tmap, rings = np.array([[0, 1]], dtype=np.int32), ([np.pi, s6], [0, 1])
    out, mirror, _ = tfd_from_angles(_dev(x), _dev(y), tmap, want_mirror=True, rings=rings)
    assert np.abs(out.cpu().numpy() - RR.tfd_terms(x, y, tmap, *rings)).max() <= TFD_ATOL
    want = RR.tfd_terms(x, y, tmap, *rings, mirror=True)
    assert np.abs(mirror.cpu().numpy() - want).max() <= TFD_ATOL and want[0, 0] == 0.0
    # negating every column -- what the plain kernel's mirror value does -- is another number: the ring term would read 1.0 rad
    negated = RR.tfd_terms(x, -y, tmap, *rings)
    assert np.abs(negated - want).max() > 0.1
    all_odd = tfd_from_angles(_dev(x), _dev(y), tmap, want_mirror=True, rings=([np.pi, s6], [0, 0]))[1]
    assert np.abs(all_odd.cpu().numpy() - negated).max() <= TFD_ATOL


def test_the_column_limit_counts_the_ring_columns():
    from agdiff_amd import _lib
    from agdiff_amd.torsions import MAX_COLUMNS, tfd_from_angles
    val = torch.zeros((2, MAX_COLUMNS + 1), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.AgdiffLimitError):
        tfd_from_angles(val, val, np.array([[0, MAX_COLUMNS]], dtype=np.int32), rings=([np.pi, 1.0], [0, 1]))
    val = torch.zeros((2, MAX_COLUMNS), dtype=torch.float32, device="cuda")           # the largest table: the kernel's largest LDS request
    tmap = np.arange(MAX_COLUMNS, dtype=np.int32)[None]
    out = tfd_from_angles(val, val, tmap, rings=(np.full(MAX_COLUMNS, 1.0), np.ones(MAX_COLUMNS)))[0]
    assert not out.any()


# ------------------------------------------------------------------------------------------------ 4. end to end
def _six_ring_ensemble():
    """15 conformers of a six-carbon ring: 5 chairs, 5 boats, 5 twist-boats, every atom jittered by 0.01 Angstrom"""
    rng = np.random.default_rng(6)
    pos = np.stack([RR.chair()] * 5 + [RR.boat()] * 5 + [RR.twist_boat()] * 5)
    return (pos + 0.01 * rng.normal(size=pos.shape)).astype(np.float32)


def _ring_item(**kw):
    at, bi, bt = TR.cyclohexane()
    return dict(atom_type=at, bond_index=bi, bond_type=bt, **kw)


def test_chairs_and_boats_are_one_family_without_ring_terms_and_two_with_them():
    from agdiff_amd.clusters import cluster_conformers
    from agdiff_amd.ensemble import leader_prune, prune_conformers
    from agdiff_amd.evaluation import CovMatEvaluator, get_tfd_confusion_matrix
    from agdiff_amd.torsions import tfd_self, torsion_table, value_table
    gen = _six_ring_ensemble()
    item = _ring_item(pos_gen=gen)
    assert torsion_table(item)[1].shape == (1, 0)                                  # T = 0: no rotatable bond
    assert prune_conformers(item, 0.2, align=False, metric="tfd")["kept"].tolist() == [0]         # today: every pair is "the same conformer"
    # with the ring as a term: chair against boat 29.3 / 36.34 = 0.81, boat against twist-boat 4.5 / 36.34 = 0.12
    out, bits = tfd_self(item, threshold=0.2, rings=True)
    table = torsion_table(item, rings=True)
    val = value_table(_dev(gen), table[0], table[4], table[5]).cpu().numpy()
    assert val.shape == (15, 1) and np.abs(out.cpu().numpy() - RR.tfd_terms(val, val, table[1], table[2], table[3])).max() <= TFD_ATOL
    o = out.cpu().numpy()
    # (the jitter: 0.01 A on levers of about 1.2 A turns a dihedral by half a degree per atom, four atoms a dihedral, two conformers a
    # pair: tau moves by under 3 degrees, 3 / 36.34 = 0.08 -- far inside the 0.2 that separates the families from the 0.81 between them)
    assert abs(o[0, 5] - 0.81) <= 0.08 and abs(o[5, 10] - 0.12) <= 0.08 and o[:5, :5].max() <= 0.08
    keep, leader, count, n_kept = leader_prune(bits, 15)
    assert torch.nonzero(keep).reshape(-1).tolist() == [0, 5] and int(n_kept.item()) == 2
    assert leader.tolist() == [0] * 5 + [5] * 10
    res = cluster_conformers(item, 0.2, metric="tfd", align=False, tfd_rings=True)
    assert sorted(res["count"].tolist()) == [5, 10] and len(set(res["leader"].tolist()[:5])) == 1
    assert set(res["leader"].tolist()[:5]).isdisjoint(res["leader"].tolist()[5:]) and len(set(res["leader"].tolist()[5:])) == 1
    assert cluster_conformers(item, 0.2, metric="tfd", align=False)["count"].tolist() == [15]
    # evaluation: the chairs as references cover the chairs only
    data = _ring_item(pos_ref=gen[:2], pos_gen=gen, smiles="C1CCCCC1")
    assert not get_tfd_confusion_matrix(data).any()
    cm = get_tfd_confusion_matrix(data, rings=True)
    assert torch.equal(cm, out[:2]) and torch.equal(get_tfd_confusion_matrix(data, hands=True, rings=True)[1], cm)       # tau is even
    quiet = lambda *_: None
    res = CovMatEvaluator(metric="tfd", tfd_rings=True, print_fn=quiet, ratio=1)(
        [_ring_item(pos_ref=gen[[0, 5]], pos_gen=gen[[1, 2]], smiles="C1CCCCC1")])
    k = int(np.argmin(np.abs(res.thresholds - 0.2)))
    assert res.CoverageR[0, k] == 0.5 and CovMatEvaluator(metric="tfd", print_fn=quiet, ratio=1)(
        [_ring_item(pos_ref=gen[[0, 5]], pos_gen=gen[[1, 2]], smiles="C1CCCCC1")]).CoverageR[0, k] == 1.0


def test_command_lines_cluster_with_ring_terms_and_write_the_ring_table(tmp_path, capsys):
    from agdiff_amd import clusters, driver, rings
    gen = _six_ring_ensemble()
    at, bi, bt = TR.cyclohexane()
    driver.save_testset(str(tmp_path / "test.npz"), [dict(atom_type=at, edge_index=bi, edge_type=bt, num_refs=2, name="cyclohexane")])
    np.savez(str(tmp_path / "samples_all.npz"), pos_gen_0=gen)
    common = ["--samples", str(tmp_path / "samples_all.npz"), "--testset", str(tmp_path / "test.npz")]
    out = clusters.main(common + ["--tfd", "0.2", "--tfd-rings", "--out", str(tmp_path / "clusters.npz")])
    assert sorted(out["count_0"].tolist()) == [5, 10]
    lead = out["leader_0"].tolist()
    assert len(set(lead[:5])) == 1 and len(set(lead[5:])) == 1 and lead[0] != lead[5]
    assert clusters.main(common + ["--tfd", "0.2", "--out", str(tmp_path / "plain.npz")])["count_0"].tolist() == [15]
    capsys.readouterr()
    rings.main(common + ["--out", str(tmp_path / "rings.npz")])
    assert "1 molecules, 1 rings" in capsys.readouterr().out
    z = np.load(str(tmp_path / "rings.npz"))
    assert z["ring_ptr_0"].tolist() == [0, 6] and z["ring_idx_0"].tolist() == [0, 1, 2, 3, 4, 5] and str(z["name_0"]) == "cyclohexane"
    assert z["ring_tau_0"].shape == (15, 1) and z["ring_amp_0"].shape == (15, 1) and z["ring_pucker_0"].shape == (15, 3)
    assert z["ring_tau_0"].dtype == z["ring_amp_0"].dtype == z["ring_pucker_0"].dtype == np.float32 and z["ring_class_0"].dtype == np.int8
    assert [rings.CLASS_NAMES[c] for c in z["ring_class_0"][:, 0]] == ["chair"] * 5 + ["boat"] * 5 + ["twist-boat"] * 5
    want = RR.ring_coords(gen, [0, 6], list(range(6)))
    assert np.abs(z["ring_tau_0"] - want[0]).max() <= ANGLE_ATOL and np.abs(z["ring_amp_0"] - want[1]).max() <= AMP_ATOL
