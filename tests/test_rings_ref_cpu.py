"""CPU: the float64 restatement of the ring definitions (tests/rings_ref.py) against the construction it is to invert -- atoms at
rho (cos a_j, -sin a_j, 0) + z_j e_z with z_j built from chosen (q_m, phi_m, q_(N/2)) -- and against the invariances the
definitions state.  What the GPU tests compare the kernels with is checked here first."""
import numpy as np
import pytest

import rings_ref as RR

SIZES = [5, 6, 7, 8, 9, 10, 11, 12, 32]


def _drawn(rng, N):
    M = len(RR.modes(N))
    return rng.uniform(0.05, 0.6, size=M), rng.uniform(0.0, 2.0 * np.pi, size=M), (rng.uniform(0.05, 0.6) * rng.choice([-1.0, 1.0]) if N % 2 == 0 else 0.0)


def _circ(a, b):
    d = np.abs(a - b) % (2.0 * np.pi)
    return np.minimum(d, 2.0 * np.pi - d)


@pytest.mark.parametrize("N", SIZES)
def test_reference_returns_what_the_ring_was_built_from(N):
    rng = np.random.default_rng(N)
    ring = list(range(N))
    for _ in range(5):
        q, phi, qh = _drawn(rng, N)
        pos = RR.construct(N, q, phi, qh)
        rot, shift = RR.random_motion(rng)
        Q, row = RR.cremer_pople((pos @ rot.T + shift)[None], ring)
        want = RR.pucker_row(N, q, phi, qh)
        is_phase = np.zeros(N - 3, dtype=bool)
        is_phase[1:2 * len(q):2] = True
        assert np.abs(row[0] - want)[~is_phase].max(initial=0.0) <= 1e-12
        assert _circ(row[0], want)[is_phase].max(initial=0.0) <= 1e-12
        # Parseval
        assert abs(Q[0] ** 2 - ((q * q).sum() + qh * qh)) <= 1e-12
        assert abs((row[0][~is_phase] ** 2).sum() - Q[0] ** 2) <= 1e-12
        # the normal of the construction is +e_z: the heights come back with their sign
        Q0, row0 = RR.cremer_pople(pos[None], ring)
        assert np.abs(row0[0] - want)[~is_phase].max(initial=0.0) <= 1e-12


def test_four_ring_has_the_signed_amplitude_only():
    pos = RR.construct(4, [], [], -0.3)
    Q, row = RR.cremer_pople(pos[None], [0, 1, 2, 3])
    assert row.shape == (1, 1) and abs(row[0, 0] + 0.3) <= 1e-12 and abs(Q[0] - 0.3) <= 1e-12


@pytest.mark.parametrize("N", [5, 6, 7, 8, 12])
def test_invariances_and_the_phase_shifts(N):
    rng = np.random.default_rng(100 + N)
    q, phi, qh = _drawn(rng, N)
    pos = RR.construct(N, q, phi, qh) + 0.02 * rng.normal(size=(N, 3))          # (not the ideal ring: tau has no symmetry to lean on)
    ring = list(range(N))
    tau0 = RR.ring_torsion(pos[None], ring)[0]
    Q0, row0 = RR.cremer_pople(pos[None], ring)
    amps = np.array([2 * k for k in range(len(q))] + ([N - 4] if N % 2 == 0 else []), dtype=int)
    phases = np.array([2 * k + 1 for k in range(len(q))], dtype=int)
    assert 0.0 <= tau0 <= np.pi
    # rigid motion and reflection: tau, Q and the |amplitudes| stay (a reflection turns the normal over: the signed q_(N/2) flips)
    for proper in (True, False):
        rot, shift = RR.random_motion(rng, proper=proper)
        moved = pos @ rot.T + shift
        assert abs(RR.ring_torsion(moved[None], ring)[0] - tau0) <= 1e-12
        Q1, row1 = RR.cremer_pople(moved[None], ring)
        assert abs(Q1[0] - Q0[0]) <= 1e-12 and np.abs(np.abs(row1[0, amps]) - np.abs(row0[0, amps])).max() <= 1e-12
        if proper:
            assert np.abs(row1[0] - row0[0])[amps].max() <= 1e-12 and _circ(row1[0], row0[0])[phases].max(initial=0.0) <= 1e-12
    # restarting the walk at atom s: phi_m -> phi_m + 2 pi m s / N, q_(N/2) -> (-1)^s q_(N/2); tau and the q_m stay
    for s in (1, 2, N - 1):
        walk = ring[s:] + ring[:s]
        assert abs(RR.ring_torsion(pos[None], walk)[0] - tau0) <= 1e-12
        Q1, row1 = RR.cremer_pople(pos[None], walk)
        assert abs(Q1[0] - Q0[0]) <= 1e-12
        for k, m in enumerate(RR.modes(N)):
            assert abs(row1[0, 2 * k] - row0[0, 2 * k]) <= 1e-12
            assert _circ(row1[0, 2 * k + 1], row0[0, 2 * k + 1] + 2.0 * np.pi * m * s / N) <= 1e-12
        if N % 2 == 0:
            assert abs(row1[0, N - 4] - (-1.0) ** s * row0[0, N - 4]) <= 1e-12
    # reversing the walk (0, N - 1, ..., 1): the normal turns over; phi_m -> pi - phi_m, q_(N/2) -> -q_(N/2); tau and the q_m stay
    walk = [ring[0]] + ring[:0:-1]
    assert abs(RR.ring_torsion(pos[None], walk)[0] - tau0) <= 1e-12
    Q1, row1 = RR.cremer_pople(pos[None], walk)
    assert abs(Q1[0] - Q0[0]) <= 1e-12
    for k in range(len(q)):
        assert abs(row1[0, 2 * k] - row0[0, 2 * k]) <= 1e-12
        assert _circ(row1[0, 2 * k + 1], np.pi - row0[0, 2 * k + 1]) <= 1e-12
    if N % 2 == 0:
        assert abs(row1[0, N - 4] + row0[0, N - 4]) <= 1e-12


def test_chair_boat_and_twist_boat_have_the_pinned_ring_torsion_values():
    ring = list(range(6))
    for build, want in ((RR.chair, 60.15), (RR.boat, 30.87), (RR.twist_boat, 35.37)):
        tau = np.degrees(RR.ring_torsion(build()[None], ring)[0])
        assert abs(tau - want) <= 0.01, (build.__name__, tau)
    # a flat ring has tau = 0, and the ring-flipped chair the chair's tau: tau does not see the sign of q_3
    assert RR.ring_torsion(RR.construct(6, [0.0], [0.0], 0.0)[None], ring)[0] <= 1e-12
    assert abs(RR.ring_torsion(RR.chair(q3=-0.63)[None], ring)[0] - RR.ring_torsion(RR.chair()[None], ring)[0]) <= 1e-12
    assert RR.cremer_pople(RR.chair(q3=-0.63)[None], ring)[1][0, 2] < 0 < RR.cremer_pople(RR.chair()[None], ring)[1][0, 2]


def test_broken_rings_are_nan():
    pos = RR.chair()[None].repeat(2, axis=0)
    pos[1, 3, 1] = np.inf
    tau, amp, pucker = RR.ring_coords(pos, [0, 6], list(range(6)))
    assert np.isfinite(tau[0]).all() and np.isfinite(amp[0]).all() and np.isfinite(pucker[0]).all()
    assert np.isnan(tau[1]).all() and np.isnan(amp[1]).all() and np.isnan(pucker[1]).all()
    tau, amp, pucker = RR.ring_coords(pos[:1], [0, 6, 12], [0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 6])
    assert np.isfinite(tau[0, 0]) and np.isnan(tau[0, 1]) and np.isnan(amp[0, 1]) and np.isnan(pucker[0, 3:]).all()
    # a ring on a line has no mean plane: the Cremer-Pople numbers are NaN (and so is tau: every quad is degenerate)
    line = np.zeros((1, 6, 3))
    line[0, :, 0] = np.arange(6)
    tau, amp, pucker = RR.ring_coords(line, [0, 6], list(range(6)))
    assert np.isnan(amp).all() and np.isnan(pucker).all() and np.isnan(tau).all()


def test_tfd_with_terms_on_cases_worked_by_hand():
    deg = np.pi / 180.0
    s6 = RR.ring_scale(6)
    assert abs(np.degrees(s6) - 36.34) <= 0.01
    x = np.array([[60.15 * deg]], dtype=np.float32)          # a chair
    y = np.array([[30.87 * deg], [35.37 * deg], [0.0], [np.nan]], dtype=np.float32)
    out = RR.tfd_terms(x, y, [[0]], [s6], [1])
    assert abs(out[0, 0] - 29.28 / 36.34) <= 1e-3 and out[0, 2] == 1.0 and out[0, 3] == 1.0          # capped; NaN counts 1
    assert abs(RR.tfd_terms(y[:1], y[1:2], [[0]], [s6], [1])[0, 0] - 4.5 / 36.34) <= 1e-3
    # one torsion and one ring: the mirror image negates the torsion only
    x = np.array([[1.0, 0.5]], dtype=np.float32)
    y = np.array([[-1.0, 0.5]], dtype=np.float32)
    tm, sc = [[0, 1]], [np.pi, s6]
    assert abs(RR.tfd_terms(x, y, tm, sc, [0, 1])[0, 0] - (2.0 / np.pi) / 2.0) <= 1e-7
    assert RR.tfd_terms(x, y, tm, sc, [0, 1], mirror=True)[0, 0] == 0.0
    assert abs(RR.tfd_terms(x, y, tm, sc, [0, 0], mirror=True)[0, 0] - 0.5) <= 1e-7           # (negating the ring column too: 1.0 > s6, capped)
    # scales pi, no even term: the plain TFD, up to the scale's fp32 rounding: float32(pi) = pi (1 + 2.8e-8), on values <= 1
    rng = np.random.default_rng(4)
    a = rng.uniform(-np.pi, np.pi, size=(5, 6)).astype(np.float32)
    b = rng.uniform(-np.pi, np.pi, size=(7, 6)).astype(np.float32)
    tm = rng.integers(0, 6, size=(3, 4))
    w = rng.uniform(0.2, 3.0, size=4)
    import tfd_ref as TR
    for mirror in (False, True):
        assert np.abs(RR.tfd_terms(a, b, tm, [np.pi] * 4, [0] * 4, w, mirror=mirror) - TR.tfd(a, b, tm, w, mirror=mirror)).max() <= 3e-8
