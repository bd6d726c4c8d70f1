"""Anchors tests/ez_ref.py, the float64 restatement the GPU tests of agdiff_flip_double_bonds compare against, on a hand-built,
exactly planar 2-butene-like frame whose answers are known in closed form.  No GPU, no library."""
import numpy as np

import ez_ref as ER
from agdiff_amd.stereo import signed_volumes


def _ang(deg, r=1.0):
    return r * np.array([np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg)), 0.0])


def _frame(cis=True):
    """a(0) - i(1) = j(2) - d(3), H 4 on i, H 5 on j, planar in z = 0; i's side is {1, 0, 4}, j's {2, 3, 5}"""
    i, j = np.zeros(3), np.array([1.34, 0.0, 0.0])
    a, hi = i + _ang(120, 1.5), i + _ang(240, 1.09)
    d, hj = (j + _ang(60, 1.5), j + _ang(-60, 1.09)) if cis else (j + _ang(-60, 1.5), j + _ang(60, 1.09))
    return np.stack([a, i, j, d, hi, hj])


QUAD = np.array([[0, 1, 2, 3]])
SIDE_I, SIDE_J = [1, 0, 4], [2, 3, 5]


def _signed_phi(p):
    b1, b2, b3 = p[1] - p[0], p[2] - p[1], p[3] - p[2]
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    return np.degrees(np.arctan2(np.cross(n1, n2) @ b2 / np.linalg.norm(b2), n1 @ n2))


def _pairs(p, atoms):
    return np.array([np.linalg.norm(p[x] - p[y]) for k, x in enumerate(atoms) for y in atoms[k + 1:]])


def test_cos_phi_and_parity_of_the_planar_frames():
    assert abs(ER.cos_phi(_frame(cis=True), QUAD)[0, 0] - 1.0) < 1e-12
    assert abs(ER.cos_phi(_frame(cis=False), QUAD)[0, 0] + 1.0) < 1e-12
    assert ER.parity(_frame(cis=True), QUAD[0]) == -1 and ER.parity(_frame(cis=False), QUAD[0]) == 1
    assert ER.states(_frame(cis=True), QUAD, [1]).tolist() == [[-1]] and ER.states(_frame(cis=True), QUAD, [-1]).tolist() == [[1]]
    assert ER.states(_frame(cis=True), QUAD, [0]).tolist() == [[0]]


def test_a_flip_turns_cos_plus_one_into_minus_one_and_keeps_every_distance_of_each_side_and_the_bond():
    for side in (SIDE_J, SIDE_I):
        p = _frame(cis=True)
        q = p.copy()
        ER.rotate_side(q, 1, 2, side)
        assert abs(ER.cos_phi(q, QUAD)[0, 0] + 1.0) < 1e-12
        assert np.abs(np.concatenate([_pairs(q, SIDE_I) - _pairs(p, SIDE_I), _pairs(q, SIDE_J) - _pairs(p, SIDE_J)])).max() < 1e-12
        assert len(_pairs(p, SIDE_I)) + len(_pairs(p, SIDE_J)) == 6
        assert abs(np.linalg.norm(q[2] - q[1]) - 1.34) < 1e-12
        assert np.array_equal(q[[1, 2]], p[[1, 2]])                                    # the axis atoms are skipped
        moved = [m for m in side if m not in (1, 2)]
        rest = [m for m in range(6) if m not in moved]
        assert np.array_equal(q[rest], p[rest]) and np.abs(q[moved] - p[moved]).max(axis=1).min() > 0.5


def test_a_bond_twisted_to_thirty_degrees_comes_out_at_minus_one_hundred_and_fifty():
    from planarity_ref import rotate_about
    p = _frame(cis=True)
    p[[3, 5]] = rotate_about(p[[3, 5]], p[1], p[2], 30.0)
    assert abs(_signed_phi(p) - 30.0) < 1e-9
    ER.rotate_side(p, 1, 2, SIDE_J)
    assert abs(_signed_phi(p) + 150.0) < 1e-9


def test_a_four_neighbour_centre_on_the_turning_side_keeps_the_sign_and_value_of_its_volume():
    rng = np.random.default_rng(3)
    p = np.concatenate([_frame(cis=True), _frame(cis=True)[3] + rng.normal(size=(4, 3))])     # atoms 6 .. 9: a centre's neighbours
    side = SIDE_J + [6, 7, 8, 9]
    before = signed_volumes(p[None], [[6, 7, 8, 9]])[0, 0]
    ER.rotate_side(p, 1, 2, side)
    after = signed_volumes(p[None], [[6, 7, 8, 9]])[0, 0]
    assert abs(before) > 1e-3 and abs(after - before) < 1e-12


def test_two_flips_are_the_identity():
    rng = np.random.default_rng(4)
    p = _frame(cis=True) + 0.1 * rng.normal(size=(6, 3))
    q = p.copy()
    ER.rotate_side(q, 1, 2, SIDE_J)
    ER.rotate_side(q, 1, 2, SIDE_J)
    assert np.abs(q - p).max() < 1e-12


def test_the_walk_flips_wrong_bonds_only_and_reports_the_state_before_the_flip():
    from planarity_ref import rotate_about
    skew = lambda p: rotate_about(p, np.array([0.3, -0.2, 0.1]), np.array([1.0, 2.0, 3.0]), 37.0)   # (about x the flip is exact in fp32)
    pos = np.stack([skew(_frame(cis=True)), skew(_frame(cis=False))]).astype(np.float32)
    ptr, idx = np.array([0, 3]), np.array(SIDE_J)
    out, state, flipped = ER.flip(pos, QUAD, [1], ptr, idx)
    assert out.dtype == np.float32 and state.tolist() == [[-1], [1]] and flipped.tolist() == [1, 0]
    assert out[1].tobytes() == pos[1].tobytes() and ER.states(out, QUAD, [1]).tolist() == [[1], [1]]
    exact, state_x, _ = ER.flip(pos, QUAD, [1], ptr, idx, exact=True)
    assert exact.dtype == np.float64 and state_x.tolist() == state.tolist()
    assert 0.0 < np.abs(exact - out).max() < 4 * 2.0 ** -24 * np.abs(pos).max()
    # an empty row: judged, not flipped; target 0: neither; a NaN in the quad: state 0
    out, state, flipped = ER.flip(pos, QUAD, [1], np.array([0, 0]), np.zeros(0, np.int64))
    assert state.tolist() == [[-1], [1]] and flipped.tolist() == [0, 0] and out.tobytes() == pos.tobytes()
    assert ER.flip(pos, QUAD, [0], ptr, idx)[1].tolist() == [[0], [0]]
    bad = pos.copy()
    bad[0, 3, 1] = np.nan
    assert ER.flip(bad, QUAD, [1], ptr, idx)[1].tolist() == [[0], [1]]
