"""CPU: known answers that anchor the float64 restatement tests/torsion_restraints_ref.py, which the GPU tests of
agdiff_restrain_torsions compare against: the sign convention of the turn, landing on the window's edge, the +-pi seam, the
independence of restraints on distinct bridges, and the composition of two half-weight calls."""
import numpy as np
import pytest

import torsion_restraints_ref as R

KNOWN = ("sign", "edge", "seam", "independent", "twice half")
TOL = 1e-6                                   # radians: positions pass through fp32 (|x| <= 2), levers >= 1.25


def _butane(theta, extra=0):
    """a, u, v, b with the dihedral theta (bonds 1.3, right angles), + `extra` points that ride with b: one graph; the row [2, 3, ...]
    turns v's side."""
    u, v = np.array([-0.65, 0.0, 0.0]), np.array([0.65, 0.0, 0.0])
    a = u + np.array([0.0, 1.3, 0.0])
    b = R._place(a, u, v, theta)
    rng = np.random.default_rng(3)
    pts = [a, u, v, b] + [b + 0.3 * rng.normal(size=3) for _ in range(extra)]
    pos = np.asarray(pts, dtype=np.float32)
    n = pos.shape[0]
    return pos, np.zeros(n, dtype=np.int64), (np.array([0]), np.array([0, n - 2]), np.arange(2, n))


def _theta(pos, quad=(0, 1, 2, 3)):
    return float(R.dihedral(pos, [quad])[0])


def test_sign_convention_turning_the_v_side_by_phi_adds_phi():
    rng = np.random.default_rng(1)
    for _ in range(50):
        p = rng.normal(size=(4, 3))
        phi = rng.uniform(-3.0, 3.0)
        before = _theta(p)
        q = p.copy()
        q[3:] = R.rotate(p[3:], p[1], p[2], phi)
        d = _theta(q) - before - phi
        assert abs(d - 2.0 * np.pi * np.round(d / (2.0 * np.pi))) < 1e-9       # theta' = theta + phi on the circle
        # reversal: theta(a, u, v, b) = theta(b, v, u, a)
        assert abs(_theta(p) - _theta(p, (3, 2, 1, 0))) < 1e-12
    pos, _, _ = _butane(0.7)
    assert abs(_theta(pos) - 0.7) < TOL                                   # _place builds what dihedral measures


@pytest.mark.parametrize("weight,left", [(1.0, 0.0), (0.5, 0.5)])
def test_lands_on_the_violated_edge(weight, left):
    for theta, centre, half, e in ((1.0, 0.0, 0.25, 0.75), (-1.0, 0.0, 0.25, -0.75), (2.0, 2.5, 0.0, -0.5)):
        pos, batch, sides = _butane(theta, extra=5)
        new, angle, viol, written = R.restrain_torsions(pos, [[0, 1, 2, 3]], [centre], [half], batch, *sides, weight=weight)
        assert abs(angle[0] - theta) < TOL and abs(viol[0] - abs(e)) < TOL
        assert abs(_theta(new) - (theta - weight * e)) < TOL               # theta' = theta - w e
        left_now = float(R.excess(_theta(new), centre, half))
        assert abs(left_now - left * e) < TOL
        assert written.tolist() == [False, False, False] + [True] * 6 and np.array_equal(new[:3], pos[:3])
        # rigid: every distance within the turned side, and to the axis atoms, is kept
        d = lambda p: np.linalg.norm(p[2:, None, :].astype(np.float64) - p[None, 1:, :], axis=2)
        assert np.abs(d(new) - d(pos)).max() < 1e-6


def test_the_window_is_circular():
    pos, batch, sides = _butane(np.deg2rad(-175.0))
    args = ([[0, 1, 2, 3]], [np.deg2rad(170.0)], [np.deg2rad(20.0)], batch) + sides
    new, angle, viol, written = R.restrain_torsions(pos, *args)
    assert viol[0] == 0.0 and not written.any() and np.array_equal(new, pos)   # 170 +- 20 contains -175
    pos, batch, sides = _butane(np.deg2rad(-150.0))
    new, angle, viol, _ = R.restrain_torsions(pos, *args[:3], batch, *sides)
    assert abs(viol[0] - np.deg2rad(20.0)) < TOL                           # Delta = +40 degrees across the seam
    assert abs(float(R.wrap(_theta(new) - np.deg2rad(-170.0)))) < TOL      # lands on the edge 190 = -170 degrees
    assert float(R.excess(np.pi, -np.pi, 0.0)) == 0.0 and float(R.excess(3.0, -3.0, 0.3)) == 0.0


def test_distinct_bridges_are_independent_and_one_pass_satisfies_all():
    c = R.case("violated")
    new, angle, viol, written = R.restrain_torsions(c["pos"], c["quads"], c["centre"], c["half"], c["batch"], *c["sides"])
    after = R.excess(R.dihedral(new, c["quads"]), c["centre"].astype(np.float64), c["half"].astype(np.float64))
    assert (np.abs(c["e0"]) > 0.1).sum() >= 10 and np.abs(after).max() < TOL
    # the angle found at each restraint's turn is the angle before the call: earlier turns have not changed it
    assert np.abs(R.wrap(angle - R.dihedral(c["pos"], c["quads"]))).max() < TOL
    assert np.array_equal(written, c["turns"] > 0)
    # bond lengths of the chain of graph 6 and of the arms of graph 2 are kept
    for a, u, v, b in c["quads"].tolist():
        for i, j in ((a, u), (u, v), (v, b)):
            assert abs(np.linalg.norm(new[i].astype(np.float64) - new[j]) - np.linalg.norm(c["pos"][i].astype(np.float64) - c["pos"][j])) < 1e-6
    same = R.case("satisfied")
    new, _, viol, written = R.restrain_torsions(same["pos"], same["quads"], same["centre"], same["half"], same["batch"], *same["sides"])
    assert np.array_equal(new.view(np.int32), same["pos"].view(np.int32)) and (viol == 0).all() and not written.any()


def test_two_half_weight_calls_compose():
    pos, batch, sides = _butane(1.0, extra=3)
    args = ([[0, 1, 2, 3]], [0.0], [0.25], batch) + sides
    once, _, _, _ = R.restrain_torsions(pos, *args, weight=0.5)
    twice, angle, viol, _ = R.restrain_torsions(once, *args, weight=0.5)
    assert abs(_theta(once) - 0.625) < TOL and abs(angle[0] - 0.625) < TOL and abs(viol[0] - 0.375) < TOL
    assert abs(_theta(twice) - 0.4375) < TOL                               # e: 0.75 -> 0.375 -> 0.1875
    # measuring moves nothing and reports the same
    same, angle0, viol0, written = R.restrain_torsions(once, *args, weight=0.5, turn=False)
    assert np.array_equal(same, once) and not written.any() and angle0[0] == angle[0] and viol0[0] == viol[0]
    # a skipped graph and a non-finite quad coordinate: untouched, NaN
    _, ang, v, w = R.restrain_torsions(pos, *args, skip=[1])
    assert np.isnan(v[0]) and np.isnan(ang[0]) and not w.any()
    bad = pos.copy()
    bad[0, 1] = np.inf
    out, ang, v, w = R.restrain_torsions(bad, *args)
    assert np.isnan(v[0]) and not w.any() and np.array_equal(out[1:], bad[1:])
