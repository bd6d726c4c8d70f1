"""CPU: the float64 restatement of the rigid core hold (tests/core_ref.py) is anchored before tests/test_hip_core.py compares the
kernel with it: a known rigid motion, oracle.covmat_oracle.kabsch_rmsd for `dev`, the selection / skip / non-finite rules, and the
conditioning of the case generators."""
import numpy as np

import core_ref as C
from oracle.covmat_oracle import kabsch_rmsd


def _same_shape(a, b):
    """Largest difference between the two point sets' distance matrices (kabsch_rmsd near zero is the square root of a cancelled
    difference, good to ~1e-7 only)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    da = np.linalg.norm(a[:, None] - a[None, :], axis=2)
    db = np.linalg.norm(b[:, None] - b[None, :], axis=2)
    return float(np.abs(da - db).max())


def test_a_rigidly_moved_template_is_fitted_exactly():
    rng = np.random.default_rng(0)
    for m in (3, 4, 9, 70):
        t = C.walk(rng, m) + rng.normal(size=3) * 4.0
        R, shift = C.rotation(rng), rng.normal(size=3) * 9.0
        x = t @ R.T + shift
        fitted, dev = C.fit(x, t)
        assert np.abs(fitted - x).max() < 1e-12 and dev < 1e-12
        # ... and the mirror image is NOT (proper rotations only), for a chiral set
        if m >= 9:
            fitted, dev = C.fit(-(t @ R.T) + shift, t)
            assert dev > 0.1
            assert abs(np.linalg.det(np.linalg.lstsq(t - t.mean(0), fitted - fitted.mean(0), rcond=None)[0]) - 1.0) < 1e-9


def test_dev_is_the_kabsch_rmsd_and_the_fit_keeps_the_template_rigid():
    rng = np.random.default_rng(1)
    for family in C.FAMILIES:
        for m in (3, 5, 64, 129):
            t = C.walk(rng, m)
            x = C.moved(rng, t, family)
            fitted, dev = C.fit(x, t)
            assert abs(dev - kabsch_rmsd(t, x)) < 1e-10 and abs(dev - kabsch_rmsd(x, t)) < 1e-10
            assert _same_shape(fitted, t) < 1e-10                      # the fit IS the template, moved
            assert np.abs(fitted.mean(0) - x.mean(0)).max() < 1e-10    # on the core's centroid
            # optimal: no small extra rotation brings it closer
            for _ in range(5):
                axis = rng.normal(size=3)
                axis /= np.linalg.norm(axis)
                Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
                q = np.eye(3) + np.sin(1e-3) * Kx + (1.0 - np.cos(1e-3)) * Kx @ Kx
                other = (fitted - x.mean(0)) @ q.T + x.mean(0)
                assert np.sqrt(((other - x) ** 2).sum() / m) >= dev - 1e-12


def test_selection_blend_skip_and_non_finite_rules():
    c = C.case("noise 0.3", seed=3, heavy=(1, 2, 5, 70))
    pos, core, sel, batch = c["pos"], c["core_pos"], c["select"], c["batch"]
    new, dev, touched = C.hold_core(pos, core, sel, batch)
    assert touched.all() and np.isfinite(dev).all()
    assert np.array_equal(new[~sel], pos[~sel].astype(np.float64))                      # unselected atoms: untouched
    i0 = np.nonzero((batch == 0) & sel)[0]
    assert np.array_equal(new[i0], pos[i0].astype(np.float64)) and dev[0] == 0.0        # m = 1: the atom stays
    i1 = np.nonzero((batch == 1) & sel)[0]
    d_new, d_tpl = np.linalg.norm(new[i1[0]] - new[i1[1]]), np.linalg.norm(core[i1[0]].astype(np.float64) - core[i1[1]])
    assert abs(d_new - d_tpl) < 1e-12                                                    # m = 2: the pair at the template's distance
    for g in (2, 3):
        idx = np.nonzero((batch == g) & sel)[0]
        assert _same_shape(new[idx], core[idx]) < 1e-10 and abs(dev[g] - kabsch_rmsd(pos[idx], core[idx])) < 1e-10
    # the blend is a straight line between where the atom was and the fit
    half, dev_half, _ = C.hold_core(pos, core, sel, batch, weight=0.5)
    assert np.allclose(half, 0.5 * (pos.astype(np.float64) + new), rtol=0, atol=1e-12) and np.array_equal(dev_half, dev)
    # skip, an empty selection, non-finite selected coordinates: the graph is left alone, dev = NaN; the others do not change
    for disturb in ("skip", "empty", "nan pos", "nan core", "nan unselected"):
        p, t, s, skip = pos.copy(), core.copy(), sel.copy(), None
        idx = np.nonzero((batch == 3) & sel)[0]
        if disturb == "skip":
            skip = np.array([0, 0, 0, 1])
        elif disturb == "empty":
            s[batch == 3] = False
        elif disturb == "nan pos":
            p[idx[66], 1] = np.nan
        elif disturb == "nan core":
            t[idx[2], 0] = np.inf
        else:
            p[np.nonzero((batch == 3) & ~sel)[0][0], 2] = np.nan
        got, d, tch = C.hold_core(p, t, s, batch, skip=skip)
        if disturb == "nan unselected":
            assert tch.all() and np.array_equal(d, dev) and np.array_equal(got[sel], new[sel])
            continue
        assert tch.tolist() == [True, True, True, False] and np.isnan(d[3]) and np.array_equal(d[:3], dev[:3])
        assert np.array_equal(got[batch == 3], p[batch == 3].astype(np.float64), equal_nan=True)
        assert np.array_equal(got[batch != 3], new[batch != 3])


def test_the_case_generators_are_well_conditioned():
    """Seeds 0-199, m in {3, 4, 5, 63, 64, 65, 129}, the three families: the smallest relative gap between the two largest Horn
    eigenvalues stays above GAP_MIN, so the assertion inside the generators excludes nothing."""
    smallest = {}
    for family in C.FAMILIES:
        gaps = []
        for seed in range(200):
            rng = np.random.default_rng(seed)
            for m in (3, 4, 5, 63, 64, 65, 129):
                t = C.walk(rng, m)
                gaps.append(C.horn_gap(C.moved(rng, t, family), t))
        smallest[family] = min(gaps)
    print("core_ref smallest relative eigenvalue gaps over 200 seeds x 7 sizes: %s" % smallest)
    assert min(smallest.values()) >= C.GAP_MIN
    # the packed cases tests/test_hip_core.py uses assert theirs on construction
    for family in C.FAMILIES:
        c = C.case(family)
        assert c["gap"] >= C.GAP_MIN and [int(c["select"][c["batch"] == g].sum()) for g in range(c["G"])] == list(C.HEAVY)
        assert int((~c["select"]).sum()) > 100
