"""A float64 numpy restatement of the rigid core hold (csrc/eval.hip: agdiff_hold_core; include/agdiff_hip.h), and the cases the
tests of it share.  SVD Kabsch with the determinant fix instead of the kernel's Horn quaternion: another route to the same proper
rotation.  Anchored in tests/test_core_ref_cpu.py by a known rigid motion and by oracle.covmat_oracle.kabsch_rmsd.

Where the two largest eigenvalues of Horn's key matrix nearly coincide the best rotation is ill-conditioned, and a comparison of
coordinates at 2e-5 Angstrom means nothing: every case generator here ASSERTS a relative gap of at least GAP_MIN for every graph
with three or more selected atoms (an assertion, not a filter: no case is skipped)."""
import numpy as np

GAP_MIN = 1e-3
HEAVY = (1, 2, 3, 63, 64, 65, 129)
FAMILIES = ("noise 0.3", "noise 1.0", "unrelated")


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def walk(rng, n, step=1.5):
    """A random walk of `step` Angstrom steps: chain-like geometry, as tests/test_hip_trajectory.py builds it."""
    d = rng.normal(size=(n, 3))
    d *= step / np.linalg.norm(d, axis=1, keepdims=True)
    return np.cumsum(d, axis=0)


def horn_gap(x, t):
    """(lambda_1 - lambda_2) / |lambda_1| of Horn's 4x4 key matrix of the centred point sets x, t [m, 3] (float64)."""
    x = np.asarray(x, dtype=np.float64) - np.asarray(x, dtype=np.float64).mean(0)
    t = np.asarray(t, dtype=np.float64) - np.asarray(t, dtype=np.float64).mean(0)
    S = t.T @ x
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    K = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    lam = np.linalg.eigvalsh(K)
    return float((lam[3] - lam[2]) / max(abs(lam[3]), 1e-300))


def fit(x, t):
    """The template t [m, 3] superposed on x [m, 3] by the optimal PROPER rotation + translation: (fitted [m, 3], dev) in float64,
    dev = the RMSD between x and the fit."""
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    cx, ct = x.mean(0), t.mean(0)
    xc, tc = x - cx, t - ct
    U, _, Vt = np.linalg.svd(tc.T @ xc)                  # H = sum t x^T; R = V diag(1, 1, d) U^T takes t onto x
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T
    fitted = tc @ R.T + cx
    return fitted, float(np.sqrt(((fitted - x) ** 2).sum() / x.shape[0]))


def hold_core(pos, core_pos, select, batch, weight=1.0, skip=None):
    """agdiff_hold_core restated: (new pos float64 [N, 3] -- NOT rounded to fp32 --, dev float64 [G], touched bool [G]).  The inputs
    are taken as the fp32 values the kernel reads.  A graph with skip != 0, without a selected atom or with a selected coordinate
    of either side that is not finite is left alone with dev = NaN; m = 1 or 2 selected atoms go through the same formula (for
    m = 2 the fit is one of the maximisers: compare distances, not coordinates)."""
    pos = np.asarray(pos, dtype=np.float32).astype(np.float64)
    core = np.asarray(core_pos, dtype=np.float32).astype(np.float64)
    select, batch = np.asarray(select) != 0, np.asarray(batch)
    G = int(batch[-1]) + 1
    w = float(np.float32(weight))
    assert 0.0 < w <= 1.0
    out, dev, touched = pos.copy(), np.full(G, np.nan), np.zeros(G, dtype=bool)
    for g in range(G):
        idx = np.nonzero((batch == g) & select)[0]
        if idx.size == 0 or (skip is not None and skip[g] != 0):
            continue
        if not (np.isfinite(pos[idx]).all() and np.isfinite(core[idx]).all()):
            continue
        fitted, dev[g] = fit(pos[idx], core[idx])
        out[idx] = fitted if w == 1.0 else pos[idx] + w * (fitted - pos[idx])
        touched[g] = True
    return out, dev, touched


def layout(seed=0, heavy=HEAVY):
    """(atom_type, batch) of one packed batch: graph g has heavy[g] heavy atoms with hydrogens interleaved irregularly (the layout
    of tests/test_hip_trajectory.py::_case): graph offsets and the selected atoms' places inside a graph are irregular, and the
    larger graphs cross the 64-lane stride."""
    rng = np.random.default_rng(seed)
    types, batch = [], []
    for g, h in enumerate(heavy):
        ty = []
        for _ in range(h):
            ty.extend([1] * int(rng.integers(0, 3)))
            ty.append(int(rng.choice([6, 7, 8])))
        ty.extend([1] * int(rng.integers(0, 4)))
        types.extend(ty)
        batch.extend([g] * len(ty))
    return np.asarray(types, dtype=np.int64), np.asarray(batch, dtype=np.int64)


def moved(rng, template, family):
    """Where the sampler might have a molecule whose template is `template` [n, 3]: the template rigidly moved plus N(0, 0.3) or
    N(0, 1.0) Angstrom of noise per coordinate, or an unrelated walk."""
    n = template.shape[0]
    if family == "unrelated":
        return walk(rng, n) @ rotation(rng).T + rng.normal(size=3) * 10.0
    noise = {"noise 0.3": 0.3, "noise 1.0": 1.0}[family]
    return template @ rotation(rng).T + rng.normal(size=3) * 10.0 + rng.normal(size=(n, 3)) * noise


def assert_gaps(pos, core_pos, select, batch):
    """Every graph with >= 3 selected atoms is well conditioned; returns the smallest gap seen."""
    smallest = np.inf
    for g in range(int(batch[-1]) + 1):
        idx = np.nonzero((batch == g) & (np.asarray(select) != 0))[0]
        if idx.size >= 3:
            gap = horn_gap(np.asarray(pos, dtype=np.float64)[idx], np.asarray(core_pos, dtype=np.float64)[idx])
            assert gap >= GAP_MIN, "graph %d (%d selected atoms): relative eigenvalue gap %.2e < %.0e" % (g, idx.size, gap, GAP_MIN)
            smallest = min(smallest, gap)
    return smallest


def case(family, seed=0, heavy=HEAVY):
    """One packed batch of len(heavy) graphs: the heavy atoms are the core, `core_pos` a walk per graph (all atoms), `pos` from
    `moved`; fp32 arrays.  Asserts the gaps."""
    atom_type, batch = layout(seed, heavy)
    rng = np.random.default_rng(1000 + seed)
    N, G = atom_type.shape[0], len(heavy)
    core_pos, pos = np.zeros((N, 3)), np.zeros((N, 3))
    for g in range(G):
        idx = np.nonzero(batch == g)[0]
        core_pos[idx] = walk(rng, idx.size) + rng.normal(size=3) * 5.0
        pos[idx] = moved(rng, core_pos[idx], family)
    c = dict(atom_type=atom_type, batch=batch, select=atom_type != 1, core_pos=core_pos.astype(np.float32), pos=pos.astype(np.float32),
             N=N, G=G, family=family)
    c["gap"] = assert_gaps(c["pos"], c["core_pos"], c["select"], batch)
    return c
