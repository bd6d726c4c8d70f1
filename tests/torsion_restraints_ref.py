"""A float64 numpy restatement of the torsion-restraint launch (csrc/eval.hip: agdiff_restrain_torsions; the rule of
include/agdiff_hip.h and DESIGN.md 4.19), and the cases the tests of it share.  It walks each graph's restraints in row order and
rounds to fp32 after each rotation, where the kernel does.  Anchored by known answers in tests/test_torsion_restraints_ref_cpu.py.

The cases are synthetic and compact on purpose -- points, not chemistry -- so that the error bound the GPU test derives stays below
the project's bar: every |coordinate| <= X_MAX (one fp32 rounding is then <= ULP), every lever arm (the distance of a quad's a and b
from its axis, and the axis length) >= L_MIN, every turned atom within D_MAX of its pivot p_v (which bounds its radius about the
axis), and no atom turned more than DEPTH_MAX times (assertions, not filters: no case is skipped)."""
import numpy as np

X_MAX = 2.0
ULP = 2.0 ** -23                             # spacing of fp32 in [1, 2): the largest rounding step of a coordinate below X_MAX
L_MIN = 1.25
D_MAX = 2.0
DEPTH_MAX = 3
MOVED = (0, 1, 1, 63, 64, 65, 129)           # atoms the (largest) side row of each graph moves; graph 2: seven rows of one atom
EXTRA = (9, 5, 7, 11, 13, 17, 19)            # atoms in no quad and no side row, per graph
FAMILIES = ("violated", "satisfied")
KINDS = ("inside", "above", "below", "inside across the seam", "violated across the seam", "tol 0", "tol pi")
PI = np.pi


def dihedral(pos, quads):
    """float64 [T]: theta = atan2(|b2| b1 . n2, n1 . n2) of every quad (a, u, v, b), from `pos` [N, 3] taken as float64; NaN for a
    zero normal or a coordinate that is not finite."""
    p = np.asarray(pos, dtype=np.float64)
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    b1, b2, b3 = p[q[:, 1]] - p[q[:, 0]], p[q[:, 2]] - p[q[:, 1]], p[q[:, 3]] - p[q[:, 2]]
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    with np.errstate(invalid="ignore"):
        y = np.sqrt((b2 * b2).sum(1)) * (b1 * n2).sum(1)
        x = (n1 * n2).sum(1)
        ok = np.isfinite(p[q].reshape(-1, 12)).all(1) & ((n1 * n1).sum(1) > 0.0) & ((n2 * n2).sum(1) > 0.0)
        return np.where(ok, np.arctan2(y, x), np.nan)


def wrap(d):
    """d in [-2 pi, 2 pi] wrapped into [-pi, pi] by one turn, as the kernel does."""
    d = np.asarray(d, dtype=np.float64)
    return np.where(d > PI, d - 2.0 * PI, np.where(d < -PI, d + 2.0 * PI, d))


def excess(theta, centre, half):
    """e of the circular window: 0 inside, else Delta - sign(Delta) half."""
    d = wrap(np.asarray(theta, dtype=np.float64) - centre)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(d) <= half, 0.0, np.where(d > 0.0, d - half, d + half))


def rotate(points, pu, pv, phi):
    """`points` [m, 3] turned by phi about the axis through pv along (pv - pu), right-handed (Rodrigues), float64."""
    k = (pv - pu) / np.sqrt(((pv - pu) ** 2).sum())
    r = np.asarray(points, dtype=np.float64) - pv
    c, s = np.cos(phi), np.sin(phi)
    return pv + r * c + np.cross(k, r) * s + k * (r @ k)[:, None] * (1.0 - c)


def restrain_torsions(pos, quads, centre, half, batch, side_row, side_ptr, side_idx, weight=1.0, turn=True, skip=None):
    """agdiff_restrain_torsions restated: (new pos float32 [N, 3], angle float64 [T], viol float64 [G], written bool [N]).  quads
    are batch-level and ordered by graph.  viol: the largest |e| of each graph before the call, 0 without restraints, NaN for a graph
    with skip != 0 or a quad coordinate that is not finite -- such a graph is not written and its angles are NaN.  angle: as found
    when the restraint's turn comes.  written: the atoms that were stored (what copy_out receives)."""
    x = np.asarray(pos, dtype=np.float32).copy()
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    centre = np.asarray(centre, dtype=np.float32).astype(np.float64).reshape(-1)
    half = np.asarray(half, dtype=np.float32).astype(np.float64).reshape(-1)
    batch = np.asarray(batch).reshape(-1)
    N, G, T = x.shape[0], int(batch[-1]) + 1, q.shape[0]
    first = np.searchsorted(batch, np.arange(G + 1))
    w = float(np.float32(weight))
    side_row, side_ptr, side_idx = (np.asarray(s, dtype=np.int64).reshape(-1) for s in (side_row, side_ptr, side_idx))
    graph_of = batch[q[:, 1]] if T else np.zeros(0, dtype=np.int64)
    assert 0.0 < w <= 1.0 and (np.diff(graph_of) >= 0).all() and centre.shape[0] == half.shape[0] == side_row.shape[0] == T
    inside = lambda t: ((q[t] >= first[graph_of[t]]) & (q[t] < first[graph_of[t] + 1])).all()
    angle, viol, written = np.full(T, np.nan), np.zeros(G), np.zeros(N, dtype=bool)
    for g in range(G):
        rows = [t for t in np.nonzero(graph_of == g)[0]]
        real = [t for t in rows if inside(t)]
        if (skip is not None and np.asarray(skip)[g] != 0) or not np.isfinite(x[q[real].reshape(-1)]).all():
            viol[g] = np.nan
            continue
        th = dihedral(x, q[real])
        e0 = np.abs(excess(th, centre[real], half[real]))
        viol[g] = np.nanmax(np.concatenate([[0.0], e0[~np.isnan(th)]]))
        for t in rows:
            if not inside(t):
                continue
            theta = dihedral(x, q[t])[0]
            angle[t] = theta
            if np.isnan(theta) or not turn:
                continue
            e = float(excess(theta, centre[t], half[t]))
            r = side_row[t]
            if e == 0.0 or not 0 <= r < side_ptr.shape[0] - 1:
                continue
            u, v = q[t, 1], q[t, 2]
            off = side_idx[side_ptr[r]:side_ptr[r + 1]]
            off = off[(off >= 0) & (off < first[g + 1] - first[g])]
            m = first[g] + off
            m = m[(m != u) & (m != v)]
            m = m[np.isfinite(x[m]).all(1)]
            x64 = x.astype(np.float64)
            x[m] = rotate(x64[m], x64[u], x64[v], -w * e).astype(np.float32)
            written[m] = True
    return x, angle, viol, written


def lever_arm(p, point, u, v):
    """Distance of `point` from the line through u and v."""
    k = (p[v] - p[u]) / np.linalg.norm(p[v] - p[u])
    r = p[point] - p[v]
    return float(np.linalg.norm(r - k * (r @ k)))


def _perp(rng, k):
    """A random unit vector perpendicular to the unit vector k."""
    while True:
        r = rng.normal(size=3)
        r -= k * (r @ k)
        if np.linalg.norm(r) > 0.3:
            return r / np.linalg.norm(r)


def _ball(rng, m, centre, radius):
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.asarray(centre) + d * (radius * rng.random(m) ** (1.0 / 3.0))[:, None]


def _place(a, u, v, theta):
    """b with bond length 1.3 at right angles to the axis u - v such that the dihedral (a, u, v, b) is theta: the cis position
    turned by theta with `rotate` -- which makes the generator itself depend on the sign convention (asserted in `case`)."""
    k = (v - u) / np.linalg.norm(v - u)
    r = a - u
    r = r - k * (r @ k)
    cis = v + 1.3 * r / np.linalg.norm(r)
    return rotate(cis[None, :], u, v, theta)[0]


def _window(kind, theta, violated):
    """(centre, half) of one window kind around the present angle theta; `violated` False: the satisfied twin of the kind."""
    if kind == "inside":
        return theta + 0.2, 0.5
    if kind == "above":
        return (theta - 0.8, 0.3) if violated else (theta - 0.25, 0.3)
    if kind == "below":
        return (theta + 0.8, 0.3) if violated else (theta + 0.25, 0.3)
    if kind == "inside across the seam":                 # theta = -175 degrees: centre 170, half 20
        return np.deg2rad(170.0), np.deg2rad(20.0)
    if kind == "violated across the seam":               # theta = -150 degrees: Delta = +40 degrees
        return (np.deg2rad(170.0), np.deg2rad(20.0)) if violated else (np.deg2rad(170.0), np.deg2rad(45.0))
    if kind == "tol 0":
        return (theta - 0.4, 0.0) if violated else (theta - 0.1, 0.15)
    assert kind == "tol pi"
    return theta + 2.5, PI


_THETA2 = {"inside across the seam": np.deg2rad(-175.0), "violated across the seam": np.deg2rad(-150.0)}


def case(family, seed=0):
    """One packed batch of 7 graphs.  Graph 0: no restraint.  Graph 1: one restraint whose row moves one atom.  Graph 2: a hub with
    seven arms, one restraint per arm and one window kind each (KINDS), each row moving one atom; its first row is graph 1's row
    (offsets 2, 3) -- the two graphs share ONE row of the side table at different first-atom offsets.  Graphs 3, 4, 5: one
    restraint whose row moves 63, 64, 65 atoms.  Graph 6: a six-atom chain c0 .. c5 with a blob of 126 points, and three nested
    restraints on c1-c2, c2-c3 and c3-c4 whose rows move 129, 128 and 127 atoms: the blob turns three times.  Every row lists v
    itself first (the kernel skips it).  Every graph ends in EXTRA[g] atoms that no quad and no row names.  "violated": every
    restraint outside its window except the satisfied kinds of graph 2; "satisfied": all inside.  fp32 arrays."""
    violated = {"violated": True, "satisfied": False}[family]
    rng = np.random.default_rng(900 + seed)
    pos, batch, quads, centre, half, side_row, kinds = [], [], [], [], [], [], []
    rows = []                                            # the side table's rows (offsets from the graph's first atom)
    row_of = {}

    def row(offsets):
        key = tuple(int(o) for o in offsets)
        if key not in row_of:
            row_of[key] = len(rows)
            rows.append(list(key))
        return row_of[key]

    def spin(p):                                         # a random proper rotation about the origin
        qm, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(qm) < 0:
            qm[:, 0] = -qm[:, 0]
        return p @ qm.T

    off = 0
    for g, (moved, extra) in enumerate(zip(MOVED, EXTRA)):
        atoms, own = [], []
        if g in (1, 3, 4, 5):
            u, v = np.array([-0.65, 0.0, 0.0]), np.array([0.65, 0.0, 0.0])
            a = u + 1.3 * _perp(rng, np.array([1.0, 0.0, 0.0]))
            b = _place(a, u, v, rng.uniform(-3.0, 3.0))
            atoms = [a, u, v, b] + list(_ball(rng, moved - 1, v + np.array([0.4, 0.0, 0.0]), 0.9))
            own.append(((0, 1, 2, 3), list(range(2, 3 + moved)), "above" if g % 2 else "below", None))
        elif g == 2:
            hub, a = np.zeros(3), np.array([-1.3, 0.0, 0.0])
            atoms = [a, hub]
            for k, kind in enumerate(KINDS):
                az = 2.0 * PI * k / len(KINDS) + rng.uniform(-0.1, 0.1)
                v = 1.3 * np.array([rng.uniform(-0.1, 0.1), np.cos(az), np.sin(az)])
                v *= 1.3 / np.linalg.norm(v)
                theta = _THETA2.get(kind, rng.uniform(-2.0, 2.0))
                atoms += [v, _place(a, hub, v, theta)]
                own.append(((0, 1, 2 + 2 * k, 3 + 2 * k), [2 + 2 * k, 3 + 2 * k], kind, theta))
        elif g == 6:
            chain = [np.array([0.8 * np.cos(k * np.deg2rad(100.0)), 0.8 * np.sin(k * np.deg2rad(100.0)), 0.45 * k - 1.125]) for k in range(6)]
            atoms = chain + list(_ball(rng, moved - 3, np.array([0.0, 0.0, 0.675]), 0.6))
            n_side = 6 + moved - 3
            for k in range(3):                           # (c_k, c_k+1, c_k+2, c_k+3): turns c_k+2 (v, skipped) and all after it
                own.append(((k, k + 1, k + 2, k + 3), list(range(k + 2, n_side)), ("above", "below", "tol 0")[k], None))
        n_core = len(atoms)
        atoms = (spin(np.asarray(atoms)) if atoms else np.zeros((0, 3)))
        atoms = np.concatenate([atoms, _ball(rng, extra, np.zeros(3), 1.9)])
        p32 = atoms.astype(np.float32)
        for quad, offsets, kind, want in own:
            theta = float(dihedral(p32, [quad])[0])
            if want is not None:
                assert abs(float(wrap(theta - want))) < 1e-5, (g, kind, theta, want)      # the sign convention of `rotate`
            c, h = _window(kind, theta, violated)
            quads.append([off + i for i in quad])
            centre.append(float(wrap(c)))
            half.append(h)
            side_row.append(row(offsets))
            kinds.append(kind)
        pos.append(p32)
        batch.extend([g] * (n_core + extra))
        off += n_core + extra
    pos, batch = np.concatenate(pos), np.asarray(batch, dtype=np.int64)
    quads = np.asarray(quads, dtype=np.int32)
    side_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    side_idx = np.asarray([o for r in rows for o in r], dtype=np.int32)
    c = dict(family=family, pos=pos, batch=batch, quads=quads, centre=np.asarray(centre, dtype=np.float32),
             half=np.asarray(half, dtype=np.float32), side_row=np.asarray(side_row, dtype=np.int32), side_ptr=side_ptr, side_idx=side_idx,
             kinds=kinds, N=pos.shape[0], G=len(MOVED), T=quads.shape[0])
    c["sides"] = (c["side_row"], side_ptr, side_idx)
    first = np.searchsorted(batch, np.arange(c["G"] + 1))
    c["first"] = first
    # ---- the quantities the GPU test's error bound uses
    p = pos.astype(np.float64)
    turns, in_row, levers, reach = np.zeros(c["N"], dtype=np.int64), np.zeros(c["N"], dtype=bool), [], []
    e0 = excess(dihedral(pos, quads), c["centre"].astype(np.float64), c["half"].astype(np.float64))
    for t, (a, u, v, b) in enumerate(quads.tolist()):
        g = batch[u]
        m = first[g] + side_idx[side_ptr[side_row[t]]:side_ptr[side_row[t] + 1]]
        m = m[(m != u) & (m != v)]
        in_row[m] = True
        if e0[t] != 0.0:
            turns[m] += 1
        levers += [lever_arm(p, a, u, v), lever_arm(p, b, u, v), float(np.linalg.norm(p[v] - p[u]))]
        reach.append(float(np.linalg.norm(p[m] - p[v], axis=1).max()))
    c.update(turns=turns, in_row=in_row, e0=e0, x_max=float(np.abs(pos).max()), l_min=min(levers), d_max=max(reach),
             depth=int(turns.max()))
    assert c["x_max"] <= X_MAX and c["l_min"] >= L_MIN and c["d_max"] <= D_MAX and c["depth"] <= DEPTH_MAX, \
        (c["x_max"], c["l_min"], c["d_max"], c["depth"])
    moved_by = [0] * c["G"]
    for t in range(c["T"]):
        g = int(batch[quads[t, 1]])
        moved_by[g] = max(moved_by[g], int(side_ptr[side_row[t] + 1] - side_ptr[side_row[t]]) - 1)
    assert tuple(moved_by) == MOVED and side_row[0] == side_row[1] and first[1] != first[2]      # graphs 1 and 2 share row 0
    assert [int((batch == g).sum() - in_row[batch == g].sum()) >= EXTRA[g] for g in range(c["G"])] == [True] * c["G"]
    if violated:
        assert c["depth"] == 3 and sorted(set(kinds)) == sorted(KINDS)
        assert [bool(x) for x in e0[1:8] != 0.0] == [False, True, True, False, True, True, False]
        assert (np.abs(e0[[0] + list(range(8, c["T"]))]) > 0.1).all()
    else:
        assert (e0 == 0.0).all()
    return c


def error_bound(c):
    """The bound on |kernel - restatement| per coordinate for a case, from the quantities `case` asserts; the derivation is in the
    docstring of tests/test_hip_torsion_restraints.py."""
    amp = 5.0 * D_MAX / L_MIN + 2.0
    d = 0.0
    for _ in range(DEPTH_MAX):
        d = amp * d + ULP
    return d
