"""Plain-numpy float64 restatement of the two geometry checks as include/agdiff_hip.h defines them (agdiff_pair_bounds,
agdiff_clash_scan): brute force over all pairs with a Python set of excluded pairs, float32 rounding of d and of the ratio before any
comparison, the kernels' tie rules.  Plus the margins a fair comparison needs and a few molecules built by hand.  Test infrastructure only."""
import numpy as np

F32_MAX = float(np.finfo(np.float32).max)
GATE = 4.0 * 2.0 ** -24          # one float32 store (2^-24) + an fp64 ulp of contraction, with room: relative
MARGIN = 1e-5                    # no value under test lies this close (relative) to the threshold that decides its count


def _conformers(pos):
    p = np.asarray(pos)
    return p.reshape(-1, p.shape[-2], 3).astype(np.float64)


def distances(pos, pairs):
    """float32 [G, K]: |p_a - p_b| in float64 from the coordinates as given, rounded once; NaN for a pair outside [0, n)"""
    p = _conformers(pos)
    n = p.shape[1]
    q = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    inside = ((q >= 0) & (q < n)).all(1)
    qs = np.where(inside[:, None], q, 0)
    with np.errstate(all="ignore"):
        diff = p[:, qs[:, 0]] - p[:, qs[:, 1]]
        d = np.sqrt((diff * diff).sum(-1))
        return np.where(inside[None, :], d, np.nan).astype(np.float32)


def violations(dist, lo, hi):
    """float32 [G, K]: max(lo - d, d - hi, 0) on the float32 d, +inf when it is not finite"""
    d = np.asarray(dist, dtype=np.float32).astype(np.float64)
    lo64, hi64 = (np.asarray(x, dtype=np.float32).astype(np.float64)[None, :] for x in (lo, hi))
    with np.errstate(all="ignore"):
        v = np.maximum(np.maximum(lo64 - d, d - hi64), 0.0)
    return np.where(np.isfinite(d), v, np.inf).astype(np.float32)


def pair_bounds(pos, pairs, lo, hi):
    """(dist float32 [G, K], viol float32 [G, K], worst float32 [G], worst_pair int32 [G], n_bad int32 [G])"""
    dist = distances(pos, pairs)
    v = violations(dist, lo, hi)
    G, K = v.shape
    if K == 0:
        return dist, v, np.zeros(G, np.float32), np.full(G, -1, np.int32), np.zeros(G, np.int32)
    return dist, v, v.max(1), v.argmax(1).astype(np.int32), (v > 0).sum(1).astype(np.int32)      # (argmax: the lowest index)


def excluded_set(ex_ptr, ex_idx):
    return {(i, int(j)) for i in range(len(ex_ptr) - 1) for j in ex_idx[ex_ptr[i]:ex_ptr[i + 1]]}


def ratios(pos, radius, excluded):
    """(ratio float32 [G, n, n], allowed bool [n, n]): the ratio of every pair, 0 where d is not finite; allowed = i < j and not in the
    Python set `excluded`"""
    p = _conformers(pos)
    n = p.shape[1]
    r = np.asarray(radius, dtype=np.float32).astype(np.float64)
    allowed = np.zeros((n, n), dtype=bool)
    for i in range(n):
        for j in range(i + 1, n):
            allowed[i, j] = (i, j) not in excluded
    with np.errstate(all="ignore"):
        diff = p[:, :, None, :] - p[:, None, :, :]
        d = np.sqrt((diff * diff).sum(-1))
        ratio = np.where(np.isfinite(d), d / (r[:, None] + r[None, :])[None], 0.0).astype(np.float32)
    return ratio, allowed


def clash_scan(pos, radius, excluded, thresh):
    """(min_ratio float32 [G], min_pair int32 [G, 2], n_clash int32 [G], the allowed pairs' ratios float32 [G, M])"""
    ratio, allowed = ratios(pos, radius, excluded)
    G, n = ratio.shape[0], ratio.shape[1]
    ii, jj = np.nonzero(allowed)                      # row-major: (i, j) ascending, i first
    vals = ratio[:, ii, jj]
    if ii.size == 0:
        return np.full(G, np.inf, np.float32), np.full((G, 2), -1, np.int32), np.zeros(G, np.int32), vals
    k = vals.argmin(1)                                # the lowest (i, j) attaining the minimum
    return (vals.min(1), np.stack([ii[k], jj[k]], 1).astype(np.int32), (vals < np.float32(thresh)).sum(1).astype(np.int32), vals)


def _apart(a, b):
    """|a - b| > MARGIN x max(|a|, |b|), elementwise; infinities and exact zeros on both sides count as apart"""
    with np.errstate(all="ignore"):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return ~np.isfinite(a - b) | (np.abs(a - b) > MARGIN * np.maximum(np.abs(a), np.abs(b)))


def assert_bounds_margins(dist, viol, lo, hi):
    """no finite distance within MARGIN (relative) of one of its bounds, and the two largest violations of a conformer apart"""
    fin = np.isfinite(dist)
    assert (_apart(dist, np.asarray(lo)[None, :]) | ~fin).all() and (_apart(dist, np.asarray(hi)[None, :]) | ~fin).all()
    if viol.shape[1] >= 2:
        top = np.sort(viol, axis=1)[:, -2:]
        assert (_apart(top[:, 0], top[:, 1]) | (top[:, 1] == 0) | np.isinf(top[:, 1])).all()


def assert_clash_margins(vals, thresh):
    """no ratio within MARGIN (relative) of the threshold, and the best and second-best ratio of a conformer apart"""
    assert _apart(vals, thresh).all()
    if vals.shape[1] >= 2:
        low = np.sort(vals, axis=1)[:, :2]
        assert (_apart(low[:, 0], low[:, 1]) | (low[:, 0] == 0)).all()


# ------------------------------------------------------------------------------------------------ molecules
def graph(atoms, bonds, order=3):
    """(atom_type [n], edge_index [2, e], edge_type [e]): bonds (i, j, type), both directions, extended to `order` as the data
    sets' AddHigherOrderEdges does (2-hop pairs get type 23, 3-hop pairs 24)"""
    from agdiff_amd.synth import extend_graph_order_np
    src = np.array([b[0] for b in bonds] + [b[1] for b in bonds], dtype=np.int64)
    dst = np.array([b[1] for b in bonds] + [b[0] for b in bonds], dtype=np.int64)
    typ = np.array([b[2] for b in bonds] * 2, dtype=np.int64)
    at = np.asarray(atoms, dtype=np.int64)
    if order <= 1:
        return at, np.stack([src, dst]), typ
    r, c, t = extend_graph_order_np(at.shape[0], src, dst, typ, order=order)
    return at, np.stack([r, c]), t


def random_chain(rng, n, branch=3):
    """a random tree over n carbons (parent among the previous `branch` atoms) + its order-3 list, and positions [n, 3] of a random
    walk with steps of ~1.5 A"""
    bonds = [(int(rng.integers(max(0, a - branch), a)), a, 1) for a in range(1, n)]
    return graph([6] * n, bonds), bonds


def star(k=40):
    """atom 0 bonded to atoms 1 .. k: its exclusion row holds k entries, and every pair of the molecule is at most two bonds apart"""
    return graph([6] * (k + 1), [(0, a, 1) for a in range(1, k + 1)])


def _unit(v):
    return v / np.linalg.norm(v)


def backbone(k, angles, torsions, cc=1.53):
    """float64 [k, 3]: a chain with bond length cc, bond angle angles[i] at atom i + 1 and dihedral torsions[i] over atoms
    i .. i + 3 (natural extension reference frame)"""
    pts = [np.zeros(3), np.array([cc, 0.0, 0.0])]
    if k > 2:
        pts.append(np.array([cc - cc * np.cos(angles[0]), cc * np.sin(angles[0]), 0.0]))
    for i in range(k - 3):
        a, b, c = pts[-3], pts[-2], pts[-1]
        bc = _unit(c - b)
        nrm = _unit(np.cross(b - a, bc))
        m = np.cross(nrm, bc)
        th, phi = angles[i + 1], torsions[i]
        pts.append(c + cc * (-np.cos(th) * bc + np.sin(th) * np.cos(phi) * m + np.sin(th) * np.sin(phi) * nrm))
    return np.stack(pts[:k])


def alkane(k, angle=np.deg2rad(111.0), torsions=None, cc=1.53, ch=1.09, tilt=0.0):
    """n-alkane with k >= 3 carbons built in float64: the backbone above (all-anti unless `torsions` [k - 3] says otherwise, every
    C-C-C angle `angle`), two hydrogens per inner carbon in the plane that bisects its C-C-C angle, three per end carbon staggered
    against the next bond, H-C-H / H-C-C 109.5 deg, C-H `ch`; tilt > 0 leans the two methyl groups' axes away from each other by
    that weight (a folded chain's end hydrogens then do not meet).  Carbons 0 .. k - 1 first, then each carbon's hydrogens in carbon order.
    Returns ((atom_type, edge_index, edge_type) extended to order 3, pos float64 [n, 3])."""
    tors = [np.pi] * (k - 3) if torsions is None else list(torsions)
    c = backbone(k, [angle] * (k - 2), tors, cc)
    atoms, bonds, pos = [6] * k, [(i, i + 1, 1) for i in range(k - 1)], [p for p in c]
    tet = np.deg2rad(109.5) / 2
    th = np.deg2rad(180.0 - 109.5)
    for i in range(k):
        if 0 < i < k - 1:
            u1, u2 = _unit(c[i - 1] - c[i]), _unit(c[i + 1] - c[i])
            out, perp = _unit(-(u1 + u2)), _unit(np.cross(u1, u2))
            dirs = [out * np.cos(tet) + s * perp * np.sin(tet) for s in (1, -1)]
        else:
            nb, nb2 = (1, 2) if i == 0 else (k - 2, k - 3)
            ax = _unit(_unit(c[i] - c[nb]) + tilt * _unit(c[i] - c[k - 1 - i]))
            ref = c[nb2] - c[nb]
            u = _unit(ref - ref.dot(ax) * ax)
            w = np.cross(ax, u)
            dirs = [ax * np.cos(th) + (u * np.cos(a) + w * np.sin(a)) * np.sin(th) for a in np.deg2rad([180.0, 60.0, 300.0])]
        for d in dirs:
            bonds.append((i, len(atoms), 1))
            atoms.append(1)
            pos.append(c[i] + ch * d)
    return graph(atoms, bonds), np.stack(pos)


TILT = 2.0                       # (found by hand: at 1.0 the end hydrogens of the folded pentane still meet)


def fold(k, target, build):
    """bisection over x in [lo, hi] of build(x) -> (mol, pos) until |C_0 - C_{k-1}| = target (the distance must grow with x)"""
    lo, hi = build.range
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        pos = build(mid)[1]
        if np.linalg.norm(pos[0] - pos[k - 1]) < target:
            lo = mid
        else:
            hi = mid
    return build(0.5 * (lo + hi))


def folded_butane(target=1.9):
    """n-butane, planar syn (torsion 0), the two C-C-C angles narrowed until the end carbons are `target` apart"""
    build = lambda ang: alkane(4, angle=ang, torsions=[0.0], tilt=TILT)
    build.range = (np.deg2rad(80.0), np.deg2rad(111.0))
    return fold(4, target, build)


def folded_pentane(target=1.9):
    """n-pentane with torsions (+t, -t), t closed from the syn-pentane arrangement until C1 and C5 are `target` apart"""
    build = lambda t: alkane(5, torsions=[t, -t], tilt=TILT)
    build.range = (np.deg2rad(5.0), np.deg2rad(120.0))
    return fold(5, target, build)
