"""Plain-numpy float64 restatement of the torsion fingerprint deviation as include/agdiff_hip.h defines it (agdiff_torsion_angles,
agdiff_tfd_matrix), a leader walk, and a few molecular graphs built by hand.  Test infrastructure only."""
import numpy as np

PI = np.pi


# ------------------------------------------------------------------------------------------------ molecules
def graph(atoms, bonds):
    """(atom_type [n], bond_index [2, 2e], bond_type [2e]) from (i, j, type) triples, both directions listed"""
    bi = np.array([[i, j] for i, j, _ in bonds] + [[j, i] for i, j, _ in bonds]).T.reshape(2, -1)
    bt = np.array([t for _, _, t in bonds] * 2)
    return np.array(atoms), bi, bt


def alkane(k):
    """the carbon chain 0 - 1 - ... - (k - 1), no hydrogens"""
    return graph([6] * k, [(i, i + 1, 1) for i in range(k - 1)])


def but_2_yne():
    return graph([6] * 4, [(0, 1, 1), (1, 2, 3), (2, 3, 1)])


def toluene():
    """ring 0 .. 5 (aromatic bonds, type 12), methyl carbon 6 on atom 0"""
    return graph([6] * 7, [(i, (i + 1) % 6, 12) for i in range(6)] + [(0, 6, 1)])


def cyclohexane():
    return graph([6] * 6, [(i, (i + 1) % 6, 1) for i in range(6)])


def biphenyl():
    """rings 0 .. 5 and 6 .. 11 (aromatic bonds), joined by the single bond 0 - 6"""
    ring = lambda o: [(o + i, o + (i + 1) % 6, 12) for i in range(6)]
    return graph([6] * 12, ring(0) + ring(6) + [(0, 6, 1)])


def butane_with_hydrogens_and_hops():
    """n-butane, carbons 0 .. 3, its ten hydrogens 4 .. 13, and every 2- and 3-hop pair listed as type 22 / 23"""
    bonds = [(0, 1, 1), (1, 2, 1), (2, 3, 1)]
    h = 4
    for c, k in ((0, 3), (1, 2), (2, 2), (3, 3)):
        for _ in range(k):
            bonds.append((c, h, 1))
            h += 1
    n = h
    adj = np.zeros((n, n), dtype=np.int64)
    for i, j, _ in bonds:
        adj[i, j] = adj[j, i] = 1
    two = ((adj @ adj) > 0) & (adj == 0) & ~np.eye(n, dtype=bool)
    three = ((adj @ adj @ adj) > 0) & ~two & (adj == 0) & ~np.eye(n, dtype=bool)
    hops = [(i, j, 22) for i in range(n) for j in range(i + 1, n) if two[i, j]]
    hops += [(i, j, 23) for i in range(n) for j in range(i + 1, n) if three[i, j]]
    return graph([6] * 4 + [1] * 10, bonds + hops)


# ------------------------------------------------------------------------------------------------ the definitions
def dihedrals(pos, quads):
    """float64 [G, Q]: theta = atan2(|b2| b1 . n2, n1 . n2) of every quad (a, u, v, b) in every conformer of pos [G, n, 3], every
    coordinate taken to float64 first; NaN when |n1|^2 or |n2|^2 is zero, a coordinate is not finite or an atom is outside [0, n)."""
    p = np.asarray(pos).astype(np.float64)
    p = p.reshape(-1, p.shape[-2], 3)
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    n = p.shape[1]
    inside = ((q >= 0) & (q < n)).all(1)
    qs = np.where(inside[:, None], q, 0)
    a, u, v, b = (p[:, qs[:, k]] for k in range(4))
    with np.errstate(all="ignore"):
        b1, b2, b3 = u - a, v - u, b - v
        n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
        y = np.sqrt((b2 * b2).sum(-1)) * (b1 * n2).sum(-1)
        x = (n1 * n2).sum(-1)
        theta = np.arctan2(y, x)
        ok = (np.isfinite(a).all(-1) & np.isfinite(u).all(-1) & np.isfinite(v).all(-1) & np.isfinite(b).all(-1)
              & ((n1 * n1).sum(-1) > 0) & ((n2 * n2).sum(-1) > 0) & inside[None, :])
    return np.where(ok, theta, np.nan)


def circular_difference(a, b):
    """delta(a, b) = min(|a - b|, 2 pi - |a - b|); pi when either angle is NaN"""
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
        r = np.minimum(d, 2.0 * PI - d)
    return np.where(np.isnan(d), PI, r)


def tfd(ang_x, ang_y, tmap, w=None, mirror=False, one_way=False):
    """float64 [R, G]: min_p min(S_p(x -> y), S_p(y -> x)) from the angle tables [R, Q], [G, Q] as stored (fp32 values, fp64
    arithmetic, t ascending); mirror: every angle of y negated; one_way: S_p(x -> y) only (NOT the TFD: what the definition guards
    against)."""
    ax, ay = np.asarray(ang_x).astype(np.float64), np.asarray(ang_y).astype(np.float64)
    if mirror:
        ay = -ay
    tm = np.asarray(tmap, dtype=np.int64)
    P, T = tm.shape
    R, G = ax.shape[0], ay.shape[0]
    if T == 0:
        return np.zeros((R, G))
    wt = np.ones(T) if w is None else np.asarray(w, dtype=np.float32).astype(np.float64)
    wsum = 0.0
    for t in range(T):
        wsum += wt[t]
    best = np.full((R, G), np.inf)
    for p in range(P):
        sxy, syx = np.zeros((R, G)), np.zeros((R, G))
        for t in range(T):
            sxy += wt[t] * circular_difference(ax[:, None, tm[0, t]], ay[None, :, tm[p, t]])
            syx += wt[t] * circular_difference(ay[None, :, tm[0, t]], ax[:, None, tm[p, t]])
        best = np.minimum(best, sxy if one_way else np.minimum(sxy, syx))
    return best / (PI * wsum)


def leader_walk(adj):
    """the greedy leader rule in conformer order on a boolean adjacency matrix: (keep, leader, count) int32"""
    G = adj.shape[0]
    kept = np.zeros(G, dtype=bool)
    leader = np.zeros(G, dtype=np.int32)
    count = np.zeros(G, dtype=np.int32)
    for i in range(G):
        hits = np.nonzero(adj[i, :i] & kept[:i])[0]
        if hits.size == 0:
            kept[i], leader[i] = True, i
        else:
            leader[i] = hits[0]
        count[leader[i]] += 1
    return kept.astype(np.int32), leader, count


def chain_positions(torsions, bond=1.5, angle=np.deg2rad(111.0)):
    """float64 [k, 3]: a chain of k = len(torsions) + 3 atoms with the given bond length and bond angle whose dihedral
    (i, i + 1, i + 2, i + 3) is torsions[i] in the convention of `dihedrals` (natural extension reference frame)"""
    pts = [np.array([0.0, 0.0, 0.0]), np.array([bond, 0.0, 0.0]),
           np.array([bond - bond * np.cos(angle), bond * np.sin(angle), 0.0])]
    for phi in torsions:
        a, b, c = pts[-3], pts[-2], pts[-1]
        bc = (c - b) / np.linalg.norm(c - b)
        nrm = np.cross(b - a, bc)
        nrm /= np.linalg.norm(nrm)
        m = np.cross(nrm, bc)
        d2 = np.array([-bond * np.cos(angle), bond * np.sin(angle) * np.cos(phi), bond * np.sin(angle) * np.sin(phi)])
        pts.append(c + d2[0] * bc + d2[1] * m + d2[2] * nrm)
    return np.stack(pts)
