"""Plain-numpy float64 restatement of the ring definitions of include/agdiff_hip.h (agdiff_ring_coords, agdiff_tfd_matrix_terms) and
agdiff_amd/rings.py: the chordless cycles by brute force, the ring torsion value, the Cremer-Pople coordinates and their inverse
(the construction the tests take as the truth), the TFD over terms with a scale and a parity, and a few graphs built by hand.
Test infrastructure only."""
import itertools

import numpy as np

import tfd_ref as TR

PI = np.pi


# ------------------------------------------------------------------------------------------------ molecules
def ring_graph(n, ty=1):
    return TR.graph([6] * n, [(i, (i + 1) % n, ty) for i in range(n)])


def naphthalene():
    """perimeter 0 .. 9 (aromatic), fused across 0 - 5"""
    return TR.graph([6] * 10, [(i, (i + 1) % 10, 12) for i in range(10)] + [(0, 5, 12)])


def bicyclo222octane():
    """bridgeheads 0 and 1, three two-carbon bridges"""
    return TR.graph([6] * 8, [(0, 2, 1), (2, 3, 1), (3, 1, 1), (0, 4, 1), (4, 5, 1), (5, 1, 1), (0, 6, 1), (6, 7, 1), (7, 1, 1)])


def norbornane():
    """bridgeheads 0 and 1, bridges 2 - 3, 4 - 5 and the one-carbon bridge 6"""
    return TR.graph([6] * 7, [(0, 2, 1), (2, 3, 1), (3, 1, 1), (0, 4, 1), (4, 5, 1), (5, 1, 1), (0, 6, 1), (6, 1, 1)])


def spiro44nonane():
    return TR.graph([6] * 9, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 0, 1), (0, 5, 1), (5, 6, 1), (6, 7, 1), (7, 8, 1), (8, 0, 1)])


def cubane():
    """corner k = the bits (x, y, z) of k; an edge where one bit differs"""
    return TR.graph([6] * 8, [(a, b, 1) for a in range(8) for b in range(a + 1, 8) if bin(a ^ b).count("1") == 1])


def cyclohexane_with_hydrogens():
    """carbons 0 .. 5 in a ring, hydrogens 6 .. 17 (two on each carbon)"""
    return TR.graph([6] * 6 + [1] * 12, [(i, (i + 1) % 6, 1) for i in range(6)] + [(i, 6 + 2 * i + k, 1) for i in range(6) for k in range(2)])


def chordless_cycles(n, bonds, lo=4, hi=12):
    """Brute force over atom subsets: a set is a ring iff its induced subgraph is connected with every degree 2 (a chordless
    cycle).  Walked and ordered as rings.find_rings states.  For the small graphs above only."""
    adj = [set() for _ in range(n)]
    for i, j in bonds:
        adj[i].add(j)
        adj[j].add(i)
    out = []
    for size in range(lo, min(hi, n) + 1):
        for sub in itertools.combinations(range(n), size):
            s = set(sub)
            if any(len(adj[a] & s) != 2 for a in sub):
                continue
            first = sub[0]
            walk = [first, min(adj[first] & s)]
            while len(walk) < size:
                nxt = [v for v in adj[walk[-1]] & s if v != walk[-2]]
                if nxt[0] == first:
                    break
                walk.append(nxt[0])
            if len(walk) == size:                                     # (one cycle through all of them, not two disjoint ones)
                out.append(tuple(walk))
    return sorted(out, key=lambda r: (len(r), r))


def heavy_bonds(mol):
    at, bi, bt = mol
    return sorted({(min(int(i), int(j)), max(int(i), int(j))) for (i, j), t in zip(bi.T, bt) if 1 <= t <= 21 and at[i] != 1 and at[j] != 1})


# ------------------------------------------------------------------------------------------------ the construction
def modes(N):
    """the m of the (q_m, phi_m) pairs of an N-ring"""
    return list(range(2, (N - 1) // 2 + 1))


def heights(N, q, phi, q_half=0.0):
    """z_j = sqrt(2 / N) sum_m q_m cos(phi_m + 2 pi m j / N) + sqrt(1 / N) q_(N/2) (-1)^j"""
    j = np.arange(N)
    z = np.zeros(N)
    for m, qm, pm in zip(modes(N), q, phi):
        z += np.sqrt(2.0 / N) * qm * np.cos(pm + 2.0 * PI * m * j / N)
    if N % 2 == 0:
        z += np.sqrt(1.0 / N) * q_half * (-1.0) ** j
    return z


def construct(N, q, phi, q_half=0.0, rho=1.45):
    """float64 [N, 3]: atoms at rho (cos a_j, -sin a_j, 0) + z_j e_z, a_j = 2 pi j / N: the ring whose Cremer-Pople coordinates are
    exactly (q, phi, q_half), with the normal +e_z"""
    a = 2.0 * PI * np.arange(N) / N
    return np.stack([rho * np.cos(a), -rho * np.sin(a), heights(N, q, phi, q_half)], axis=1)


def pucker_row(N, q, phi, q_half=0.0):
    """the ring's N - 3 numbers in the order of agdiff_ring_coords: q_2, phi_2, ..., q_M, phi_M[, q_(N/2)]"""
    row = [v for pair in zip(q, phi) for v in pair]
    return np.array(row + ([q_half] if N % 2 == 0 else []), dtype=np.float64)


def random_motion(rng, proper=True):
    """(rotation [3, 3], shift [3]); proper=False: a rotation-reflection"""
    qm, r = np.linalg.qr(rng.normal(size=(3, 3)))
    qm = qm * np.sign(np.diag(r))
    if (np.linalg.det(qm) < 0) == proper:
        qm[:, 0] = -qm[:, 0]
    return qm, rng.normal(size=3)


# ------------------------------------------------------------------------------------------------ the definitions
def ring_torsion(pos, ring):
    """float64 [G]: (1 / N) sum_j |theta(r_j, r_j+1, r_j+2, r_j+3)|; NaN when a dihedral is NaN or an atom is outside [0, n)"""
    N = len(ring)
    quads = [[ring[j], ring[(j + 1) % N], ring[(j + 2) % N], ring[(j + 3) % N]] for j in range(N)]
    th = np.abs(TR.dihedrals(pos, quads))
    tau = np.zeros(th.shape[0])
    for j in range(N):
        tau = tau + th[:, j]
    return tau / N


def cremer_pople(pos, ring):
    """(Q float64 [G], numbers float64 [G, N - 3] in the order q_2, phi_2, ..., q_M, phi_M[, q_(N/2)]) of one ring in every
    conformer of pos [G, n, 3]; all NaN when |R' x R''|^2 is zero, a coordinate is not finite or an atom is outside [0, n)"""
    p = np.asarray(pos).astype(np.float64)
    p = p.reshape(-1, p.shape[-2], 3)
    G, n = p.shape[0], p.shape[1]
    N = len(ring)
    ring = np.asarray(ring, dtype=np.int64)
    if ((ring < 0) | (ring >= n)).any():
        return np.full(G, np.nan), np.full((G, N - 3), np.nan)
    r = p[:, ring]
    j = np.arange(N)
    with np.errstate(all="ignore"):
        d = r - r.mean(1, keepdims=True)
        rp = (d * np.sin(2.0 * PI * j / N)[None, :, None]).sum(1)
        rpp = (d * np.cos(2.0 * PI * j / N)[None, :, None]).sum(1)
        nrm = np.cross(rp, rpp)
        nsq = (nrm * nrm).sum(-1)
        ok = np.isfinite(r).all((1, 2)) & (nsq > 0)
        z = (d * (nrm / np.sqrt(nsq)[:, None])[:, None, :]).sum(-1)
        z = np.where(ok[:, None], z, np.nan)
        cols = []
        for m in modes(N):
            a = np.sqrt(2.0 / N) * (z * np.cos(2.0 * PI * m * j / N)).sum(1)
            b = -np.sqrt(2.0 / N) * (z * np.sin(2.0 * PI * m * j / N)).sum(1)
            cols += [np.sqrt(a * a + b * b), np.mod(np.arctan2(b, a), 2.0 * PI)]
        if N % 2 == 0:
            cols.append(np.sqrt(1.0 / N) * (z * (-1.0) ** j).sum(1))
        return np.sqrt((z * z).sum(1)), np.stack(cols, axis=1)


def ring_coords(pos, ring_ptr, ring_idx):
    """(tau [G, Rg], amp [G, Rg], pucker [G, K]) float64: agdiff_ring_coords restated"""
    p = np.asarray(pos)
    p = p.reshape(-1, p.shape[-2], 3)
    ptr = np.asarray(ring_ptr, dtype=np.int64)
    Rg = ptr.shape[0] - 1
    tau, amp = np.zeros((p.shape[0], Rg)), np.zeros((p.shape[0], Rg))
    pucker = np.zeros((p.shape[0], int(ptr[-1]) - 3 * Rg))
    for r in range(Rg):
        ring = [int(a) for a in ring_idx[ptr[r]:ptr[r + 1]]]
        tau[:, r] = ring_torsion(p, ring)
        amp[:, r], pucker[:, ptr[r] - 3 * r:ptr[r + 1] - 3 * (r + 1)] = cremer_pople(p, ring)
    return tau, amp, pucker


def phase_columns(ring_ptr):
    """bool [K]: which columns of `pucker` hold a phase; and int [K]: for a phase column, the column of its amplitude (else -1)"""
    ptr = np.asarray(ring_ptr, dtype=np.int64)
    K = int(ptr[-1]) - 3 * (ptr.shape[0] - 1)
    is_phase, amp_of = np.zeros(K, dtype=bool), np.full(K, -1)
    for r in range(ptr.shape[0] - 1):
        c0 = ptr[r] - 3 * r
        for k in range(len(modes(int(ptr[r + 1] - ptr[r])))):
            is_phase[c0 + 2 * k + 1] = True
            amp_of[c0 + 2 * k + 1] = c0 + 2 * k
    return is_phase, amp_of


def ring_scale(N):
    return PI * np.exp(-0.025 * (N - 14.0) ** 2)


def tfd_terms(val_x, val_y, tmap, scale, even, w=None, mirror=False):
    """float64 [R, G]: min_p min(S_p(x -> y), S_p(y -> x)), S_p(x -> y) = sum_t w_t min(1, delta_t / s_t) / sum_t w_t from the value
    tables as stored (fp32 values, fp64 arithmetic, t ascending), delta_t = s_t when a value is NaN; mirror: y negated where even_t
    is 0.  tmap row 0 names each term's own column."""
    vx, vy = np.asarray(val_x).astype(np.float64), np.asarray(val_y).astype(np.float64)
    tm = np.asarray(tmap, dtype=np.int64)
    P, T = tm.shape
    R, G = vx.shape[0], vy.shape[0]
    if T == 0:
        return np.zeros((R, G))
    s = np.asarray(scale, dtype=np.float32).astype(np.float64)
    sign = np.where(np.asarray(even) != 0, 1.0, -1.0) if mirror else np.ones(T)
    wt = np.ones(T) if w is None else np.asarray(w, dtype=np.float32).astype(np.float64)
    wsum = 0.0
    for t in range(T):
        wsum += wt[t]

    def term(a, b, t):
        with np.errstate(invalid="ignore"):
            d = np.abs(a - b)
            delta = np.minimum(d, 2.0 * PI - d)
            return np.where(np.isnan(d), 1.0, np.minimum(1.0, delta / s[t]))
    best = np.full((R, G), np.inf)
    for p in range(P):
        sxy, syx = np.zeros((R, G)), np.zeros((R, G))
        for t in range(T):
            sxy += wt[t] * term(vx[:, None, tm[0, t]], sign[t] * vy[None, :, tm[p, t]], t)
            syx += wt[t] * term(sign[t] * vy[None, :, tm[0, t]], vx[:, None, tm[p, t]], t)
        best = np.minimum(best, np.minimum(sxy, syx))
    return best / wsum


# ------------------------------------------------------------------------------------------------ six-ring conformers
def chair(rho=1.45, q3=0.63):
    return construct(6, [0.0], [0.0], q3, rho)


def boat(rho=1.45, q2=0.7):
    return construct(6, [q2], [0.0], 0.0, rho)


def twist_boat(rho=1.45, q2=0.7):
    return construct(6, [q2], [PI / 6], 0.0, rho)
