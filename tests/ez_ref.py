"""float64 numpy restatement of agdiff_flip_double_bonds (include/agdiff_hip.h), written from the contract and not
from the kernel's source: cos phi of a quad, the state of a bond against its target, and the sequential walk over the bonds with a
180 degree rotation of one side of every wrong one.  The kernel stores fp32 between bonds, so the walk rounds every rotated
coordinate to float32 before the next bond reads it; exact=True never rounds (what the rotation is in exact arithmetic from the
same input), which is how the tests measure what the fp32 rounding between nested flips costs.
"""
import numpy as np


def normals_dot(p, quad):
    """(n1 . n2, |n1|^2, |n2|^2) of one quad (a, i, j, d) in one conformer p float64 [n, 3]"""
    a, i, j, d = (int(x) for x in quad)
    b1, b2, b3 = p[i] - p[a], p[j] - p[i], p[d] - p[j]
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    return float(n1 @ n2), float(n1 @ n1), float(n2 @ n2)


def cos_phi(pos, quads):
    """float64 [G, D]: cos of the dihedral a - i - j - d (0: a and d eclipsed, cis; pi: opposite, trans); NaN for a zero normal or a
    coordinate that is not finite"""
    p = np.asarray(pos, dtype=np.float64)
    p = p.reshape(-1, p.shape[-2], 3)
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    out = np.full((p.shape[0], q.shape[0]), np.nan)
    for g in range(p.shape[0]):
        for c in range(q.shape[0]):
            if not np.isfinite(p[g][q[c]]).all():
                continue
            x, n1sq, n2sq = normals_dot(p[g], q[c])
            if n1sq > 0.0 and n2sq > 0.0:
                out[g, c] = x / np.sqrt(n1sq * n2sq)
    return out


def parity(p, quad):
    """+1 trans (cos phi < 0), -1 cis, 0 undecided: of one quad in one conformer p float64 [n, 3]"""
    if not np.isfinite(p[np.asarray(quad, dtype=np.int64)]).all():
        return 0
    x, n1sq, n2sq = normals_dot(p, quad)
    if not (n1sq > 0.0 and n2sq > 0.0):
        return 0
    return 1 if x < 0.0 else (-1 if x > 0.0 else 0)


def states(pos, quads, target):
    """int8 [G, D] of the positions as given: +1 right, -1 wrong, 0 undecided or target 0"""
    p = np.asarray(pos, dtype=np.float64)
    p = p.reshape(-1, p.shape[-2], 3)
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    t = np.sign(np.asarray(target, dtype=np.int64).reshape(-1))
    out = np.zeros((p.shape[0], q.shape[0]), dtype=np.int8)
    for g in range(p.shape[0]):
        for c in range(q.shape[0]):
            out[g, c] = parity(p[g], q[c]) * t[c]
    return out


def rotate_side(p, i, j, atoms):
    """p' = 2 (p_i + u (u . (p - p_i))) - p for the listed atoms, u = (p_j - p_i) / |p_j - p_i|; i and j themselves are skipped.
    p float64 [n, 3], changed in place."""
    axis = p[j] - p[i]
    u = axis / np.sqrt(axis @ axis)
    idx = np.array([m for m in atoms if m != i and m != j], dtype=np.int64)
    idx = idx[np.isfinite(p[idx]).all(axis=1)]              # (a listed atom that is not finite stays as it is)
    p[idx] = 2.0 * (p[i] + np.outer((p[idx] - p[i]) @ u, u)) - p[idx]


def flip(pos, quads, target, side_ptr, side_idx, exact=False):
    """(pos_out, state int8 [G, D], flipped int32 [G]): the bonds in row order; state from the positions as they are when the bond's
    turn comes; a wrong bond with a side row has that row rotated.  pos_out is float32 (every rotated coordinate rounded to float32
    when it is stored, untouched ones bit for bit), or with exact=True float64 without any rounding after the input's."""
    src = np.asarray(pos, dtype=np.float32)
    src = src.reshape(-1, src.shape[-2], 3)
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    t = np.sign(np.asarray(target, dtype=np.int64).reshape(-1))
    sp, si = np.asarray(side_ptr, dtype=np.int64), np.asarray(side_idx, dtype=np.int64)
    G, D = src.shape[0], q.shape[0]
    out = src.astype(np.float64)
    state, flipped = np.zeros((G, D), dtype=np.int8), np.zeros(G, dtype=np.int32)
    for g in range(G):
        p = out[g]
        for c in range(D):
            state[g, c] = parity(p, q[c]) * t[c]
            row = si[sp[c]:sp[c + 1]]
            if state[g, c] < 0 and row.size:
                rotate_side(p, int(q[c, 1]), int(q[c, 2]), row.tolist())
                if not exact:
                    p[row] = p[row].astype(np.float32).astype(np.float64)
                flipped[g] += 1
    return (out if exact else out.astype(np.float32)), state, flipped
