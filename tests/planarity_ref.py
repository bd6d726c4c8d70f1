"""Plain-numpy float64 restatement of agdiff_planar_groups as include/agdiff_hip.h defines it, with numpy.linalg.eigh for the
normal: the dev table, worst, worst_group, n_bent, and per entry the gap g = lambda_mid - lambda_min that says how well the normal
is determined and r = the largest distance of a member from the centroid.  Plus the margins a fair comparison needs, the random
inputs of the kernel test and a few molecules built by hand.  Test infrastructure only."""
import numpy as np

GATE_REL = 4.0 * 2.0 ** -24      # the final float32 store (2^-24), with room
GATE_ABS = 1e-9                  # Angstrom: the two eigen solvers (derivation: tests/test_hip_planarity.py)
MARGIN = 1e-5                    # no dev lies this close (relative) to the threshold that decides its count
MIN_GAP = 1e-3                   # Angstrom^2: below it the normal is too poorly determined to compare values
MAX_ATOMS = 8


def planar(pos, grp_ptr, grp_idx, thresh):
    """dict: dev float32 [G, P] (NaN: a group of fewer than 3 or more than 8 members or with an atom outside [0, n); +inf: a member
    coordinate that is not finite), gap / radius float64 [G, P] (NaN where dev is not finite), worst float32 [G], worst_group int32
    [G], n_bent int32 [G]"""
    p = np.asarray(pos)
    p = p.reshape(-1, p.shape[-2], 3).astype(np.float64)
    G, n = p.shape[0], p.shape[1]
    ptr, idx = np.asarray(grp_ptr, dtype=np.int64), np.asarray(grp_idx, dtype=np.int64)
    P = ptr.shape[0] - 1
    dev = np.full((G, P), np.nan, dtype=np.float32)
    gap, radius = np.full((G, P), np.nan), np.full((G, P), np.nan)
    for k in range(P):
        mem = idx[ptr[k]:ptr[k + 1]]
        if not 3 <= mem.shape[0] <= MAX_ATOMS or (mem < 0).any() or (mem >= n).any():
            continue
        for g in range(G):
            x = p[g, mem]
            if not np.isfinite(x).all():
                dev[g, k] = np.inf
                continue
            y = x - x.mean(0)
            lam, vec = np.linalg.eigh(y.T @ y / mem.shape[0])        # (ascending: column 0 is the normal)
            dev[g, k] = np.abs(y @ vec[:, 0]).max()
            gap[g, k] = lam[1] - lam[0]
            radius[g, k] = np.sqrt((y * y).sum(1)).max()
    live = ~np.isnan(dev)
    key = np.where(live, dev, -1.0)
    has = live.any(1) if P else np.zeros(G, dtype=bool)
    worst = np.where(has, key.max(1) if P else 0.0, 0.0).astype(np.float32)
    worst_group = np.where(has, key.argmax(1) if P else -1, -1).astype(np.int32)          # (argmax: the lowest index)
    with np.errstate(invalid="ignore"):
        n_bent = (dev > np.float32(thresh)).sum(1).astype(np.int32)
    return dict(dev=dev, gap=gap, radius=radius, worst=worst, worst_group=worst_group, n_bent=n_bent)


def left_out(ref):
    """bool [G, P]: the entries whose value is not compared -- finite, and the gap below MIN_GAP"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(ref["dev"]) & (ref["gap"] < MIN_GAP)


def assert_margins(ref, pos, thresh, ties=False):
    """run on the reference's own output before the kernel is asked anything: no dev within MARGIN (relative) of thresh, a
    conformer's best and second-best dev that far apart (not in the hand-built tie cases), every |coordinate| below 16"""
    p = np.asarray(pos, dtype=np.float64)
    assert (np.abs(p[np.isfinite(p)]) < 16).all()
    dev = ref["dev"].astype(np.float64)
    fin = np.isfinite(dev)
    assert (np.abs(dev[fin] - np.float32(thresh)) > MARGIN * np.float32(thresh)).all()
    if not ties and dev.shape[1] >= 2:
        top = np.sort(np.where(np.isnan(dev), -1.0, dev), axis=1)[:, -2:]
        with np.errstate(invalid="ignore"):
            apart = np.isinf(top[:, 1]) | (top[:, 0] < 0) | (top[:, 1] - top[:, 0] > MARGIN * top[:, 1])
        assert apart.all()


def close(got, want):
    """every entry within GATE_REL relative + GATE_ABS of the reference; infinities and NaNs in the same places"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    if not (np.array_equal(fin, np.isfinite(got)) and np.array_equal(np.isnan(want), np.isnan(got))):
        return False
    return bool((np.abs(got[fin] - want[fin]) <= GATE_REL * np.abs(want[fin]) + GATE_ABS).all())


# ------------------------------------------------------------------------------------------------ inputs
def random_case(n, G, P, seed):
    """(pos float32 [G, n, 3], grp_ptr, grp_idx int32, shape int8 [P]): P groups of 3 .. 8 distinct atoms, ascending, the sizes cycling so
    that all are present from P = 6, over coordinates ~ N(0, 1.5^2).  Groups share atoms, so a group cannot be shaped on its own: the
    atoms are dealt into three pools instead, and group k takes its atoms from pool k % 3 --
      0  random: left as drawn
      1  nearly planar: per conformer the pool is squashed to a tenth along a random axis through its centroid
      2  planar up to float32 rounding: per conformer the pool is projected onto a random plane through its centroid in float64
    (a subset of a flat pool is flat).  With fewer than 9 atoms every group is of shape 0; a pool smaller than a group's size caps it."""
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(G, n, 3)) * 1.5
    pools = np.array_split(rng.permutation(n), 3) if n >= 9 else [np.arange(n)] * 3
    if n >= 9:
        for which, keep in ((1, 0.1), (2, 0.0)):
            mem = pools[which]
            axis = rng.normal(size=(G, 3))
            axis /= np.linalg.norm(axis, axis=1, keepdims=True)
            y = pos[:, mem] - pos[:, mem].mean(1, keepdims=True)
            pos[:, mem] -= (1.0 - keep) * (y * axis[:, None, :]).sum(-1, keepdims=True) * axis[:, None, :]
    shape = (np.arange(P) % 3 if n >= 9 else np.zeros(P)).astype(np.int8)
    sizes = [min(3 + (k // 3 + k) % (MAX_ATOMS - 2), len(pools[shape[k]])) for k in range(P)]
    ptr = np.zeros(P + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(sizes)
    idx = [np.sort(rng.permutation(pools[shape[k]])[:m]) for k, m in enumerate(sizes)]
    return pos.astype(np.float32), ptr, (np.concatenate(idx) if P else np.zeros(0)).astype(np.int32), shape


# (n, G, P) of the kernel test.  P = 64 fills the wave's lanes once, 65 and 130 stride into a second and third round whose tail is
# reduced with idle lanes; n = 6 has one group, (9, 3, 0) none.  The seeds are 1000 n + P: chosen on the CPU so that the reference's
# own margins hold and it leaves out at most 1 % of a case's entries (tests/test_planarity_cpu.py checks both without a GPU).
CASES = [(6, 1, 1), (9, 3, 0), (23, 33, 5), (61, 10, 64), (61, 10, 65), (200, 7, 130)]
THRESH = 0.25
_cases = {}


def case(n, G, P):
    """((pos, grp_ptr, grp_idx, shape), the reference's results) -- computed once, read-only, margins asserted before any kernel runs"""
    if (n, G, P) not in _cases:
        inputs = random_case(n, G, P, 1000 * n + P)
        ref = planar(inputs[0], inputs[1], inputs[2], THRESH)
        assert_margins(ref, inputs[0], THRESH)
        for a in inputs + tuple(ref.values()):
            a.setflags(write=False)
        _cases[(n, G, P)] = (inputs, ref)
    return _cases[(n, G, P)]


def square(h, centre=(0.0, 0.0, 0.0)):
    """float64 [4, 3]: (+-1, +-1, +-h) around `centre`, the sign of z alternating around the square: the best plane is z = 0 and every
    corner is h from it, exactly"""
    return np.array([[1, 1, h], [-1, 1, -h], [-1, -1, h], [1, -1, -h]], dtype=np.float64) + np.asarray(centre, dtype=np.float64)


def hexagon():
    """float64 [6, 3]: a planar hexagon on the integer grid (z = 3)"""
    return np.array([[2, 0, 3], [1, 2, 3], [-1, 2, 3], [-2, 0, 3], [-1, -2, 3], [1, -2, 3]], dtype=np.float64)


# ------------------------------------------------------------------------------------------------ molecules
def graph(atoms, bonds, order=3):
    """(atom_type [n], edge_index [2, e], edge_type [e]): bonds (i, j, type) in both directions, extended to `order` as the data sets
    are (2-hop pairs get type 23, 3-hop pairs 24); order 1: the raw bonds"""
    from agdiff_amd.synth import extend_graph_order_np
    src = np.array([b[0] for b in bonds] + [b[1] for b in bonds], dtype=np.int64)
    dst = np.array([b[1] for b in bonds] + [b[0] for b in bonds], dtype=np.int64)
    typ = np.array([b[2] for b in bonds] * 2, dtype=np.int64)
    at = np.asarray(atoms, dtype=np.int64)
    if order <= 1 or not bonds:
        return at, np.stack([src, dst]).reshape(2, -1), typ
    r, c, t = extend_graph_order_np(at.shape[0], src, dst, typ, order=order)
    return at, np.stack([r, c]), t


def groups_of(ptr, idx, kind):
    """[(kind, [atoms])] of a CSR"""
    return [(int(kind[k]), idx[ptr[k]:ptr[k + 1]].tolist()) for k in range(len(kind))]


def styrene():
    """(mol, pos float64 [16, 3]): a benzene ring (aromatic bonds, type 12) with a vinyl group, planar in z = 0.  Atoms: ring carbons
    0 .. 5, vinyl carbons 6 (on ring carbon 0) and 7, ring hydrogens 8 .. 12 on carbons 1 .. 5, 13 on C6, 14 and 15 on C7.
    Its planar groups: the ring [0 .. 5] (kind 0, index 0) and the double bond [0, 6, 7, 13, 14, 15] (kind 1, index 1)."""
    ang = lambda deg: np.array([np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg)), 0.0])
    pos = [1.39 * ang(60 * k) for k in range(6)]
    pos.append(pos[0] + 1.47 * ang(0))                   # C6
    pos.append(pos[6] + 1.34 * ang(60))                  # C7
    pos += [2.48 * ang(60 * k) for k in range(1, 6)]     # ring hydrogens
    pos.append(pos[6] + 1.09 * ang(-60))                 # H on C6
    pos += [pos[7] + 1.09 * ang(0), pos[7] + 1.09 * ang(120)]
    atoms = [6] * 8 + [1] * 8
    bonds = [(k, (k + 1) % 6, 12) for k in range(6)] + [(0, 6, 1), (6, 7, 2)] + [(k, 7 + k, 1) for k in range(1, 6)]
    bonds += [(6, 13, 1), (7, 14, 1), (7, 15, 1)]
    return graph(atoms, bonds), np.stack(pos)


def rotate_about(points, a, b, degrees):
    """the points turned about the axis from a to b (Rodrigues)"""
    u = (b - a) / np.linalg.norm(b - a)
    t = np.deg2rad(degrees)
    v = points - a
    return a + v * np.cos(t) + np.cross(u, v) * np.sin(t) + u * (v @ u)[:, None] * (1 - np.cos(t))


def styrene_conformers():
    """(mol, pos float32 [4, 16, 3]): planar; ring carbon 3 and its hydrogen lifted by 0.6 A; the CH2 end of the vinyl group twisted
    by 40 degrees about the C=C axis; planar again with 0.01 A of noise"""
    mol, flat = styrene()
    bent = flat.copy()
    bent[[3, 10], 2] += 0.6
    twisted = flat.copy()
    twisted[[14, 15]] = rotate_about(flat[[14, 15]], flat[6], flat[7], 40.0)
    noisy = flat + 0.01 * np.random.default_rng(0).normal(size=flat.shape)
    return mol, np.stack([flat, bent, twisted, noisy]).astype(np.float32)
