"""Plain-numpy float64 restatement of agdiff_relax_planar as include/agdiff_hip.h defines it: tests/relax_ref.py's restatement of
agdiff_relax_bounds (its `_evaluate` gives the distance terms) plus the plane term -- per group the centroid and the unit normal of
the best plane, per member h = n . (x_i - c), e = max(|h| - flat_to, 0), the step -sign(h) e n with factor 1, the weight
omega / (b_i + q_i + 1), the stop rule with every e <= pad / 2 and the entry test with (float32)dev > thresh.  `reverse` sums every
atom's terms in the opposite order AND takes the normals by another route (the last right singular vector of the centred members
instead of numpy.linalg.eigh of their covariance), so the self-difference also measures the eigen solver.  Plus the margins a fair
comparison of status and iteration counts needs, and the conformers the tests flatten.  Test infrastructure only."""
import functools

import numpy as np

import planarity_ref as PR
import relax_ref as RR
import validity_ref as VR

THRESH, FLAT_TO = 0.25, 0.10
Margin = RR.Margin


def membership(n, grp_ptr, grp_idx):
    """(mb_ptr, mb_grp) by a plain loop: the groups of every atom, ascending, one entry per occurrence"""
    rows = [[] for _ in range(n)]
    for k in range(len(grp_ptr) - 1):
        for a in grp_idx[grp_ptr[k]:grp_ptr[k + 1]]:
            rows[int(a)].append(k)
    ptr = np.zeros(n + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, np.array([k for r in rows for k in r], dtype=np.int32)


def _planes(x, groups, svd):
    """per group (members, h [m] signed distances, unit normal, gap lambda_mid - lambda_min of the covariance)"""
    out = []
    for mem in groups:
        y = x[mem] - x[mem].mean(0)
        lam, vec = np.linalg.eigh(y.T @ y / mem.shape[0])
        nrm = np.linalg.svd(y)[2][2] if svd else vec[:, 0]
        out.append((mem, y @ nrm, nrm, lam[1] - lam[0]))
    return out


def relax(pos, grp_ptr, grp_idx, pairs, lo, hi, radius, ex_ptr, ex_idx, thresh=THRESH, flat_to=FLAT_TO, clash=RR.CLASH, pad=RR.PAD,
          omega=1.0, max_iter=RR.MAX_ITER, reverse=False, margins=True):
    """dict(pos float32 [G, n, 3], pos64, status int32 [G], iters int32 [G], resid float64 [G], moved float64 [G], gap: the smallest
    eigenvalue gap of any group at any iteration) of agdiff_relax_planar in float64.  With `margins`, Margin is raised when a
    quantity the stop rule compares comes within RR.STOP_MARGIN of its threshold at any iteration, when a distance, ratio or dev
    lies within VR.MARGIN of the bound that decides status 0, or when a group's gap falls below PR.MIN_GAP at any iteration."""
    p32 = np.asarray(pos, dtype=np.float32)
    p32 = p32.reshape(-1, p32.shape[-2], 3)
    G, n = p32.shape[:2]
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    a, b = pr[:, 0], pr[:, 1]
    lo32, hi32 = (np.asarray(v, dtype=np.float32).reshape(-1) for v in (lo, hi))
    lo64, hi64 = lo32.astype(np.float64), hi32.astype(np.float64)
    cl, pd, om, th, ft = (RR._f32(v) for v in (clash, pad, omega, thresh, flat_to))
    r = np.asarray(radius, dtype=np.float32).astype(np.float64)
    rs = r[:, None] + r[None, :]
    T = cl * rs + pd
    pk = np.minimum(pd, 0.5 * (hi64 - lo64))
    ok = RR.allowed_pairs(n, ex_ptr, ex_idx)
    gp, gi = np.asarray(grp_ptr, dtype=np.int64), np.asarray(grp_idx, dtype=np.int64)
    groups = [gi[gp[k]:gp[k + 1]] for k in range(gp.shape[0] - 1)]
    weight = om / (np.bincount(a, minlength=n) + np.bincount(b, minlength=n) + np.bincount(gi, minlength=n) + 1.0)
    out = dict(pos=p32.copy(), pos64=p32.astype(np.float64), status=np.zeros(G, np.int32), iters=np.zeros(G, np.int32),
               resid=np.zeros(G), moved=np.zeros(G), gap=np.full(G, np.inf))
    for g in range(G):
        x0 = p32[g].astype(np.float64)
        if not np.isfinite(x0).all():
            out["status"][g], out["resid"][g] = 3, np.inf
            continue
        # the entry test: agdiff_pair_bounds', agdiff_clash_scan's and agdiff_planar_groups' own rules
        df = np.sqrt(((x0[a] - x0[b]) ** 2).sum(-1)).astype(np.float32)
        v = np.maximum(np.maximum(lo64 - df, df.astype(np.float64) - hi64), 0.0).astype(np.float32)
        diff = x0[:, None, :] - x0[None, :, :]
        ratio = (np.sqrt((diff * diff).sum(-1)) / rs).astype(np.float32)
        dev = np.array([np.abs(h).max() for _, h, _, _ in _planes(x0, groups, reverse)], dtype=np.float32).reshape(-1)
        if margins and not (VR._apart(df, lo32).all() and VR._apart(df, hi32).all() and VR._apart(ratio[ok], np.float32(cl)).all()
                            and VR._apart(dev, np.float32(th)).all()):
            raise Margin("conformer %d: a distance, ratio or dev within %g of the bound that decides status 0" % (g, VR.MARGIN))
        if not (v > 0).any() and not (ratio[ok] < np.float32(cl)).any() and not (dev > np.float32(th)).any():
            continue                                   # status 0: pos and pos64 are the input
        x, it = x0, 0
        while True:
            acc, met, worst, values, limits = RR._evaluate(x, a, b, lo64, hi64, pk, T, ok, pd, reverse)
            planes = _planes(x, groups, reverse)
            if planes:
                flat = np.zeros((n, 3))
                for mem, h, nrm, gap in (planes[::-1] if reverse else planes):
                    e = np.maximum(np.abs(h) - ft, 0.0)
                    np.add.at(flat, mem, (-np.sign(h) * e)[:, None] * nrm[None, :])
                    out["gap"][g] = min(out["gap"][g], gap)
                    values = np.concatenate([values, e])
                    limits = np.concatenate([limits, np.full(e.shape[0], 0.5 * pd)])
                acc = flat + acc if reverse else acc + flat
                met = bool((values <= limits).all())
                worst = float(values.max())
                if margins and out["gap"][g] < PR.MIN_GAP:
                    raise Margin("conformer %d, iteration %d: an eigenvalue gap below %g" % (g, it, PR.MIN_GAP))
            if margins and not (np.abs(values - limits) > RR.STOP_MARGIN * limits).all():
                raise Margin("conformer %d, iteration %d: a stop-rule quantity within %g of its threshold" % (g, it, RR.STOP_MARGIN))
            if met or it == max_iter:
                break
            x = x + weight[:, None] * acc
            it += 1
        out["status"][g], out["iters"][g], out["resid"][g] = (1 if met else 2), it, worst
        out["moved"][g] = np.sqrt(((x - x0) ** 2).sum(-1).mean())
        out["pos64"][g], out["pos"][g] = x, x.astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ the conformers the tests flatten
def item_of(mol, **kw):
    at, ei, et = mol
    return dict(atom_type=at, edge_index=ei, edge_type=et, **kw)


def tables(mol):
    """(grp_ptr, grp_idx, pairs, lo, hi, radius, ex_ptr, ex_idx) of a molecule: planar_groups and the table bounds"""
    from agdiff_amd.planarity import planar_groups
    ptr, idx, _ = planar_groups(item_of(mol))
    return (ptr, idx) + RR.tables(mol)


def styrene4():
    """planarity_ref.styrene_conformers, centred: flat, ring carbon 3 lifted, the CH2 end twisted by 40 degrees, flat with noise"""
    mol, pos = PR.styrene_conformers()
    return mol, RR.centred(pos)


def boat(stretch=0.0):
    """styrene with the ring folded into a boat (carbons 0 and 3 and what hangs on them lifted by 0.5 A); stretch > 0: the vinyl CH2
    end also moved that far along the C=C bond"""
    mol, flat = PR.styrene()
    pos = flat.copy()
    pos[[0, 3, 6, 10], 2] += 0.5
    pos[[7, 13, 14, 15], 2] += 0.5 + 0.3                # the substituent lifted with its carbon, and further
    if stretch:
        pos[[7, 14, 15]] += stretch * (flat[7] - flat[6]) / np.linalg.norm(flat[7] - flat[6])
    return mol, RR.centred(pos)[None]


def vinyl_twist(degrees):
    mol, flat = PR.styrene()
    pos = flat.copy()
    pos[[14, 15]] = PR.rotate_about(flat[[14, 15]], flat[6], flat[7], degrees)
    return mol, RR.centred(pos)[None]


def _methyl(c, away, up, ch=1.09):
    """three hydrogens on carbon c whose other bond points along -away: staggered about `away`, one of them towards `up`"""
    a = away / np.linalg.norm(away)
    e1 = up - (up @ a) * a
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(a, e1)
    t = np.deg2rad(70.5)
    return [c + ch * (np.cos(t) * a + np.sin(t) * (np.cos(f) * e1 + np.sin(f) * e2)) for f in np.deg2rad([0.0, 120.0, 240.0])]


def acetone(lift=0.5):
    """(mol, pos float32 [1, 10, 3]): C0 (carbonyl), O1, C2, C3, hydrogens 4 .. 6 on C2 and 7 .. 9 on C3; planar heavy atoms, then the
    carbonyl carbon lifted out of their plane.  One group: the double bond [0, 1, 2, 3]."""
    ang = lambda deg: np.array([np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg)), 0.0])
    z = np.array([0.0, 0.0, 1.0])
    pos = [np.zeros(3), 1.22 * ang(0), 1.51 * ang(120), 1.51 * ang(240)]
    pos += _methyl(pos[2], ang(120), z) + _methyl(pos[3], ang(240), z)
    pos = np.stack(pos)
    pos[0, 2] += lift
    bonds = [(0, 1, 2), (0, 2, 1), (0, 3, 1)] + [(2, h, 1) for h in (4, 5, 6)] + [(3, h, 1) for h in (7, 8, 9)]
    return PR.graph([6, 8, 6, 6] + [1] * 6, bonds), RR.centred(pos)[None]


def naphthalene(noise=0.3, seed=0, G=1):
    """(mol, pos float32 [G, 18, 3]): carbons 0 .. 9 (0 and 1 are shared by the two rings), hydrogens 10 .. 17, aromatic bonds; planar,
    then Gaussian noise on every coordinate.  Two groups, the rings, with atoms 0 and 1 in both."""
    s, h = 1.40 * np.sqrt(3.0) / 2, 0.70
    c = np.array([[0, h], [0, -h], [s, 2 * h], [2 * s, h], [2 * s, -h], [s, -2 * h], [-s, 2 * h], [-2 * s, h], [-2 * s, -h], [-s, -2 * h]])
    centre = lambda k: np.array([s if k < 6 else -s, 0.0])
    hyd = [c[k] + 1.08 * (c[k] - centre(k)) / np.linalg.norm(c[k] - centre(k)) for k in range(2, 10)]
    flat = np.concatenate([np.concatenate([c, np.stack(hyd)]), np.zeros((18, 1))], axis=1)
    ring = lambda v: [(min(v[k], v[(k + 1) % 6]), max(v[k], v[(k + 1) % 6]), 12) for k in range(6)]
    bonds = sorted(set(ring([0, 2, 3, 4, 5, 1]) + ring([0, 6, 7, 8, 9, 1]))) + [(k, 8 + k, 1) for k in range(2, 10)]
    rng = np.random.default_rng(seed)
    return PR.graph([6] * 10 + [1] * 8, bonds), RR.centred(flat[None] + noise * rng.normal(size=(G, 18, 3)))


def mixed():
    """styrene, six conformers: flat; ring carbon 3 and its hydrogen lifted by 0.7 A (bent only); the CH2 end moved 0.487 A along the
    C=C bond, to 1.827 A, 0.003 past the bound (stretched only: four updates mend it, every one closes a fifth of the gap); both; one
    with a NaN; planarity_ref's bent conformer.  Run with max_iter = 5 the stretched one is repaired and the bent ones are cut short."""
    mol, flat = PR.styrene()
    along = (flat[7] - flat[6]) / np.linalg.norm(flat[7] - flat[6])
    bent, stretched = flat.copy(), flat.copy()
    bent[[3, 10], 2] += 0.7
    stretched[[7, 14, 15]] += 0.487 * along
    both = stretched.copy()
    both[[3, 10], 2] += 0.7
    hard = flat.copy()
    hard[[3, 10], 2] += 0.6
    pos = RR.centred(np.stack([flat, bent, stretched, both, flat, hard]))
    pos[4, 9, 1] = np.nan
    return mol, pos


SITES_9 = [(x, y, 0) for x in (-12, 0, 12) for y in (-12, 0, 12)]
SITES_20 = [(x, y, z) for x in (-12, 0, 12) for y in (-12, 0, 12) for z in (-12, 0, 12) if abs(x) + abs(y) + abs(z) >= 24]


def many_styrenes(sites, G=2, seed=0, first=0):
    """(mol, pos float32 [G, 16 k, 3]): k styrenes 12 A apart as ONE molecule (no bonds between them), each on a lattice site and
    centred on its own box; conformer g deals planarity_ref's four conformers round the sites starting at conformer g + first, with 0.005 A of
    noise per coordinate"""
    mol, four = PR.styrene_conformers()
    at, ei, et = mol
    four = four.astype(np.float64)
    four -= 0.5 * (four[0].max(0) + four[0].min(0))
    k = len(sites)
    atoms = np.tile(at, k)
    edges = np.concatenate([ei + 16 * s for s in range(k)], axis=1)
    rng = np.random.default_rng(16 * k + seed)
    pos = np.stack([np.concatenate([four[(s + g + first) % 4] + np.asarray(sites[s], dtype=np.float64) for s in range(k)]) for g in range(G)])
    return (atoms, edges, np.tile(et, k)), RR.centred(pos + 0.005 * rng.normal(size=pos.shape))


def extra_groups(k, total, seed=0):
    """the caller's own groups on top of the 2 k of k styrenes: subsets of 3 .. 8 of the twelve atoms that lie in a styrene's ring
    plane (the ring carbons, their hydrogens and C6), well away from collinear in the flat molecule (gap >= 0.1 A^2), dealt round
    the styrenes until there are `total` groups"""
    _, flat = PR.styrene()
    plane = np.array([0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12])
    rng = np.random.default_rng(seed)
    extra = []
    while 2 * k + len(extra) < total:
        mem = np.sort(rng.permutation(plane)[:3 + len(extra) % 6])
        y = flat[mem] - flat[mem].mean(0)
        lam = np.linalg.eigvalsh(y.T @ y / mem.shape[0])
        if lam[1] - lam[0] >= 0.1:
            extra.append(mem + 16 * (len(extra) % k))
    return extra


def with_groups(tab, extra):
    ptr, idx = tab[0], tab[1]
    sizes = np.concatenate([np.diff(ptr), [len(e) for e in extra]]).astype(np.int64)
    new_ptr = np.zeros(sizes.shape[0] + 1, dtype=np.int32)
    new_ptr[1:] = np.cumsum(sizes)
    return (new_ptr, np.concatenate([idx] + list(extra)).astype(np.int32)) + tuple(tab[2:])


def _full(k):
    from agdiff_amd import _lib
    return extra_groups(k, _lib.DEFINES["AGDIFF_FLATTEN_MAX_GROUPS"])


# name -> () -> (mol, pos, extra groups or None)
CASES = {
    "styrene4": lambda: styrene4() + (None,),
    "boat": lambda: boat() + (None,),
    "boat_stretched": lambda: boat(1.2) + (None,),
    "acetone": lambda: acetone() + (None,),
    "naphthalene": lambda: naphthalene() + (None,),
    "vinyl85": lambda: vinyl_twist(85.0) + (None,),
    "vinyl90": lambda: vinyl_twist(90.0) + (None,),
    "mixed": lambda: mixed() + (None,),
    "styrene_x9": lambda: many_styrenes(SITES_9) + (None,),
    "styrene_x20": lambda: many_styrenes(SITES_20) + (None,),
    "styrene_x20_full": lambda: many_styrenes(SITES_20, G=1, first=1) + (_full(20),),
}


@functools.lru_cache(maxsize=None)
def solved(key, max_iter=RR.MAX_ITER, omega=1.0):
    """(inputs, forward result, reversed result) of a named case, computed once and left read-only; the margins are asserted by the
    forward run, before any kernel is asked.  inputs = (pos, grp_ptr, grp_idx, pairs, lo, hi, radius, ex_ptr, ex_idx)"""
    mol, pos, extra = CASES[key]()
    tab = tables(mol) if extra is None else with_groups(tables(mol), extra)
    fwd = relax(pos, *tab, max_iter=max_iter, omega=omega)
    rev = relax(pos, *tab, max_iter=max_iter, omega=omega, reverse=True, margins=False)
    inputs = (np.asarray(pos, dtype=np.float32),) + tuple(np.asarray(t) for t in tab)
    for arr in inputs + tuple(fwd.values()) + tuple(rev.values()):
        arr.setflags(write=False)
    return inputs, fwd, rev
