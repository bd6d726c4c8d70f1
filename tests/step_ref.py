"""float64 NumPy reference of the Langevin update (k_langevin_update, csrc/node.hip; update phase of k_sampler_front,
csrc/front.hip) and of the loss kernels (k_perturb_positions, k_diffusion_loss), plus the batch recipes, score draws and
settings that tests/test_step_ref_cpu.py anchors on the CPU and tests/test_hip_step_kernels.py runs on the GPU.

The arithmetic takes edge lists as plain arrays (row, col, score) and knows nothing of device layouts; no torch on that path.
Every scalar and every array arrives as the float32 value the device gets and is widened to float64 before any arithmetic.
"""
import functools

import numpy as np

from agdiff_amd import synth

CUTOFF = 10.0
MIN_PAIR = 0.05          # a draw with two atoms of one molecule closer than this is rejected


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _s(x):
    """A launch scalar as the device receives it: rounded to float32, then widened."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------- arithmetic
def eq_term(pos, row, col, score):
    """geometry.py:9-17: with dd = (pos[row] - pos[col]) / |pos[row] - pos[col]|, dd * score is added to `row` and
    -dd * score to `col`.  Lengths from the float64 positions."""
    pos, score = _f64(pos), _f64(score).reshape(-1)
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    d = pos[row] - pos[col]
    dd = d / np.sqrt((d * d).sum(axis=1, keepdims=True))
    out = np.zeros_like(pos)
    np.add.at(out, row, dd * score[:, None])
    np.add.at(out, col, -dd * score[:, None])
    return out


def clip_norm(v, limit):
    """dualenc.py:586-589; a negative limit means no clipping."""
    v = _f64(v)
    if limit < 0:
        return v.copy()
    nrm = np.sqrt((v * v).sum(axis=-1, keepdims=True))
    return v * np.where(nrm > limit, limit / np.where(nrm > 0, nrm, 1.0), 1.0)


def center(x, batch):
    """dualenc.py:581-583: minus the mean of the atom's graph."""
    x, batch = _f64(x), np.asarray(batch, dtype=np.int64)
    g = int(batch.max()) + 1
    s = np.zeros((g, x.shape[1]))
    np.add.at(s, batch, x)
    cnt = np.maximum(np.bincount(batch, minlength=g), 1)
    return x - (s / cnt[:, None])[batch]


def _type0(radius):
    row, col, score = (np.asarray(a) for a in radius[:3])
    if len(radius) > 3:                          # (row, col, score, type): only type-0 edges enter the global term
        keep = np.asarray(radius[3]) == 0
        row, col, score = row[keep], col[keep], score[keep]
    return row, col, score


def langevin_step(pos, batch, local, radius, noise, *, sigma, step_size, noise_scale, w_global, clip, clip_local, clip_pos,
                  use_global):
    """dualenc.py:506-545: center(pos + step_size * (clip_local(eq_local) + w_global * clip(eq_global)) / sigma
    + noise * noise_scale), clamped to +-clip_pos when clip_pos >= 0.  Returns the new positions and the per-atom masks
    (local clip engaged, global clip engaged, a coordinate clamped)."""
    pos = _f64(pos)
    sigma, step_size, noise_scale, w_global = _s(sigma), _s(step_size), _s(noise_scale), _s(w_global)
    clip, clip_local, clip_pos = _s(clip), _s(clip_local), _s(clip_pos)
    eq_l = eq_term(pos, *local)
    m_local = np.sqrt((eq_l * eq_l).sum(1)) > clip_local if clip_local >= 0 else np.zeros(pos.shape[0], dtype=bool)
    eps = clip_norm(eq_l, clip_local)
    m_global = np.zeros(pos.shape[0], dtype=bool)
    if use_global:
        eq_g = eq_term(pos, *_type0(radius))
        m_global = np.sqrt((eq_g * eq_g).sum(1)) > clip
        eps = eps + w_global * clip_norm(eq_g, clip)
    new = center(pos + step_size * eps / sigma + _f64(noise) * noise_scale, batch)
    m_pos = np.zeros(pos.shape[0], dtype=bool)
    if clip_pos >= 0:
        m_pos = (np.abs(new) > clip_pos).any(axis=1)
        new = np.clip(new, -clip_pos, clip_pos)
    return new, (m_local, m_global, m_pos)


def perturb(pos, noise, alpha, batch):
    """dualenc.py:308-312: pos + noise * sqrt(1 - a) / sqrt(a), a = alpha[graph] (float32 values, widened)."""
    a = _f64(np.asarray(alpha, dtype=np.float32))[np.asarray(batch, dtype=np.int64)][:, None]
    return _f64(pos) + _f64(noise) * np.sqrt(1.0 - a) / np.sqrt(a)


def diffusion_loss(pos_gt, pos_pert, alpha, batch, local, radius, cutoff, rounding=False):
    """dualenc.py:337-385 as k_diffusion_loss documents it: (total, global, local) per atom.  Local = 5 |pred - target|^2 over
    the local edges, global = 2 |...|^2 over the type-0 edges with d_pert <= cutoff; per edge
    d_target = (d_gt - d_pert) / sqrt(1 - a) * sqrt(a), a = alpha[graph of the edge].
    rounding=True appends, per atom and for each of the three, what float32 rounding of the two distances of every edge alone
    does to it (FLOAT32_DISTANCE)."""
    pos_gt, pos_pert = _f64(pos_gt), _f64(pos_pert)
    batch = np.asarray(batch, dtype=np.int64)
    a = _f64(np.asarray(alpha, dtype=np.float32))

    def part(row, col, score, weight, masked):
        row, col, score = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64), _f64(score).reshape(-1)
        dist = lambda p: np.sqrt(((p[row] - p[col]) ** 2).sum(axis=1))
        d_gt, d_pert = dist(pos_gt), dist(pos_pert)
        ae = a[batch[row]]
        amp = np.sqrt(ae) / np.sqrt(1.0 - ae)
        d_target = (d_gt - d_pert) * amp
        if masked:
            keep = d_pert <= cutoff
            row, col, score, d_target, d_gt, d_pert, amp = (x[keep] for x in (row, col, score, d_target, d_gt, d_pert, amp))
        diff = eq_term(pos_pert, row, col, score) - eq_term(pos_pert, row, col, d_target)
        # independent errors of up to FLOAT32_DISTANCE x d on both distances of every edge, added in quadrature over the edges
        # that touch the atom, move its target vector by tau; the loss w |diff|^2 then moves by 2 w |diff| tau
        var = np.zeros(pos_gt.shape[0])
        e2 = (FLOAT32_DISTANCE * amp) ** 2 * (d_gt ** 2 + d_pert ** 2)
        np.add.at(var, row, e2)
        np.add.at(var, col, e2)
        return weight * (diff * diff).sum(axis=1), 2.0 * weight * np.sqrt((diff * diff).sum(axis=1)) * np.sqrt(var)

    l_local, r_local = part(*local[:3], 5.0, False)
    l_global, r_global = part(*_type0(radius), 2.0, True)
    out = (l_global + l_local, l_global, l_local)
    return out + ((r_global + r_local, r_global, r_local),) if rounding else out


# Relative error bound of a float32 distance sqrt((dx dx + dy dy) + dz dz), u = 2^-24 per correctly rounded operation: u on each
# difference, 2 u + u on each square, + 2 u for the two sums of non-negative terms = 5 u under the root, which halves it, + u
# for the root itself (2 u where sqrtf is faithful, not correctly rounded): 4.5 u.
FLOAT32_DISTANCE = 4.5 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------- batch recipes
def dendrimer():
    """Centre with 4 neighbours, each with 3 children, each with 3 children: 53 atoms, raw single bonds (both directions).  The
    order-3 extension gives the centre 52 local edges."""
    pairs, nxt, level = [], 1, [0]
    for fan in (4, 3, 3):
        new = []
        for p in level:
            for _ in range(fan):
                pairs.append((p, nxt))
                new.append(nxt)
                nxt += 1
        level = new
    assert nxt == 53
    a = np.array([p[0] for p in pairs], dtype=np.int64)
    b = np.array([p[1] for p in pairs], dtype=np.int64)
    at = np.full(nxt, 6, dtype=np.int64)
    return at, np.concatenate([a, b]), np.concatenate([b, a]), np.ones(2 * a.shape[0], dtype=np.int64)


def _molecule(rng, n, raw_bonds):
    if raw_bonds or n <= 512:
        return synth.random_molecule(rng, n, raw_bonds=raw_bonds)
    # synth.random_molecule extends with dense n x n int64 products (seconds past 1,000 atoms); the sparse restatement
    # returns the same lists (tests/test_large_molecules_cpu.py)
    from large_mols import large_molecule
    return large_molecule(rng, n)


TAIL = (1, 2, 23)        # in every batch: idle lanes and ragged tails at every P
# (next to a largest molecule of 16 or 17 atoms the ragged one has 7: with 23 the batch would launch like "max23")
tail_of = lambda n: TAIL if n > 23 else (1, 2, 7)
UNFUSED_LAUNCH_SIZES = (16, 17, 64, 65, 128, 129, 256, 257, 512, 513)
# name -> (molecule sizes | "dendrimer", extend_order)
RECIPES = {"max%d" % n: ((n,) + tail_of(n), False) for n in UNFUSED_LAUNCH_SIZES}
RECIPES["max1025"] = ((1025,) + TAIL, False)
RECIPES["mixed"] = ((1, 2, 16, 32, 33, 64, 65, 128, 129, 256, 257, 512, 23), False)
RECIPES["small"] = ((32, 16, 9, 27) + TAIL, False)
RECIPES["many512"] = (tuple(1 + (7 * k + k // 40) % 40 for k in range(512)), False)
RECIPES["dendrimer"] = (("dendrimer", 31) + TAIL, True)
# the loss kernels' batch: 3 n around one and several rounds of 256 threads, plus the dendrimer (not an update batch)
LOSS_RECIPE = (("dendrimer", 1, 85, 86, 300), True)
_ALL = sorted(list(RECIPES) + ["loss"])


def recipe_sizes(name):
    return tuple(53 if n == "dendrimer" else n for n in (LOSS_RECIPE if name == "loss" else RECIPES[name])[0])


def _positions(seed, sizes):
    """Seeded normals x 3: pair distances have standard deviation 4.2 per axis, so part of every larger molecule lies beyond the
    cutoff of the rest.  A molecule with two atoms closer than MIN_PAIR is drawn again."""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        while True:
            p = (rng.standard_normal((n, 3)) * 3.0).astype(np.float32)
            d = p[:, None, :].astype(np.float64) - p[None, :, :]
            d2 = (d * d).sum(-1) + np.eye(n) * 1e9
            if d2.min() >= MIN_PAIR ** 2:
                break
        out.append(p)
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def make_batch(name):
    """dict: atom_type, bond_index, bond_type, batch, num_graphs, sizes, extend_order, pos (float32 [N, 3])."""
    spec, extend_order = LOSS_RECIPE if name == "loss" else RECIPES[name]
    seed = _ALL.index(name)
    rng = np.random.default_rng(1000 + seed)
    ats, rs, cs, ts, bs, sizes, off = [], [], [], [], [], [], 0
    for g, n in enumerate(spec):
        at, r, c, t = dendrimer() if n == "dendrimer" else _molecule(rng, n, extend_order)
        ats.append(at); rs.append(r + off); cs.append(c + off); ts.append(t)
        bs.append(np.full(at.shape[0], g, dtype=np.int64))
        sizes.append(at.shape[0])
        off += at.shape[0]
    b = dict(atom_type=np.concatenate(ats), bond_index=np.stack([np.concatenate(rs), np.concatenate(cs)]).astype(np.int64),
             bond_type=np.concatenate(ts).astype(np.int64), batch=np.concatenate(bs), num_graphs=len(spec), sizes=tuple(sizes),
             extend_order=extend_order)
    b["pos"] = _positions(2000 + seed, sizes)
    return b


# ------------------------------------------------------------------------------------------------- scores and settings
def draw_scores(name, n_local, n_radius, variant=0):
    """Seeded scores, not network outputs: local edges in (row, col) order, radius (type-0) edges in (col, row) order -- the
    orders of the device's static local list and of its destination-sorted edge list / radius rows."""
    rng = np.random.default_rng(3000 + 17 * _ALL.index(name) + variant)
    return rng.standard_normal(n_local).astype(np.float32), rng.standard_normal(n_radius).astype(np.float32)


def draw_noise(name, n, variant=0):
    rng = np.random.default_rng(4000 + 17 * _ALL.index(name) + variant)
    return rng.standard_normal((n, 3)).astype(np.float32)


# The full step.  step_size / sigma = 0.5 and |term| <= clip_local + w_global * clip = 5: the move is of the order of the
# positions (standard deviation 3), so one missing edge (|score| ~ 1) shifts its atom by ~0.5, a percent-level error.
# Limits against the norms of sums of k unit vectors x N(0, 1) scores, ~ sqrt(0.8 k) in the median: a local term sees every
# local edge twice (k ~ 2 x 8..20), a global term up to 2 x 32 radius edges; new coordinates have standard deviation ~3.5.
FULL = dict(sigma=0.7, step_size=0.35, noise_scale=0.5, w_global=0.3, clip=5.0, clip_local=3.5, clip_pos=4.0, use_global=1)
ISOLATING = {
    "no_global": dict(FULL, use_global=0),
    "no_local": dict(FULL),                                  # (run with the local scores zero)
    "no_clips": dict(FULL, clip_local=-1.0, clip=1e30),
    "no_step": dict(FULL, step_size=0.0),
}


def reference_edges(b):
    """The batch's edges from the oracle on the CPU: local (row, col) in (row, col) order and radius (row, col) in (col, row)
    order, as draw_scores counts them."""
    import torch
    from oracle import agdiff_oracle as O
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    n = b["atom_type"].shape[0]
    ei, et = O.extend_graph_order_radius(n, t(b["pos"]), t(b["bond_index"]), t(b["bond_type"]), t(b["batch"]), cutoff=CUTOFF,
                                         extend_order=b["extend_order"])
    ei, et = ei.numpy(), et.numpy()
    loc = et > 0
    rad = np.nonzero(et == 0)[0]
    rad = rad[np.lexsort((ei[0][rad], ei[1][rad]))]
    return (ei[0][loc], ei[1][loc]), (ei[0][rad], ei[1][rad])
