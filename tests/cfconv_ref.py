"""float64 restatement (NumPy) of agdiff_cfconv_node -- k_cfconv_quad and k_cfconv_node of csrc/nodeconv.hip: the two CFConvs of an
InteractionBlock with their filters from d-polynomials --, the seeded inputs and coefficient sets the tests write into the buffers
the kernels read, and the launcher's shape rules.  tests/test_cfconv_ref_cpu.py anchors it on the CPU,
tests/test_hip_cfconv_kernels.py runs the kernels against it on the GPU.

Test infrastructure only.  Coefficient sets are DATA here: C[192, K] per set in term order f = 8 g + j (phi_f = T_{8 g} T_j), so
that every k-tile of a set carries weight a wrong kernel cannot hide (a fitted network's high terms are zero to rounding or worth
1e-6 of the filter).  The row tables are data too: per-target radius counts, lengths, sources and scales are drawn, not built from
positions; only the static local tiles (quad_tgt, lt_ptr, lt_src, lt_type, lt_real) come from a BatchTopology.

    agg[i, c] = sum_{live local rows of i} s_c(row) P_{slot(type)}(len)[c] xs[src, c]
              + sum_{r < rad_cnt[i]} s_c(r) P_rad(len_r)[c] xs[src_r, c]

s_c: the conv1 scale of block k for channels 0..127 (plane 2 k), the conv2 scale for 128..191 (plane 2 k + 1);
P(d)[c] = sum_f C[c, f] phi_f(x), x = clamp(2 d / rc - 1, -1, 1).  The reference never looks at a dead row's values."""
import numpy as np

from agdiff_amd import _lib
from node_ref import draw

RS = _lib.DEFINES["AGDIFF_RAD_STRIDE"]           # rows reserved per target
CAP = _lib.RADIUS_CAP                            # most radius rows of a target (33)
TW = _lib.TILE
NCONV = 6                                        # blocks of the drugs / qm9 configs: 12 scale planes
MAX_CONVS = _lib.DEFINES["AGDIFF_MAX_CONVS"]
NAN = float("nan")
MODES = {"f32": 0, "bf16x3": 1, "f16x3": 2}
KT_PLANS = ((1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (4, 0), (4, 1), (4, 2), (4, 3))


# ------------------------------------------------------------------------------------------------- features
def cheb(n, x):
    """T_n(x) from the definition, float64."""
    return np.cos(n * np.arccos(np.clip(np.asarray(x, dtype=np.float64), -1.0, 1.0)))


def phi(x, K, short_from=None):
    """phi_f(x) = T_{8 g}(x) T_j(x), f = 8 g + j < K: [..., K] in term order.  short_from (a mutation): T_{8 g} is taken one step
    of eight short for g >= short_from."""
    x = np.asarray(x, dtype=np.float64)
    Tj = np.stack([cheb(j, x) for j in range(8)], axis=-1)
    out = []
    for g in range(K // 8):
        gg = g - 1 if short_from is not None and g >= short_from else g
        out.append(cheb(8 * gg, x)[..., None] * Tj)
    return np.concatenate(out, axis=-1)


def phi32(x, K):
    """The same in plain float32, by the three-term recurrences a float32 kernel would use (T_0..T_8 in steps of one, T_{8 g} in
    steps of eight).  cos(n arccos x) is no float32 algorithm: arccos alone is off by n 2^-24."""
    x = np.asarray(x, dtype=np.float32)
    T = [np.ones_like(x), x]
    for _ in range(2, 9):
        T.append(np.float32(2) * x * T[-1] - T[-2])
    G = [np.ones_like(x), T[8]]
    while len(G) < K // 8:
        G.append(np.float32(2) * T[8] * G[-1] - G[-2])
    return np.stack([G[f // 8] * T[f % 8] for f in range(K)], axis=-1)


def natural_columns(C, kt):
    """C[out, K] in term order -> the column order the kernels' packed blocks use (packing.poly_feature_order): the ONE place
    where that order is applied; pack_filter_sets below packs what this returns."""
    from agdiff_amd import packing
    return np.ascontiguousarray(np.asarray(C)[:, packing.poly_feature_order(kt)])


def length_x(d, cutoff):
    return np.clip(2.0 * np.asarray(d, dtype=np.float64) / float(cutoff) - 1.0, -1.0, 1.0)


# ------------------------------------------------------------------------------------------------- coefficient sets
def high_weight(mode):
    """The weight w of the terms a plan gives ONE hi x hi pass: POLY_EPS1[mode] w is a quarter of the mode's normwise gate."""
    from agdiff_amd import packing
    from helpers import TOL_NORM
    name = {v: k for k, v in MODES.items()}[mode]
    return TOL_NORM[name] / 4.0 / packing.POLY_EPS1[mode]


def one_pass_from(kt, plan):
    """First term that takes one pass under `plan` (None: plan 0)."""
    if plan == 0:
        return None
    return 16 if kt == 1 else 32 * plan


COEF_STD = 0.125
# Standard deviation of the coefficients of k-tile t: COEF_STD TILE_WEIGHT[t].  Equal weight in every k-tile is more than float32
# supports: the recurrences that make T_32 .. T_120 (the kernels' own, in float32 in every mode) are off by 1e-6 / 1.9e-6 / 3e-6 rms
# and 1.7e-5 / 3.7e-5 / 6.7e-5 at worst in k-tiles 1 / 2 / 3, against 2.9e-7 and 4.8e-6 in k-tile 0, and the plain-float32
# restatement of a set with equal weights misses the "f32" gate itself (normwise 4e-6 .. 1e-5 at 128 terms;
# tests/test_cfconv_ref_cpu.py asserts a quarter of it).  These weights bring a k-tile's worst feature error times its weight
# below k-tile 0's.  The top k-tile of a 128-term set still carries 2e-3 of the filter -- a thousand times what an accepted fit
# leaves there --, and a lost, swapped or mis-evaluated k-tile stays past ten times the loosest gate (asserted there too).
TILE_WEIGHT = (1.0, 1.0 / 16, 1.0 / 128, 1.0 / 512)
# ... and of the constant term (nn.2.bias sits there in a fitted set).  Without it a filter is a sum of 32 terms of random sign
# and the plain-float32 restatement sits AT a quarter of the "f32" gates (normwise 1.24e-6, element-wise 5.1e-4 at worst).
BIAS_STD = 0.75


def _draw_set(tag, kt, plan, mode):
    """One set C[192, 32 kt] (float32 values).  Plan 0: the terms of k-tile t N(0, COEF_STD TILE_WEIGHT[t]).
    Plans 1..3: the full-pass terms likewise; every one-pass k-tile (at one k-tile: its terms 16..31) has ONE non-zero term per
    channel, all of one magnitude, sized so that packing.poly_high_weight of the set is high_weight(mode)."""
    from agdiff_amd import packing
    K = 32 * kt
    C = draw(tag, (192, K), COEF_STD).astype(np.float64) * np.repeat(TILE_WEIGHT[:kt], 32)[None, :]
    C[:, 0] = draw(tag + ":bias", (192,), BIAS_STD)
    hi = one_pass_from(kt, plan)
    if hi is not None:
        C[:, hi:] = 0.0
        groups = [(hi, K)] if kt == 1 else [(32 * t, 32 * t + 32) for t in range(plan, kt)]
        pick = draw(tag + ":pick", (192, len(groups), 2))
        for gi, (a, b) in enumerate(groups):
            f = a + (np.abs(pick[:, gi, 0]) * 1e4).astype(np.int64) % (b - a)
            C[np.arange(192), f] = np.where(pick[:, gi, 1] < 0, -1.0, 1.0)
        w = high_weight(mode)
        for _ in range(3):
            C[:, hi:] *= w / packing.poly_high_weight(natural_columns(C, kt), kt, hi)
    return C.astype(np.float32).astype(np.float64)


def coefficient_sets(name, kt, plan, mode, num_slots, k):
    """(C_rad [192, K], C_typed [num_slots, 192, K], S) of conv block k: every set and every block its own draw; plan-0 sets do not
    depend on the mode.  The device holds 2^S times these (pack_filter_sets), conv[k].filt_poly_unscale = 2^-S, S != 0."""
    tag = "coef:%s:kt%d:p%d:m%d:k%d" % (name, kt, plan, mode if plan else 0, k)
    rad = _draw_set(tag + ":rad", kt, plan, mode)
    typed = np.stack([_draw_set(tag + ":slot%d" % s, kt, plan, mode) for s in range(num_slots)]) if num_slots else np.zeros((0, 192, 32 * kt))
    return rad, typed, 7 + k % 3


def pack_filter_sets(C, kt, plan, mode, S):
    """One set as PackedParams._pack_filter_sets packs it: pack_blocks(c 2^S, mode) in natural column order, mix_units under plan 1."""
    from agdiff_amd import packing
    v = packing.pack_blocks(natural_columns(C, kt) * 2.0 ** S, mode=mode)
    return packing.mix_units(v, kt) if plan == 1 else v


# ------------------------------------------------------------------------------------------------- batches
def _tree(rng, n, types, off):
    """A random tree over n atoms (parent among the previous three), bond types from `types`: both directions."""
    a = np.arange(1, n)
    p = np.array([rng.integers(max(0, i - 3), i) for i in a], dtype=np.int64)
    ty = rng.choice(np.asarray(types), size=a.shape[0])
    return np.concatenate([p, a]) + off, np.concatenate([a, p]) + off, np.concatenate([ty, ty])


ROWS_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 33, 34, 35, 64)
SLOTTED = (1, 2, 3, 4, 5, 6, 7)
UNSLOTTED = 9


def make_batch(name):
    """dict(atom_type, bond_index, bond_type, batch, num_graphs, extend_order).
    rows:  three rounds of ROWS_SIZES (615 atoms), order extension over bonds of types 1, 2, 3, 12; in the last round the 4-,
           8- and 64-atom molecules have no bond at all: quads without a local tile.
    hub:   step_ref.dendrimer() (a centre with 52 local in-edges under order extension) and a 9-atom tree.
    types: four trees of 24..27 atoms with bonds of the seven SLOTTED types and of UNSLOTTED, no extension.
    qN:    N molecules of 4 atoms -- N quads --, every fifth without bonds, raw bonds of types 1, 2."""
    import step_ref
    rng = np.random.default_rng(sum(map(ord, name)) + 9000)
    rs, cs, ts, sizes, off, extend = [], [], [], [], 0, False

    def add(n, types, bonded=True):
        nonlocal off
        if bonded and n > 1:
            r, c, t = _tree(rng, n, types, off)
            rs.append(r); cs.append(c); ts.append(t)
        sizes.append(n)
        off += n
    if name == "rows":
        extend = True
        for rnd in range(3):
            for n in ROWS_SIZES:
                add(n, (1, 2, 3, 12), bonded=not (rnd == 2 and n in (4, 8, 64)))
    elif name == "hub":
        extend = True
        _, r, c, t = step_ref.dendrimer()
        rs.append(r); cs.append(c); ts.append(t)
        sizes.append(53)
        off = 53
        add(9, (1, 2))
    elif name == "types":
        for n in (24, 25, 26, 27):
            add(n, SLOTTED + (UNSLOTTED,))
    else:
        for m in range(int(name[1:])):
            add(4, (1, 2), bonded=m % 5 != 3)
    cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, dtype=np.int64)
    return dict(atom_type=np.full(off, 6, dtype=np.int64), bond_index=np.stack([cat(rs), cat(cs)]), bond_type=cat(ts),
                batch=np.repeat(np.arange(len(sizes)), sizes), num_graphs=len(sizes), extend_order=extend)


def topology(name, group_targets=4, device="cpu"):
    from agdiff_amd.topology import BatchTopology
    b = make_batch(name)
    return BatchTopology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], num_graphs=b["num_graphs"],
                         extend_order=b["extend_order"], device=device, group_targets=group_targets)


def view(topo):
    """The host-side arrays of a BatchTopology the tables and the reference need (int64)."""
    g = lambda x: x.cpu().numpy().astype(np.int64)
    gp = g(topo.graph_ptr)
    return dict(N=topo.N, GT=topo.group_targets, Q=topo.Q, T=topo.T, quad_tgt=g(topo.quad_tgt).reshape(-1, 4), lt_ptr=g(topo.lt_ptr),
                lt_src=g(topo.lt_src), lt_type=g(topo.lt_type), lt_real=np.asarray(topo.lt_real, dtype=bool), graph_ptr=gp,
                mol=np.repeat(np.arange(gp.shape[0] - 1), np.diff(gp)),
                wg_ptr=None if topo.quad_wg_ptr is None else g(topo.quad_wg_ptr))


# ------------------------------------------------------------------------------------------------- row tables
CNT_CHOICES = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, CAP)
QUAD_PATTERNS = ((0, 0, 0, 0), (0, 1, CAP, 16), (17, 0, 0, 0))
DECOYS = (0.0, 0.3, 2.0, 1e30)          # x rc, except the last


def _r16(c):
    return (c + TW - 1) // TW * TW


def tables(tv, name, cutoff, slotted=None):
    """The buffers of one batch as DATA (dict).  Host invariants kept, so that a wrong read is a wrong number and never a fault:
    every source anywhere is an atom of the row's own molecule; rows [cnt, roundup16(cnt)) of a target have scale 0 and a finite
    length (what the front kernel writes; k_cfconv_node does not mask them); rows from there to the end of the quad's last
    four-row tile (k_cfconv_quad walks max over the quad of ceil(cnt / 4) tiles) carry NaN scales and the finite DECOYS as lengths;
    rows past those carry NaN lengths and scales.  Pad rows of local tiles have scale 0, tiles of a type outside `slotted` NaN
    scales.  Live rows include lengths 0, rc, and > rc with scale 0.
      rad_cnt [N], rad_src [N, RS], rad_len [N, RS], r_scale [12, N, RS], lt_len [16 T], lt_scale [12, 16 T], xs [N, 192]: device
      r_raw / l_raw: every row's drawn scale (what a kernel that counted a dead row would most plausibly multiply by)
      lt_tgt [16 T]: the target a local row adds to (-1: none), lt_live [16 T]: real row of a slotted type"""
    N, Q, T, GT = tv["N"], tv["Q"], tv["T"], tv["GT"]
    rc = float(cutoff)
    gp, mol, qt = tv["graph_ptr"], tv["mol"], tv["quad_tgt"]
    rng = np.random.default_rng(sum(map(ord, name)) + 100 * GT)
    nmol = (gp[1:] - gp[:-1])[mol]
    cnt = np.minimum(rng.choice(np.asarray(CNT_CHOICES), size=N), nmol - 1)
    full = np.nonzero((qt >= 0).all(axis=1) & (nmol[np.maximum(qt[:, 0], 0)] >= CAP + 1))[0]
    for qi, pat in zip(full[1:], QUAD_PATTERNS):
        cnt[qt[qi]] = pat
    if name.startswith("q"):                     # 4-atom molecules: every fifth (the bondless ones) without radius rows either
        cnt[(mol % 5) == 3] = 0
    src = gp[mol][:, None] + rng.integers(0, 1 << 30, size=(N, RS)) % nmol[:, None]
    r = np.arange(RS)[None, :]
    live = r < cnt[:, None]
    for i in np.nonzero(cnt > 0)[0]:             # live rows: distinct ascending sources other than the target, as radius_graph gives
        others = np.setdiff1d(np.arange(gp[mol[i]], gp[mol[i] + 1]), [i])
        src[i, :cnt[i]] = np.sort(rng.choice(others, size=cnt[i], replace=False))
    rlen = rng.uniform(0.03, 0.98, size=(N, RS)) * rc
    raw = rng.uniform(0.1, 1.0, size=(2 * NCONV, N, RS))
    zero = np.zeros((N, RS), dtype=bool)         # live rows beyond the cutoff: scale exactly 0
    big = np.nonzero(cnt >= 4)[0]
    rlen[big[0::3], 0] = 0.0
    rlen[big[1::3], 1] = rc
    rlen[big[2::3], 2] = 1.5 * rc
    zero[big[2::3], 2] = True
    # rows a quad walks: 4 nR per target, nR = max over the quad of ceil(cnt / 4)
    walked = np.zeros(N, dtype=np.int64)
    nR = (np.where(qt >= 0, cnt[np.maximum(qt, 0)], 0).max(axis=1) + 3) // 4
    walked[qt[qt >= 0]] = np.repeat(4 * nR, 4).reshape(-1, 4)[qt >= 0]
    r16 = _r16(cnt)[:, None]
    decoy = (r >= r16) & (r < walked[:, None])
    dec = np.asarray([DECOYS[0] * rc, DECOYS[1] * rc, DECOYS[2] * rc, DECOYS[3]])
    rlen = np.where(decoy, dec[(r + np.arange(N)[:, None]) % 4], rlen)
    rlen = np.where((r >= r16) & ~decoy, NAN, rlen)
    scale = np.where(live & ~zero, raw, np.where(r < r16, 0.0, NAN))
    # local tiles
    RT = 16 // GT
    trow = np.arange(16 * T)
    tile_quad = np.repeat(np.arange(Q), np.diff(tv["lt_ptr"]))
    lt_tgt = qt[tile_quad[trow // 16], (trow % 16) // RT] if T else np.zeros(0, dtype=np.int64)
    real = tv["lt_real"]
    typ = tv["lt_type"]
    has_slot = np.ones(16 * T, dtype=bool) if slotted is None else np.isin(typ, np.asarray(slotted))
    llen = rng.uniform(0.03, 0.98, size=16 * T) * rc
    l_raw = rng.uniform(0.1, 1.0, size=(2 * NCONV, 16 * T))
    lzero = np.zeros(16 * T, dtype=bool)
    lr = np.nonzero(real & has_slot)[0]
    llen[lr[0::7]] = 0.0
    llen[lr[1::7]] = rc
    llen[lr[2::7]] = 1.25 * rc
    lzero[lr[2::7]] = True
    lscale = np.where(~has_slot, NAN, np.where(real & ~lzero, l_raw, 0.0))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(rad_cnt=cnt, rad_src=src, rad_len=f32(rlen), r_scale=f32(scale), r_raw=f32(np.where(zero, 0.0, raw)), lt_len=f32(llen),
                lt_scale=f32(lscale), l_raw=f32(np.where(lzero, 0.0, l_raw)), lt_tgt=lt_tgt, lt_live=real & has_slot & (lt_tgt >= 0),
                xs=draw("xs:" + name, (N, 192)), walked=walked, nR=nR)


# ------------------------------------------------------------------------------------------------- the reference
def _rows_of(tv, tb, type_slot, mutate):
    """The live rows as flat lists: (target, source, length, plane-row index for the scale lookup, set) for local rows (set = slot)
    and radius rows (set = -1).  Scales are looked up in the RAW draws for rows a mutation adds, in the device table for live
    rows (identical there)."""
    cnt = tb["rad_cnt"].copy()
    m = dict(mutate)
    if "radius_last_dropped" in m:
        cnt[m["radius_last_dropped"]] -= 1
    if "radius_cnt_counted" in m:
        cnt[m["radius_cnt_counted"]] += 1
    ii, rr = np.nonzero(np.arange(RS)[None, :] < cnt[:, None])
    if "row33_dropped" in m:
        keep = ~((ii == m["row33_dropped"]) & (rr == CAP - 1))
        ii, rr = ii[keep], rr[keep]
    rad = dict(tgt=ii, src=tb["rad_src"][ii, rr], len=tb["rad_len"][ii, rr].astype(np.float64), at=(ii, rr), set=np.full(ii.shape[0], -1))
    live = tb["lt_live"].copy()
    slot = np.asarray(type_slot)[tv["lt_type"]] if tv["T"] else np.zeros(0, dtype=np.int64)
    if "unslotted_counted" in m:
        live = live | (tv["lt_real"] & (tb["lt_tgt"] >= 0))
    live = live & ((slot >= 0) | ("unslotted_counted" in m))
    if "pad_local_counted" in m:
        live[m["pad_local_counted"]] = True
    e = np.nonzero(live)[0]
    s = slot[e].copy()
    if "neighbour_slot" in m:
        tile, nslots = m["neighbour_slot"]
        s[e // 16 == tile] = (s[e // 16 == tile] + 1) % nslots
    loc = dict(tgt=tb["lt_tgt"][e], src=tv["lt_src"][e], len=tb["lt_len"][e].astype(np.float64), at=(e,), set=s)
    return loc, rad


def cfconv(coef_rad, coef_typed, type_slot, rows, xs, cutoff, k, mutate=(), dtype=np.float64):
    """agg [N, 192] of block k.  rows = (view(topo), tables(...)).  dtype float32: the same sums in plain float32 in the kernels'
    row order (a target's local rows by tile, then its radius rows by row index), features by phi32.
    mutate: a dict of the wrong kernels tests/test_cfconv_ref_cpu.py lists (name -> parameter)."""
    tv, tb = rows
    m = dict(mutate)
    f32 = dtype == np.float32
    K = coef_rad.shape[1]
    N = tv["N"]
    kk = k + 1 if "next_block_scale" in m else k
    p1, p2 = (2 * kk + 1, 2 * kk) if "conv_scales_swapped" in m else (2 * kk, 2 * kk + 1)
    loc, rad = _rows_of(tv, tb, type_slot, m)
    xs = np.asarray(xs, dtype=dtype)
    agg = np.zeros((N, 192), dtype=dtype)
    feats = (lambda d: phi32(length_x(d, cutoff).astype(np.float32), K)) if f32 else \
        (lambda d: phi(length_x(d, cutoff), K, m.get("T8g_short")))
    for part, raw in ((loc, tb["l_raw"]), (rad, tb["r_raw"])):
        n = part["tgt"].shape[0]
        if not n:
            continue
        s = np.empty((n, 192), dtype=dtype)
        s[:, :128] = raw[p1][part["at"]][:, None]
        s[:, 128:] = raw[p2][part["at"]][:, None]
        ph = feats(part["len"])
        P = np.empty((n, 192), dtype=dtype)
        for st in np.unique(part["set"]):
            C = coef_rad if st < 0 else coef_typed[st]
            sel = part["set"] == st
            P[sel] = ph[sel] @ np.asarray(C, dtype=dtype).T
        contrib = s * P * xs[part["src"]]
        if not f32:
            np.add.at(agg, part["tgt"], contrib)
        else:                                    # row order: the p-th row of every target at once
            order = np.argsort(part["tgt"], kind="stable")
            tg = part["tgt"][order]
            rank = np.arange(n) - np.searchsorted(tg, tg)
            for p in range(int(rank.max()) + 1):
                sel = order[rank == p]
                agg[part["tgt"][sel]] += contrib[sel]
    if "fourth_gets_third" in m:
        q = tv["quad_tgt"][m["fourth_gets_third"]]
        agg[q[3]] = agg[q[2]]
    if "quads_skipped" in m:
        q = tv["quad_tgt"][np.asarray(m["quads_skipped"])].reshape(-1)
        agg[q[q >= 0]] = 0.0
    if "no_unscale" in m:
        agg = agg * dtype(2.0 ** m["no_unscale"])
    return agg


# ------------------------------------------------------------------------------------------------- launch shapes
FOUR_MIN_QUADS = 8192    # agdiff_params_t.tune_cfconv_four_min_quads
CUS = 256
LDS_BYTES = 160 * 1024


def launch(Q, kt, tuning=None, group_targets=4, num_slots=0, have_ranges=True):
    """agdiff_cfconv_node's choices for Q quads at kt k-tiles: dict(kernel = "quad" | "node", four, waves = 16 / 8 / 12 per
    workgroup, grid = min(256, ceil(Q / waves)), per_wg quads of a workgroup without ranges, remap (the XCD remap: grids divisible by
    8), ranges (k_cfconv_quad on a grid of 256 with topo.quad_wg_ptr), lds_slots typed sets in LDS, last = quads of the last
    workgroup without ranges (<= 0: none), bits = the variant word of a launch with local tiles."""
    tn = dict(tuning or {})
    four_min = int(tn.get("cfconv_four_min_quads", 0)) or FOUR_MIN_QUADS
    four = kt == 1 and four_min >= 0 and Q >= four_min
    waves = 16 if four else 8 if kt >= 3 else 12
    grid = min(CUS, (Q + waves - 1) // waves)
    quad = group_targets == 4 and int(tn.get("cfconv_quad_tiles", 0)) >= 0
    max_sets = LDS_BYTES // (12 * kt * 2048)
    cap = int(tn.get("poly_lds_sets", 0))
    if 0 < cap < max_sets:
        max_sets = cap
    lds_slots = min(num_slots, max_sets - 1)
    per_wg = (Q + grid - 1) // grid
    D = _lib.DEFINES
    bits = D["AGDIFF_VAR_CFCONV_NODE"] | (D["AGDIFF_VAR_CFCONV_NODE_LOCAL"] if num_slots else 0) | \
        (D["AGDIFF_VAR_POLY_L2_SETS"] if lds_slots < num_slots else 0) | (D["AGDIFF_VAR_CFCONV_NODE_FOUR"] if four else 0) | \
        (D["AGDIFF_VAR_CFCONV_NODE_QUAD"] if quad else 0)
    return dict(kernel="quad" if quad else "node", four=four, waves=waves, grid=grid, per_wg=per_wg, remap=grid % 8 == 0,
                ranges=quad and grid == CUS and have_ranges, lds_slots=lds_slots, last=Q - (grid - 1) * per_wg, bits=bits)


def workgroup_of_block(block, grid):
    """The workgroup index a hardware block takes (blocks go round-robin over 8 XCDs: a workgroup's neighbours share an L2)."""
    return (block % 8) * (grid // 8) + block // 8 if grid % 8 == 0 else block
