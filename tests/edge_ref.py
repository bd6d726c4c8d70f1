"""float64 restatement of the per-edge producers of csrc/edge.hip and csrc/common.hpp -- the distance-weighting scale lw(d) C(d)
(cf_dist_weight x cf_envelope: k_edge_scales, k_rad_scales, the fill passes of k_graph / k_lg_thr, both forms of k_sampler_front),
the MLP edge encoder (k_edge_encoder) and the Gaussian one (k_edge_gaussian) --, the case data the tests run them on, and the wrong
kernels (`mutate=`) the comparison must catch.  tests/test_edge_ref_cpu.py anchors it on the CPU, tests/test_hip_edge_kernels.py runs
the kernels against it on the GPU.  Test infrastructure only.

The twelve distance-weighting networks (one per scale plane of a six-block config, plane 2 k = conv1 and 2 k + 1 = conv2 of block
k) are DATA: layer1.weight = +-2^j, layer1.bias = -w1 kink (both exact in float32), so every kink sits at a float32 value the
tests choose, and the lengths are those kinks with their float32 neighbours.  They go into a state dict; agdiff_amd.packing builds
the segment tables and the union table from it, the reference evaluates the network itself."""
import numpy as np
import torch

from pair_head_ref import PAYLOAD_BITS, scatter_indices  # noqa: F401  (re-exported: the encoder cases' scatter)

RC = 10.0                       # cutoff of both configs
NPLANES = 12
RC32 = np.float32(RC)
NAN = float("nan")
TAIL_PLANE = 8
# what each plane is there for (asserted in tests/test_edge_ref_cpu.py)
PLANES = {0: "no kink (w1 = 0 everywhere)", 1: "32 kinks inside (0, 0.6 rc): the s == 31 fix-up runs on every longer length",
          2: "31 kinks inside (0, rc), one beyond", 3: "all kinks negative", 4: "all kinks beyond rc",
          5: "two pairs of coinciding kinks", 6: "two kinks shared with plane 1", 7: "a kink at exactly 0 and one at exactly rc",
          8: "pre-activation from -40 up to +36 and down to -140, past the sigmoid's clamp at -87.3 (dyadic kinks, integer slopes: the table is exact)",
          9: "32 kinks inside (0, rc)", 10: "32 kinks inside (0, rc)", 11: "32 kinks inside (0, rc)"}


# ------------------------------------------------------------------------------------------------- the networks
def _grid(p, wide):
    """32 ascending float32 values inside (0, rc): 10 (i + 1) / 33, shifted by 0.01 (p + 1) in the wide set (distinct per plane)"""
    return (RC * (np.arange(32) + 1.0) / 33.0 + (0.01 * (p + 1) if wide else 0.0)).astype(np.float32)


def plane_kinks(p, wide=True):
    """float32 [32] kinks of plane p in unit order (not sorted), or None for plane 0"""
    g = _grid(p, wide)
    if p == 0:
        return None
    if p == 1:              # (narrow: the shared grid itself, or the union would pass 64 kinks)
        return (0.6 * g.astype(np.float64)).astype(np.float32) if wide else g
    if p == 2:
        g[31] = np.float32(1.25 * RC)
    elif p == 3:
        g = -g
    elif p == 4:
        g = (g.astype(np.float64) + RC).astype(np.float32)
    elif p == 5:
        g[7], g[20] = g[6], g[19]
    elif p == 6:
        one = plane_kinks(1, wide)
        g[3], g[15] = one[9], one[30]
    elif p == 7:
        g[0], g[31] = np.float32(0.0), RC32
    elif p == TAIL_PLANE:
        inside = 0.5 * (np.arange(16) + 1.0)
        g = np.concatenate([inside, -inside]).astype(np.float32)
    return g


def _network(p, wide):
    """(w1, b1, w2, b2) float32 of plane p.  Slopes change by delta_i = w2_i |w1_i| = +-(1 .. 1.75) at kink i, alternating in sign
    along the sorted kinks, so the pre-activation zigzags with slopes of order 1 and stays of order 1 itself."""
    t = plane_kinks(p, wide)
    i = np.arange(32)
    if p == 0:
        b1 = np.where(i % 2 == 0, 0.5, -0.5) * (1.0 + i / 32.0)
        w2 = np.where(i % 4 < 2, 0.25, -0.125)
        return np.zeros(32, np.float32), b1.astype(np.float32), w2.astype(np.float32), np.float32(0.3)
    if p == TAIL_PLANE:
        w1 = np.where(t > 0, 1.0, -1.0)
        target = np.where(t[:16] < 5.0, 16.0, -32.0) + 8.0 * (-1.0) ** i[:16]      # slope after inside kink i
        delta = np.concatenate([[target[0]], np.diff(target), np.ones(16)])
        b2 = -40.0
    else:
        rank = np.argsort(np.argsort(t, kind="stable"), kind="stable")              # position of unit i among the sorted kinks
        # slope after the kink of rank r, less the slope before the first kink: T_{r+1} = -+(0.5 .. 0.875), constant over four
        # ranks.  Units of rank 1, 2 mod 4 have w1 < 0 (active BELOW their kink): each such pair's changes cancel, so the slope
        # before the first kink is 0 -- in plane 4, where [0, rc] lies before every kink, rank 0 is negative too and it is T_1.
        m = np.arange(33)
        T = np.where(m == 0, 0.0, (-1.0) ** m * (0.5 + 0.125 * ((m // 4 + p) % 4)))
        delta = (T[1:] - T[:-1])[rank]
        negative = np.isin(rank % 4, (1, 2)) | ((p == 4) & (rank == 0))
        w1 = np.where(negative, -1.0, 1.0) * 2.0 ** ((i + p) % 5 - 2)
        b2 = 0.0
    w2 = delta / np.abs(w1)
    b1 = -w1 * t.astype(np.float64)
    w1, b1, w2 = (x.astype(np.float32) for x in (w1, b1, w2))
    if p != TAIL_PLANE:         # centre the pre-activation over [0, rc] (a float32 number like any other)
        d = np.linspace(0.0, RC, 2001)
        b2 = -float(np.median(preact64((w1, b1, w2, np.float32(0.0)), d)))
    return w1, b1, w2, np.float32(b2)


def networks(which="wide"):
    """[12] x (w1, b1, w2, b2).  "wide": every plane's kinks its own (dist_union_table: K = 512); "narrow": one grid shared by
    the planes (K <= 64)."""
    return [_network(p, which == "wide") for p in range(NPLANES)]


def plane_keys(p):
    c = "encoder_global.interactions.%d.conv%d.distance_weighting." % (p // 2, p % 2 + 1)
    return c + "layer1.weight", c + "layer1.bias", c + "layer2.weight", c + "layer2.bias"


def with_networks(sd, nets):
    """A copy of state dict `sd` (six blocks) with the twelve networks in place, under both names of every tensor"""
    from agdiff_amd import synth
    new = {}
    for p, (w1, b1, w2, b2) in enumerate(nets):
        k = plane_keys(p)
        new[k[0]], new[k[1]] = torch.from_numpy(w1).view(32, 1), torch.from_numpy(b1)
        new[k[2]], new[k[3]] = torch.from_numpy(w2).view(1, 32), torch.from_numpy(np.asarray([b2], dtype=np.float32))
    out, hit = {}, set()
    for k, v in sd.items():
        c = synth.canonical_key(k)
        out[k] = new[c].clone() if c in new else v
        hit.add(c)
    assert set(new) <= hit
    return out


def segment_tables(nets):
    """float64 [12, 100] from packing.dist_segments, and the same rounded to float32 (what the kernels read)"""
    from agdiff_amd import packing
    tabs = np.stack([packing.dist_segments(w1, b1, w2, float(b2)) for (w1, b1, w2, b2) in nets])
    return tabs, tabs.astype(np.float32)


def union_table(nets, cutoff=RC):
    from agdiff_amd import packing
    tabs = segment_tables(nets)[0]
    return packing.dist_union_table([np.concatenate([tabs[2 * k], tabs[2 * k + 1]]) for k in range(NPLANES // 2)], cutoff)


# ------------------------------------------------------------------------------------------------- the reference
def preact64(net, d):
    """layer2(relu(layer1(d))) in float64, from the network itself"""
    w1, b1, w2, b2 = (np.asarray(x, dtype=np.float64) for x in net)
    d = np.asarray(d, dtype=np.float64)
    return np.maximum(d[..., None] * w1 + b1, 0.0) @ w2 + b2


def envelope64(d, cutoff, smooth, mutate=()):
    """C(d) as schnet.py:140-146 / oracle.agdiff_oracle.cfconv write it.  mutate: "envelope_lt", "smooth_for_gaussian"."""
    d = np.asarray(d, dtype=np.float64)
    rc = float(cutoff)
    if smooth or "smooth_for_gaussian" in mutate:
        C = 0.5 * (np.cos(d * np.pi / rc) + 1.0)
    else:
        C = np.exp(-((d - rc) ** 2) / (2.0 * rc * rc))
    inside = (d < rc) if "envelope_lt" in mutate else (d <= rc)
    return C * inside * (d >= 0.0)


def scales64(nets, d, cutoff, smooth):
    """[12, n] float64: sigmoid(layer2(relu(layer1(d)))) C(d) of every plane"""
    C = envelope64(d, cutoff, smooth)
    return np.stack([C / (1.0 + np.exp(-preact64(net, d))) for net in nets])


def table_scales(tabs, d, cutoff, smooth, dtype=np.float64, mutate=()):
    """[12, n]: the scales from the segment tables [12, 100], as cf_dist_weight / cf_envelope evaluate them: s = number of kinks
    <= d, sigmoid(alpha_s d + beta_s) C(d).  dtype float32: tables and lengths in float32, ONE rounding for the FMA, for the sigmoid,
    for the envelope and for the product (what a correctly rounding float32 kernel gives).
    mutate: "segment_low", "segment_high", "no_fixup" (s stops at 31), "alpha_beta_swapped", "conv_planes_swapped", "envelope_lt",
    "smooth_for_gaussian"."""
    f32 = dtype == np.float32
    tabs = np.asarray(tabs, dtype=np.float32 if f32 else np.float64)
    d = np.asarray(d, dtype=np.float32 if f32 else np.float64)
    rnd = (lambda x: x.astype(np.float32).astype(np.float64)) if f32 else (lambda x: x)
    C = rnd(envelope64(d, np.float32(cutoff) if f32 else cutoff, smooth, mutate))
    out = []
    for tab in tabs:
        s = (tab[None, :32] <= d[:, None]).sum(axis=1)
        if "segment_low" in mutate:
            s = np.maximum(s - 1, 0)
        if "segment_high" in mutate:
            s = np.minimum(s + 1, 32)
        if "no_fixup" in mutate:
            s = np.minimum(s, 31)
        a, b = tab[32:65].astype(np.float64), tab[65:98].astype(np.float64)
        if "alpha_beta_swapped" in mutate:
            a, b = b, a
        f = rnd(a[s] * d.astype(np.float64) + b[s])
        out.append(rnd(rnd(1.0 / (1.0 + np.exp(-f))) * C))
    out = np.stack(out)
    if "conv_planes_swapped" in mutate:
        out = out.reshape(-1, 2, d.shape[0])[:, ::-1].reshape(out.shape)
    return out


def union_scales(table, K, n, d, cutoff, smooth):
    """[n, len(d)] float64 from packing.dist_union_table's table: u = number of union kinks <= d, line (u, cc)"""
    table = np.asarray(table, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    u = (table[None, :K] <= d[:, None]).sum(axis=1)
    C = envelope64(d, cutoff, smooth)
    return np.stack([C / (1.0 + np.exp(-(table[K + (u * n + cc) * 2] * d + table[K + (u * n + cc) * 2 + 1]))) for cc in range(n)])


# ------------------------------------------------------------------------------------------------- lengths
def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def all_kinks(which="wide"):
    return np.unique(np.concatenate([plane_kinks(p, which == "wide") for p in range(1, NPLANES)]))


def lengths(which="wide", sweep=97):
    """float32, sorted, unique up to the sign of zero: every kink and both of its float32 neighbours; 0 and -0.0; rc, its two
    neighbours, 1.5 rc, 100 rc; a log-spaced sweep from 1e-3 to rc.  (A negative kink brings negative lengths: C = 0 there.)"""
    k = all_kinks(which)
    nb = np.concatenate([k, np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-np.inf))])
    special = np.concatenate([[RC32, np.nextafter(RC32, np.float32(np.inf)), np.nextafter(RC32, np.float32(-np.inf))],
                              _f32([1.5 * RC, 100.0 * RC])])
    v = np.unique(np.concatenate([nb, special, _f32(np.logspace(-3.0, 1.0, sweep))]))
    v = v[v != 0]
    at = int(np.searchsorted(v, 0.0))
    return np.concatenate([v[:at], np.asarray([-0.0, 0.0], dtype=np.float32), v[at:]]).astype(np.float32)


def mid_segment_lengths(which="wide"):
    """float32: per plane, the midpoints between neighbouring distinct kinks inside [0, rc] -- where a segment off by one is a
    different line at a distance from the kink (AT a kink it cannot show: the function is continuous there)"""
    out = []
    for p in range(1, NPLANES):
        k = np.unique(plane_kinks(p, which == "wide")).astype(np.float64)
        k = k[(k >= 0) & (k <= RC)]
        out.append(0.5 * (k[1:] + k[:-1]))
    return np.unique(_f32(np.concatenate(out)))


# ------------------------------------------------------------------------------------------------- radius rows (k_rad_scales)
RAD_COUNTS = (0, 1, 15, 16, 17, 32, 33)


def r16(c):
    return (np.asarray(c) + 15) // 16 * 16


def rad_expected(cnt, rad_len, scales, RS, mutate=()):
    """What k_rad_scales leaves in r_scale [12, N, RS] pre-filled with the payload, as (values float64 with NaN where the payload
    stays, written mask [N, RS]): live rows the scales [12, N, RS] of their lengths, rows [cnt, roundup16(cnt)) exactly 0.
    mutate "pad_rows_not_zeroed": those rows keep the payload."""
    cnt = np.asarray(cnt)
    r = np.arange(RS)[None, :]
    live, pad = r < cnt[:, None], (r >= cnt[:, None]) & (r < r16(cnt)[:, None])
    val = np.where(live[None], scales, np.where(pad[None], 0.0, NAN))
    written = live | pad
    if "pad_rows_not_zeroed" in mutate:
        val = np.where(pad[None], NAN, val)
        written = live
    return val, written


# ------------------------------------------------------------------------------------------------- encoder cases
E_COUNTS = (1, 15, 16, 17, 33)
# agdiff_edge_encoder caps its grid at 256 workgroups of 16 waves: 4096 tiles per round.  4097 tiles = 65,537 edges is the
# smallest count at which a wave takes a SECOND tile (the persistent loop's stride).
E_ROUNDS = 16 * 4096 + 1
TYPE_POOL = (0, 1, 2, 3, 99, 12, 23, 24, 50)
FE_SCALE = 4.0                   # the second weight set: feature_expansion x 4 -- first-GELU arguments to +-14 inside the cutoff


def edge_types(n):
    """int32 [n] from TYPE_POOL: edge 0 has type 0, edge 1 type 99, every tile mixes at least four types"""
    e = np.arange(n)
    return np.asarray(TYPE_POOL, dtype=np.int32)[(e * 4 + e // 16) % len(TYPE_POOL)]


def edge_lengths(n):
    """float32 [n]: the wide set's lengths in a fixed shuffled order (100 rc, 0 and a kink's neighbour among the first 15), then a
    log sweep from 1e-3 to rc"""
    pool = lengths("wide")
    pool = pool[np.random.default_rng(71).permutation(pool.size)]
    first = _f32([0.37 * RC, 100.0 * RC, 0.0, RC, 1.5 * RC])
    pool = np.concatenate([first, pool])
    if n <= pool.size:
        return pool[:n].copy()
    return np.concatenate([pool, _f32(np.logspace(-3.0, 1.0, n - pool.size))])


def near(length):
    """rows judged together: |d| <= 1.5 rc.  The rows at 100 rc are a thousand times larger and are judged on their own, or the
    normwise figure of every other row would be measured against them."""
    return np.abs(np.asarray(length, dtype=np.float64)) <= 1.5 * RC


def scaled_feature_expansion(sd, factor=FE_SCALE):
    from agdiff_amd import synth
    keys = ("edge_encoder_global.feature_expansion.weight", "edge_encoder_global.feature_expansion.bias")
    return {k: (v * factor if synth.canonical_key(k) in keys else v) for k, v in sd.items()}


def first_gelu_arguments(sd, length):
    w = sd["edge_encoder_global.feature_expansion.weight"].double().numpy()[:, 0]
    b = sd["edge_encoder_global.feature_expansion.bias"].double().numpy()
    return np.asarray(length, dtype=np.float64)[:, None] * w + b


def mlp_encoder(sd, length, etype, dtype=torch.float64, mutate=()):
    """O.mlp_edge_encoder on edge_encoder_global in `dtype`: [n, 128].  mutate "type0_tables": every edge's type taken as 0."""
    from oracle import agdiff_oracle as O
    p = "edge_encoder_global"
    sdd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(p + ".")}
    ty = torch.as_tensor(np.asarray(etype)).long()
    if "type0_tables" in mutate:
        ty = torch.zeros_like(ty)
    return O.mlp_edge_encoder(sdd, p, torch.as_tensor(np.asarray(length)).to(dtype).view(-1, 1), ty)


def gaussian_encoder(sd, length, etype, cutoff=RC, dtype=torch.float64):
    from oracle import agdiff_oracle as O
    p = "edge_encoder_global"
    sdd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(p + ".")}
    return O.gaussian_edge_encoder(sdd, p, torch.as_tensor(np.asarray(length)).to(dtype), torch.as_tensor(np.asarray(etype)).long(), cutoff)


def gaussian_lengths(n):
    """float32 [n]: 0, -0.0, the 64 offsets' range [0, 2 rc] swept, 2 rc, and lengths beyond it up to 100 rc where every Gaussian
    underflows"""
    head = _f32([0.0, -0.0, 2.0 * RC, 3.0 * RC, 100.0 * RC, RC])
    if n <= head.size:
        return head[:n].copy()
    return np.concatenate([head, _f32(np.linspace(0.0, 2.2 * RC, n - head.size))])


def row_index_case(n, seed=29):
    """(row_index int32 [2 n], n_rows) for the positions pos_index / mir_index = scatter_indices(n) name: every fifth edge's
    position has no row (-1); every fourth edge with a mirror shares ONE row between its two positions; every other named position
    has a row of its own, in a shuffled order; unnamed positions have none.  n_rows counts the rows handed out plus three no
    position names."""
    pos, mir = scatter_indices(n)
    ri = np.full(2 * n, -1, dtype=np.int32)
    slots = []
    for e in range(n):
        if e % 5 == 4:
            if mir[e] >= 0:
                slots.append((mir[e],))
            continue
        if mir[e] >= 0 and e % 4 == 0:
            slots.append((pos[e], mir[e]))
        else:
            slots.append((pos[e],))
            if mir[e] >= 0:
                slots.append((mir[e],))
    n_rows = len(slots) + 3
    rows = np.random.default_rng(seed).permutation(n_rows)[:len(slots)]
    for r, ps in zip(rows, slots):
        for p in ps:
            ri[p] = r
    return ri, n_rows


def scatter_expected(values, size, pos=None, mir=None, row_index=None, mutate=()):
    """What a launch leaves in an output of `size` rows pre-filled with the payload: (rows float64 [size, ...] with NaN where the
    payload stays, written mask [size]).  Edge e's values go to position pos[e] (e itself without pos) and mir[e] (>= 0); with
    row_index, position p stands for row row_index[p] (< 0: none).  mutate "mirror_not_written"."""
    values = np.asarray(values, dtype=np.float64)
    n = values.shape[0]
    out = np.full((size,) + values.shape[1:], NAN)
    written = np.zeros(size, dtype=bool)
    p = np.arange(n) if pos is None else np.asarray(pos, dtype=np.int64)
    targets = [(p, np.arange(n))]
    if mir is not None and "mirror_not_written" not in mutate:
        has = np.nonzero(np.asarray(mir) >= 0)[0]
        targets.append((np.asarray(mir, dtype=np.int64)[has], has))
    for where, e in targets:
        if row_index is not None:
            where = np.asarray(row_index, dtype=np.int64)[where]
            e, where = e[where >= 0], where[where >= 0]
        out[where] = values[e]
        written[where] = True
    return out, written


def payload_error(got, ref):
    """max |got - ref| where both hold numbers; inf where exactly one of them holds the payload (NaN)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if (np.isnan(got) != np.isnan(ref)).any():
        return float("inf")
    both = ~np.isnan(ref)
    return float(np.abs(got[both] - ref[both]).max()) if both.any() else 0.0


# ------------------------------------------------------------------------------------------------- flagged tiles (test E)
UNSLOTTED_TYPE = 23         # the local type the test's model refuses a polynomial slot (poly_refuse_types)
SLOTTED_TYPES = (1, 2, 12, 24)


def flagged_case(n_tiles=7, live_last=11):
    """A canonical local list of n_tiles tiles, the last with `live_last` rows, as dict(length float32 [E], etype int32 [E], hard bool
    [E], masks [n_tiles], soft_length, soft_type).  Tile 1 has hard-row mask 0x0001 (a length beyond 10 rc: past any far set), tile
    3 0x8000 (UNSLOTTED_TYPE at a length inside the cutoff), the last tile every live row (both causes in turn); tiles 0, 2, 4, 5 are
    clean.  soft_*: the same list with the hard rows made soft -- their lengths moved inside the cutoff, their types slotted."""
    E = 16 * (n_tiles - 1) + live_last
    rng = np.random.default_rng(83)
    length = rng.uniform(0.05, 0.95, size=E) * RC
    etype = np.asarray(SLOTTED_TYPES, dtype=np.int32)[(np.arange(E) * 3 + np.arange(E) // 16) % len(SLOTTED_TYPES)]
    by_length, by_type = np.zeros(E, dtype=bool), np.zeros(E, dtype=bool)
    by_length[16 * 1 + 0] = True
    by_type[16 * 3 + 15] = True
    last = np.arange(16 * (n_tiles - 1), E)
    by_length[last[0::2]] = True
    by_type[last[1::2]] = True
    hard = by_length | by_type
    soft_length, soft_type = length.copy(), etype.copy()
    soft_length[by_length] = 0.5 * RC
    length[by_length] = 12.0 * RC + np.arange(int(by_length.sum()))
    etype[by_type] = UNSLOTTED_TYPE
    masks = np.asarray([sum(1 << r for r in range(16) if 16 * k + r < E and hard[16 * k + r]) for k in range(n_tiles)])
    return dict(length=_f32(length), etype=etype, hard=hard, masks=masks, soft_length=_f32(soft_length), soft_type=soft_type)


# ------------------------------------------------------------------------------------------------- the producers' batch (test C)
def producer_batch(which="wide"):
    """dict(atom_type, bond_index, bond_type, batch, num_graphs, pos float32 [N, 3], kinks) of four molecules:
      A  atom 0 at the origin and atom j at (kink_j, 0, 0) for every kink of the set inside (0, rc): the radius row 0 -> j has length
         kink_j exactly (sqrt(fl(x^2)) == x in binary floating point), and every atom has more neighbours than the 33-row cap
         keeps; one bond (1, 2)
      B  two bonded atoms: no radius row at all
      C  two atoms without a bond, 5 apart: one radius row each
      D  40 atoms around the origin, a chain of single bonds: every target has more neighbours than the cap keeps (the last six
         end with all 33 rows, the others lose one to themselves and one or two to their bonds)"""
    k = all_kinks(which)
    k = k[(k > 0) & (k < RC32)]
    nA = 1 + k.size
    rng = np.random.default_rng(97)
    posA = np.zeros((nA, 3), dtype=np.float32)
    posA[1:, 0] = k
    posB = np.asarray([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0]], dtype=np.float32)
    posC = np.asarray([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]], dtype=np.float32)
    posD = (rng.standard_normal((40, 3)) * 1.5).astype(np.float32)
    offB, offC, offD = nA, nA + 2, nA + 4
    chain = np.arange(39) + offD
    src = np.concatenate([[1, 2], [offB, offB + 1], chain, chain + 1])
    dst = np.concatenate([[2, 1], [offB + 1, offB], chain + 1, chain])
    sizes = [nA, 2, 2, 40]
    return dict(atom_type=np.full(sum(sizes), 6, dtype=np.int64), bond_index=np.stack([src, dst]).astype(np.int64),
                bond_type=np.ones(src.size, dtype=np.int64), batch=np.repeat(np.arange(4), sizes).astype(np.int64), num_graphs=4,
                pos=np.concatenate([posA, posB, posC, posD]), kinks=k, sizes=sizes)
