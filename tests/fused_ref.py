"""float64 restatement of k_cfconv_fused (csrc/edge.hip) -- the two CFConvs of an InteractionBlock with their filters from the filter
MLPs, over ONE destination-sorted edge list cut into chunks --, the operand form of its attribute rows, what a launch must leave
in agg and agg_first, the launcher's shape rules, and the edge lists the tests run it on.  tests/test_fused_ref_cpu.py anchors it on
the CPU, tests/test_hip_fused_kernels.py runs the kernel against it on the GPU (agdiff_cfconv_fused, agdiff_cfconv_local).

Test infrastructure only.  Everything the kernel reads is DATA here: in_ptr, sources, the twelve scale planes, the attribute rows and
xs are drawn or written down, not built from molecules.

    W_e[c]   = (Linear2(ShiftedSoftplus(Linear1(attr_e))))[c] * s_c(e)          s_c: plane 2 k for c < 128 (conv1), 2 k + 1 after
    agg[dst] += xs[src] * W_e                                                   conv1: channels 0..127, conv2: 128..191

The lists are degree sequences.  A tile is 16 consecutive edges; a chunk is chunk_tiles (1, 2, 4, 8) consecutive tiles, walked by one
wave that keeps the open list's sums in registers.  A list's part in the chunk where it starts goes to agg[node], every later
chunk's part to agg_first[chunk]."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from node_ref import ATTR_STD, draw

TW = 16
MAX_CHUNK_TILES = 8      # AGDIFF_MAX_CHUNK_TILES
CONV_WAVES = 8           # waves (= chunks per round) of a workgroup
CUS = 256
NPLANES = 12             # 2 x 6 blocks
MODES = ("f32", "bf16x3", "f16x3")


# ------------------------------------------------------------------------------------------------- operand form
def _split(x, precision):
    """(hi, lo) float32: hi = x rounded to the 16-bit type of the mode, lo = the rounded remainder."""
    dt = torch.float16 if precision == "f16x3" else torch.bfloat16
    x = torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32)
    hi = x.to(dt)
    lo = (x - hi.to(torch.float32)).to(dt)
    return hi, lo


def operands(rows, precision):
    """What the kernel multiplies: the rows themselves in f32, hi + lo (float64, exact) in the split modes."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if precision == "f32":
        return rows.astype(np.float64)
    hi, lo = _split(rows, precision)
    return hi.double().numpy() + lo.double().numpy()


def frag(rows, precision):
    """fp32 rows [n][128] -> the operand-form buffer of the mode (float32 words, n rounded up to whole tiles with zero rows): the
    inverse of test_hip_parity.unfrag.  f32: [tile][t][u][edge][q][r], feature 32 t + 16 u + 4 q + r.  Split modes:
    [tile][t][part][edge][q][u][r] 16-bit values, part 0 = hi, part 1 = lo."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n = rows.shape[0]
    tiles = (n + TW - 1) // TW
    x = torch.zeros(tiles * TW, 128, dtype=torch.float32)
    x[:n] = torch.from_numpy(rows)
    x = x.view(tiles, TW, 4, 2, 4, 4)                                  # (tile, edge, t, u, q, r)
    if precision == "f32":
        return x.permute(0, 2, 3, 1, 4, 5).contiguous().view(-1)
    hi, lo = _split(x.permute(0, 2, 1, 4, 3, 5).contiguous(), precision)   # (tile, t, edge, q, u, r)
    both = torch.stack([hi, lo], dim=2).contiguous()                   # (tile, t, part, edge, q, u, r)
    return both.view(torch.int16).view(-1).view(torch.float32)


# ------------------------------------------------------------------------------------------------- the arithmetic
def _lin(sd, p, x, bias=True):
    return F.linear(x, sd[p + ".weight"], sd[p + ".bias"] if bias else None)


def messages(sd, cfg, k, attr, scale1, scale2, src, xs, mutate=()):
    """xs[src] * W_e per edge: float64 [E, 192].  mutate: the wrong kernels tests/test_fused_ref_cpu.py lists, a dict name -> parameter."""
    blk = "encoder_global.interactions.%d" % k
    attr = torch.as_tensor(np.asarray(attr)).double()
    xs = torch.as_tensor(np.asarray(xs)).double()
    src = torch.as_tensor(np.asarray(src)).long()
    s1, s2 = (torch.as_tensor(np.asarray(s)).double().view(-1) for s in (scale1, scale2))
    if "scales_swapped" in mutate:
        s1, s2 = s2, s1
    out = torch.zeros(attr.shape[0], 192, dtype=torch.float64)
    for c, lo, hi, s in ((1, 0, 128, s1), (2, 128, 192, s2)):
        p = "%s.conv%d" % (blk, c)
        beta = 1.0 if "no_beta" in mutate else sd[p + ".nn.1.beta"]
        pre = _lin(sd, p + ".nn.0", attr, bias="no_bias1" not in mutate)
        hid = F.softplus(beta * pre) - (0.0 if "no_shift" in mutate else math.log(2.0))
        W = _lin(sd, p + ".nn.2", hid, bias="no_bias2" not in mutate)
        if "no_scale%d" % c not in mutate:
            W = W * s.view(-1, 1)
        out[:, lo:hi] = xs[src, lo:hi] * W
    return out


def cfconv_fused(sd, cfg, k, attr, scale1, scale2, src, dst, xs, mutate=()):
    """agg [N, 192] in float64, N = rows of xs: the body of test_hip_kernels._agg_ref with the scales as data."""
    msg = messages(sd, cfg, k, attr, scale1, scale2, src, xs, mutate)
    src = torch.as_tensor(np.asarray(src)).long()
    dst = torch.as_tensor(np.asarray(dst)).long()
    if "src_for_dst" in mutate:
        dst = src
    if "edge_dropped" in mutate:
        msg[mutate["edge_dropped"]] = 0.0
    return torch.zeros(np.asarray(xs).shape[0], 192, dtype=torch.float64).index_add_(0, dst, msg)


# ------------------------------------------------------------------------------------------------- agg / agg_first
def split(in_ptr, per_edge, chunk_edges):
    """What a launch must leave: dict(agg [N, 192], agg_first [chunks, 192] (float64; rows never written are 0 here), rows_agg,
    rows_first: the sorted rows of each buffer a launch writes -- a node with a non-empty list; a chunk that some list enters from
    an earlier chunk).  per_edge [E, 192] in list order.  node_ref.gathered_aggregate inverts it."""
    ip = np.asarray(in_ptr, dtype=np.int64)
    msg = torch.as_tensor(np.asarray(per_edge)).double()
    n, ce, E = ip.shape[0] - 1, int(chunk_edges), int(ip[-1])
    assert msg.shape[0] == E
    chunks = (E + ce - 1) // ce
    agg = torch.zeros(n, 192, dtype=torch.float64)
    first = torch.zeros(max(chunks, 1), 192, dtype=torch.float64)
    rows_agg, rows_first = [], set()
    for i in range(n):
        lo, hi = int(ip[i]), int(ip[i + 1])
        if hi <= lo:
            continue
        rows_agg.append(i)
        c0 = lo // ce
        agg[i] = msg[lo:min(hi, (c0 + 1) * ce)].sum(dim=0)
        for c in range(c0 + 1, (hi - 1) // ce + 1):
            first[c] += msg[c * ce:min(hi, (c + 1) * ce)].sum(dim=0)
            rows_first.add(c)
    return dict(agg=agg, agg_first=first, rows_agg=np.asarray(rows_agg, dtype=np.int64),
                rows_first=np.asarray(sorted(rows_first), dtype=np.int64))


# ------------------------------------------------------------------------------------------------- launch shapes
def conv_chunk_tiles(max_edges):
    """agdiff_conv_chunk_tiles restated (csrc/api.hip)."""
    tiles = (int(max_edges) + TW - 1) // TW
    c = 1
    while c < MAX_CHUNK_TILES and tiles // (2 * c) >= 16 * 2048:
        c *= 2
    return c


def smallest_capacity(chunk_tiles, rule=conv_chunk_tiles):
    """The smallest max_edges at which `rule` (monotone) returns `chunk_tiles`: by bisection, not from the rule's constants."""
    if rule(1) == chunk_tiles:
        return 1
    lo, hi = 1, 1 << 30
    assert rule(hi) >= chunk_tiles
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if rule(mid) >= chunk_tiles:
            hi = mid
        else:
            lo = mid
    assert rule(hi) == chunk_tiles
    return hi


def classify(in_ptr, E, chunk_tiles, max_edges):
    """What a launch over the list `in_ptr` (E live edges, capacity max_edges, chunk_tiles tiles per chunk) goes through.
    dict(tiles = one dict per live tile: ntg (t1 - t0 + 1: empty lists between the tile's first and last target count), path
    ("one" / "two" / "general"), flush (the wave's previous tile ended on a list end), carry (an open list enters from the wave's
    previous tile), big (ntg > 64), first_from_earlier_chunk (the tile's first list started before the chunk);
    zeroed = the empty lists inside a general tile (the general reduction stores their zero sums);
    grid = min(ceil(chunks / 8), 256), remap (grid % 8 == 0), rounds = chunks one wave walks at most, chunks)."""
    ip = np.asarray(in_ptr, dtype=np.int64)
    E, ct = int(E), int(chunk_tiles)
    assert E == ip[-1] and E <= max_edges
    n = ip.shape[0] - 1
    dst = np.repeat(np.arange(n), np.diff(ip))
    tiles, zeroed = [], []
    for tile in range((E + TW - 1) // TW):
        tb = tile * TW
        t0, t1 = int(dst[tb]), int(dst[min(tb + TW, E) - 1])
        ntg = t1 - t0 + 1
        first = tile % ct == 0
        prev = None if first else int(dst[tb - 1])
        path = "one" if ntg == 1 else "two" if ntg == 2 else "general"
        if path == "general":
            zeroed += [t for t in range(t0 + 1, t1) if ip[t + 1] == ip[t]]
        tiles.append(dict(ntg=ntg, path=path, flush=prev is not None and prev != t0, carry=prev is not None and prev == t0,
                          big=ntg > 64, first_from_earlier_chunk=int(ip[t0]) < (tile // ct) * ct * TW, partial=tb + TW > E))
    max_tiles = (int(max_edges) + TW - 1) // TW
    max_chunks = (max_tiles + ct - 1) // ct
    grid = min((max_chunks + CONV_WAVES - 1) // CONV_WAVES, CUS)
    live = min((E + TW * ct - 1) // (TW * ct), max_chunks)
    stride = grid * CONV_WAVES
    return dict(tiles=tiles, zeroed=np.asarray(sorted(set(zeroed)), dtype=np.int64), chunk_tiles=ct, chunks=max_chunks, grid=grid,
                remap=grid % 8 == 0 and grid > 0, rounds=(live + stride - 1) // stride if stride else 0)


def list_classes(in_ptr, chunk_edges):
    """Names of what the lists do at chunk boundaries (tests/test_fused_ref_cpu.py asserts the whole set)."""
    ip, ce = np.asarray(in_ptr, dtype=np.int64), int(chunk_edges)
    out = set()
    for i, (lo, hi) in enumerate(zip(ip[:-1], ip[1:])):
        if hi == lo:
            continue
        span = (hi - 1) // ce - lo // ce + 1
        out.add("spans %d" % min(span, 4))
        if lo % ce == 0 and lo > 0:
            out.add("starts on a boundary after another list")
        if lo % ce == ce - 1 and hi - lo >= 2:
            out.add("starts one edge before a boundary")
        if span >= 3:
            out.add("a chunk inside one hub")
        if hi % TW == 0 and hi % ce != 0 and lo // ce < (hi - 1) // ce and hi < ip[-1]:
            out.add("entered list ends on a tile end inside a chunk")
    return out


# ------------------------------------------------------------------------------------------------- the lists
# Offsets in the comments are edge offsets; a tile is [16 j, 16 j + 16).
_SHAPES = (
    [0, 0]                     # empty lists before the first list
    + [16, 16]                 # tiles 0, 1: one target each, aligned; tile 0's list ends on the tile end, tile 1 brings a new target
    + [0]                      # an empty list between two tiles (offset 32)
    + [8, 8]                   # tile 2: two targets
    + [5, 5, 6]                # tile 3: three targets
    + [1] * 16                 # tile 4: sixteen targets of degree 1
    + [33]                     # a hub at offset 0 of tile 5: tiles 5, 6 whole, one edge of tile 7
    + [3, 0, 4, 8]             # tile 7: the hub's last edge, then 3 | an empty list inside the tile | 4 | 8; ends on the tile end (128)
    + [1, 40]                  # tile 8: one edge, then a hub at offset 1: 129 .. 168 (tile 9 whole, nine edges of tile 10)
    + [3] + [0] * 70 + [1] * 4   # tile 10: hub | 3 | seventy empty lists | four lists of one edge: 76 targets; ends on 176
    + [15, 64]                 # tile 11: fifteen edges, then a hub at offset 15: 191 .. 254 (tiles 12..14 whole, 15 edges of tile 15)
    + [1]                      # tile 15: hub | 1; ends on 256
    + [100]                    # a hub at offset 0: tiles 16 .. 21 whole, four edges of tile 22
    + [2, 3, 7]                # tile 22: hub | 2 | 3 | 7; ends on 368
)
_TAILS = {0: [], 1: [1], 15: [4, 0, 5, 6]}        # E mod 16: a last tile with one edge; with fifteen (three lists and an empty one)
N_SMALL = 512                                      # nodes of shapes / chunks (the sequences are padded with empty lists)
SHAPES = ("mod0", "mod1", "mod15", "one", "none")
CHUNK_EDGES = (16, 32, 128)


def _pad(deg, n):
    assert len(deg) + 2 <= n
    return np.asarray(list(deg) + [0] * (n - len(deg)), dtype=np.int64)


def shapes(variant):
    """in_ptr [N_SMALL + 1] of the `shapes` list: "mod0" / "mod1" / "mod15" (E = 368, 369, 383), "one" (E = 1), "none" (E = 0)."""
    if variant == "one":
        deg = [0, 1, 0]
    elif variant == "none":
        deg = [0, 0, 0]
    else:
        deg = list(_SHAPES) + _TAILS[int(variant[3:])]
    return np.concatenate([[0], np.cumsum(_pad(deg, N_SMALL))])


def chunks(ce):
    """in_ptr [N_SMALL + 1] of the `chunks` list for chunks of `ce` edges (16, 32, 128); the shapes list follows from a chunk
    boundary on."""
    assert ce in CHUNK_EDGES
    deg = ([ce]                # 0 .. ce: boundary to boundary
           + [ce - 1]          # starts exactly on the boundary ce (all of it in agg), ends one edge before 2 ce
           + [2]               # starts one edge before the boundary 2 ce: one edge in agg, one in agg_first[2]
           + [3 * ce - 3]      # a hub over three chunks: 2 ce + 1 .. 5 ce - 3 (chunk 3 lies inside it)
           + [2]               # 5 ce - 2, 5 ce - 1: a tile with the hub's end and a second target, the hub's part in agg_first[4]
           + [0]               # an empty list on the boundary 5 ce
           + [ce]              # starts exactly on the boundary 5 ce after another list
           + [ce - 1]
           + [2 * ce + 3]      # starts one edge before 7 ce, four chunks: 7 ce - 1 .. 9 ce + 1 (chunks 7 and 8 lie inside it)
           + [5, 0, 3]         # the tile at 9 ce: hub (agg_first[9]) | 5 | empty | 3 | the next list's first six edges
           + [ce + 6]          # 9 ce + 10 .. 10 ce + 15: entered chunk 10 from chunk 9, ends on a tile end inside chunk 10 (ce > 16)
           + ([ce - 16] if ce > 16 else []))         # a new target up to the boundary 11 ce
    assert sum(deg) == 11 * ce
    return np.concatenate([[0], np.cumsum(_pad(deg + list(_SHAPES) + _TAILS[15], N_SMALL))])


ROUNDS_PATTERN = (16, 7, 9, 33, 1, 0, 20, 12, 2, 64, 5, 11, 8, 8, 3, 0, 0, 27)        # 226 edges per 18 nodes
ROUNDS_REPEATS = 150                                                                  # 33,900 edges > 2048 x 16
N_ROUNDS = len(ROUNDS_PATTERN) * ROUNDS_REPEATS + 3


def rounds():
    """in_ptr [N_ROUNDS + 1]: ROUNDS_PATTERN repeated -- more than 2048 chunks of one tile, so that on a grid of 256 workgroups
    (2048 waves) some waves walk a second chunk."""
    deg = list(ROUNDS_PATTERN) * ROUNDS_REPEATS
    return np.concatenate([[0], np.cumsum(_pad(deg, N_ROUNDS))])


def prefix(in_ptr, cap):
    """The list cut to a capacity: the lists that end within `cap` edges stay, every later one is empty."""
    ip = np.asarray(in_ptr, dtype=np.int64)
    e = int(ip[ip <= cap].max())
    return np.minimum(ip, e)


def inputs(name, in_ptr, n_attr=None):
    """The seeded data of a list (dict): src, dst [E]; attr [Epad, 128] float32 (rows past E: finite decoys); xs [N, 192]; planes
    [12, Epad] float32 in [0, 1], about one in ten exactly 0 (entries past E: decoys of 0.75 -- the kernel must select 0 there)."""
    ip = np.asarray(in_ptr, dtype=np.int64)
    n, E = ip.shape[0] - 1, int(ip[-1])
    epad = max((E + TW - 1) // TW, 1) * TW
    rng = np.random.default_rng(sum(map(ord, name)) + 4000)
    dst = np.repeat(np.arange(n), np.diff(ip))
    src = rng.integers(0, n, size=epad)
    planes = rng.uniform(0.0, 1.0, size=(NPLANES, epad))
    planes[rng.uniform(size=planes.shape) < 0.1] = 0.0
    planes[:, E:] = 0.75
    return dict(src=src[:E], src_pad=src, dst=dst, attr=draw("attr:" + name, (epad, 128), ATTR_STD), xs=draw("xs:" + name, (n, 192)),
                planes=planes.astype(np.float32), E=E, N=n, epad=epad)


# ------------------------------------------------------------------------------------------------- the local batch
STAR_LEAVES = (7, 8, 9, 33, 64, 1)
STAR_TYPES = (1, 2, 3)


def star_batch():
    """Stars without order extension: a centre with 7, 8, 9, 33, 64 and 1 bonded leaves -- local in-degrees 7, 8, 9, 33, 64 at the
    centres and 1 at every leaf; bond types 1, 2, 3 in turn.  dict as cfconv_ref.make_batch."""
    rs, cs, ts, sizes, off = [], [], [], [], 0
    for m in STAR_LEAVES:
        leaves = off + 1 + np.arange(m)
        ty = np.asarray(STAR_TYPES)[np.arange(m) % len(STAR_TYPES)]
        rs += [np.full(m, off), leaves]
        cs += [leaves, np.full(m, off)]
        ts += [ty, ty]
        sizes.append(m + 1)
        off += m + 1
    cat = lambda xs: np.concatenate(xs).astype(np.int64)
    return dict(atom_type=np.full(off, 6, dtype=np.int64), bond_index=np.stack([cat(rs), cat(cs)]), bond_type=cat(ts),
                batch=np.repeat(np.arange(len(sizes)), sizes), num_graphs=len(sizes), extend_order=False)
