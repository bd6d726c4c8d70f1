"""float64 restatement of the dense per-node kernels of csrc/node.hip -- the SchNet node stage (k_schnet_node_stage,
k_schnet_node_stage_split), the aggregate sources it reads (ag_agg_src / ag_agg_slice) and the GIN encoder (k_gin_gather,
k_gin_layer, k_gin_layer_persistent) --, the seeded inputs, and the launchers' shape rules, which tests/test_node_ref_cpu.py
anchors on the CPU and tests/test_hip_node_kernels.py runs on the GPU.

Test infrastructure only.  The arithmetic is torch, straight from the UNPACKED state dict: batch norm is applied as batch norm,
ShiftedSoftplus in base e, nothing folded -- so a folding error of packing.py in one block shows as that block's stage.  The
functions compute in the dtype of the state dict they are given (float64 for the reference; tests/test_node_ref_cpu.py also runs
them in float32 to show how far plain float32 arithmetic lies from it).  In-lists are data: (in_ptr, in_src, in_row), not
molecules."""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

G = "encoder_global"
L = "encoder_local"


# ------------------------------------------------------------------------------------------------- state dict
# GINEConv.eps is a buffer the reference initialises to 0 (gin.py:19-36) and the synthetic checkpoint keeps; a kernel that
# dropped the (1 + eps) factor would then go unnoticed.  The tests' checkpoint gives every layer its own non-zero value.
GIN_EPS = (0.25, -0.125, 0.375, -0.3125, 0.1875, -0.0625, 0.4375, -0.1875)


def state_dict(cfg):
    """The synthetic checkpoint of `cfg` (float32, as the model loads it) with GIN_EPS, cut to cfg.num_convs_local layers (the
    key list has the four of the reference's configs).  Aliases share storage, as in oracle.synth_state_dict_for."""
    from agdiff_amd import synth
    from oracle import agdiff_oracle as O
    sd = O.synth_state_dict_for(cfg)
    out = {}
    for k, v in sd.items():
        c = synth.canonical_key(k)
        parts = c.split(".")
        if parts[0] == L and parts[1] in ("convs", "batch_norms") and int(parts[2]) >= cfg.num_convs_local:
            continue
        if parts[0] == L and parts[1] == "convs" and parts[-1] == "eps":
            sd[c].fill_(GIN_EPS[int(parts[2])])
        out[k] = v
    return out


def to64(sd):
    return {k: (v.detach().double().cpu() if v.is_floating_point() else v.detach().cpu()) for k, v in sd.items()}


def _lin(sd, p, x):
    return F.linear(x, sd[p + ".weight"], sd.get(p + ".bias"))


def _bn(sd, p, x, eps=1e-5):
    return (x - sd[p + ".running_mean"]) / torch.sqrt(sd[p + ".running_var"] + eps) * sd[p + ".weight"] + sd[p + ".bias"]


def _ssp(beta, x):
    return F.softplus(beta * x) - math.log(2.0)


def _as(sd, x):
    """`x` (array or tensor) in the floating dtype of the state dict."""
    x = torch.as_tensor(np.ascontiguousarray(x)) if not torch.is_tensor(x) else x
    return x.to(sd[G + ".embedding.weight"].dtype)


def _idx(x):
    return torch.as_tensor(np.ascontiguousarray(x) if not torch.is_tensor(x) else x).long().reshape(-1)


# ------------------------------------------------------------------------------------------------- SchNet node stage
def prep(sd, k, h):
    """xs of block k: LeakyReLU(BN(lin1(h))) of conv1 | conv2, 128 + 64 columns (schnet.py:153-155)."""
    return torch.cat([F.leaky_relu(_bn(sd, "%s.interactions.%d.conv%d.norm1" % (G, k, c),
                                       _lin(sd, "%s.interactions.%d.conv%d.lin1" % (G, k, c), h)), 0.2) for c in (1, 2)], dim=1)


def increment(sd, k, agg):
    """What block k adds to h, from its 192-wide aggregate (128 columns of conv1 | 64 of conv2): p_c = BN(lin2_c(agg_c))
    (schnet.py:157-158), x = lin(ssp(cat)), x *= sigmoid(att(x)) (schnet.py:206-214), x * sigmoid(fc2(relu(fc0(x))))
    (schnet.py:230-234)."""
    p = "%s.interactions.%d" % (G, k)
    p1 = _bn(sd, p + ".conv1.norm2", _lin(sd, p + ".conv1.lin2", agg[:, :128]))
    p2 = _bn(sd, p + ".conv2.norm2", _lin(sd, p + ".conv2.lin2", agg[:, 128:192]))
    x = _lin(sd, p + ".lin", _ssp(sd[p + ".act.beta"], torch.cat([p1, p2], dim=1)))
    x = x * torch.sigmoid(_lin(sd, p + ".attention.2", F.relu(_lin(sd, p + ".attention.0", x))))
    s = "%s.scaling_modules.%d" % (G, k)
    return x * torch.sigmoid(F.linear(F.relu(F.linear(x, sd[s + ".fc.0.weight"])), sd[s + ".fc.2.weight"]))


def stage(sd, cfg, k, h_in, agg, atom_type, mutate=()):
    """Stage k of SchNetEncoder.forward as agdiff_schnet_node_stage(k) cuts it: (h, xs).
    k = 0: h = embedding[z] (the rows as the state dict holds them: the max_norm renorm is the caller's).
    k >= 1: h = h_in + block k-1's increment from `agg`.   k < num_convs: xs = prep(k, h), else None.
    mutate (the sensitivity tests): "no_residual_last_node" returns the increment alone in the last row."""
    if k == 0:
        h = sd[G + ".embedding.weight"][_idx(atom_type)]
    else:
        h_in, inc = _as(sd, h_in), increment(sd, k - 1, _as(sd, agg))
        h = h_in + inc
        if "no_residual_last_node" in mutate:
            h[-1] = inc[-1]
    return h, (prep(sd, k, h) if k < cfg.num_convs else None)


def gathered_aggregate(in_ptr, agg, agg_first, chunk_edges):
    """The aggregate ag_agg_src / ag_agg_slice hand a node from one chunked CFConv pass (csrc/edge.hip leaves the part of a
    node's edge list that lies in the chunk where the list starts in agg[node], every later chunk's part in agg_first[chunk]):
    0 for an empty list -- agg[node] is then not read --, else agg[i] + agg_first[c] for c = lo // ce + 1 .. (hi - 1) // ce in
    chunk order.  float64 [N, 192].  A block that ran two passes (split bit 8) gets the sum of two calls."""
    ip = np.asarray(in_ptr, dtype=np.int64)
    agg = torch.as_tensor(np.asarray(agg)).double()
    first = torch.as_tensor(np.asarray(agg_first)).double()
    n, ce = ip.shape[0] - 1, int(chunk_edges)
    out = torch.zeros(n, agg.shape[1], dtype=torch.float64)
    for i in range(n):
        lo, hi = int(ip[i]), int(ip[i + 1])
        if hi <= lo:
            continue
        row = agg[i].clone()
        for c in range(lo // ce + 1, (hi - 1) // ce + 1):
            row += first[c]
        out[i] = row
    return out


def chunks_read(in_ptr, chunk_edges):
    """The rows of agg_first some list refers to."""
    ip, ce = np.asarray(in_ptr, dtype=np.int64), int(chunk_edges)
    return sorted({c for lo, hi in zip(ip[:-1], ip[1:]) if hi > lo for c in range(lo // ce + 1, (hi - 1) // ce + 1)})


# ------------------------------------------------------------------------------------------------- GIN encoder
def gin(sd, cfg, atom_type, in_ptr, in_src, in_row, rows, mutate=()):
    """GINEncoder.forward (gin.py:112-148) with GINEConv (:38-69) over in-lists: node i's messages are the slots
    in_ptr[i] .. in_ptr[i + 1] - 1, slot s from node in_src[s] with attribute row rows[in_row[s]]:
    m_i = sum relu(h[src] + rows[row]) + (1 + eps) h_i; u = BN(lin1(relu(lin0(m)))); relu except after the last layer;
    h = u + h.  Layer 0 reads node_emb[z].  cfg.num_convs_local layers.
    mutate (the sensitivity tests): "relu_last" applies the relu after the last layer too, "no_residual_last_node" leaves
    the last layer's h out of the last node's row."""
    ip = _idx(in_ptr)
    n = ip.shape[0] - 1
    total = int(ip[-1])
    src, row = _idx(in_src)[:total], _idx(in_row)[:total]
    dst = torch.repeat_interleave(torch.arange(n), ip[1:] - ip[:-1])
    attr = _as(sd, rows)[row]
    h = sd[L + ".node_emb.weight"][_idx(atom_type)]
    nconv = cfg.num_convs_local
    for k in range(nconv):
        m = torch.zeros_like(h).index_add_(0, dst, F.relu(h[src] + attr)) + (1 + sd["%s.convs.%d.eps" % (L, k)]) * h
        q = "%s.convs.%d.nn.layers" % (L, k)
        u = _bn(sd, "%s.batch_norms.%d" % (L, k), _lin(sd, q + ".1", F.relu(_lin(sd, q + ".0", m))))
        if k < nconv - 1 or "relu_last" in mutate:
            u = F.relu(u)
        new = u + h
        if k == nconv - 1 and "no_residual_last_node" in mutate:
            new[-1] = u[-1]
        h = new
    return h


def in_lists(n, src, dst, row):
    """(in_ptr, in_src, in_row) of an edge list: grouped by destination, sources ascending inside a list (topology.py)."""
    src, dst, row = (np.asarray(a, dtype=np.int64) for a in (src, dst, row))
    o = np.lexsort((src, dst))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))])
    return ptr, src[o], row[o]


# ------------------------------------------------------------------------------------------------- seeded inputs
def draw(name, shape, std=1.0):
    """float32 normals, seeded by `name`: h, agg and agg_first at std 1 (an aggregate drawn at 0.05 makes the block's increment
    so small that element-wise float32 noise on it alone reaches the f32 gate), attribute rows at ATTR_STD."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return (rng.standard_normal(shape) * std).astype(np.float32)


ATTR_STD = 0.3           # the forward fixtures' edge_attr has standard deviation 0.22


def atom_types(n, rows=100):
    """Types that walk the whole embedding table, the last row and row 0 first: 99, 0, 1, ..."""
    return ((rows - 1 + np.arange(n)) % rows).astype(np.int64)


# The synthetic in-lists of the GIN tests.  (even, odd) node pairs share a wave of k_gin_gather, a half-wave each, and walk
# max(degree) slots 32 at a time: pairs with a list past 32 / 64 / 96 next to a short or empty one, in both orders.
PAIR_DEGREES = ((0, 0), (0, 1), (1, 0), (3, 4), (4, 5), (31, 32), (32, 33), (33, 0), (0, 33), (64, 65), (65, 1), (100, 2))
HUB = 22                 # the node with 100 in-edges


def synthetic_in_lists(n, num_rows, seed=0, tail_degree=5):
    """In-lists as data for `n` nodes (odd: the last node's half-wave partner does not exist): PAIR_DEGREES on the first 24 nodes,
    degrees 0..6 after them, `tail_degree` on the last.  Sources are arbitrary nodes -- the node itself and repeats included,
    ascending inside a list as topology.py leaves them -- except LEAF = n - 1, which sends exactly one message: the hub's last
    (slot 99 of its list, the fourth 32-slot pass).  Row indices are drawn from [0, num_rows) twice, once for the `row` table and
    once for the `eid` table.  Returns dict(in_ptr, in_src, in_row, in_eid, degree, leaf, hub_last_slot)."""
    assert n % 2 == 1 and n >= 2 * len(PAIR_DEGREES) + 3
    rng = np.random.default_rng(7000 + seed)
    deg = np.zeros(n, dtype=np.int64)
    deg[: 2 * len(PAIR_DEGREES)] = np.asarray(PAIR_DEGREES).reshape(-1)
    deg[2 * len(PAIR_DEGREES):] = rng.integers(0, 7, size=n - 2 * len(PAIR_DEGREES))
    deg[-1] = tail_degree
    leaf = n - 1
    ptr = np.concatenate([[0], np.cumsum(deg)])
    total = int(ptr[-1])
    src = np.empty(total, dtype=np.int64)
    others = np.setdiff1d(np.arange(n), [leaf])
    for i in range(n):
        s = np.sort(rng.choice(others, size=deg[i], replace=True))
        if deg[i] >= 3:
            s[0] = s[1]                                # a repeat ...
            s[2] = i if i != leaf else s[2]            # ... and the node itself
            s = np.sort(s)
        src[ptr[i]:ptr[i + 1]] = s
    hub_last = int(ptr[HUB + 1] - 1)
    src[hub_last] = leaf                               # (the largest index: the list stays ascending)
    row = rng.permutation(num_rows)[:total] if total <= num_rows else rng.integers(0, num_rows, size=total)
    eid = rng.permutation(num_rows)[:total] if total <= num_rows else rng.integers(0, num_rows, size=total)
    assert deg[HUB] == 100 and not np.array_equal(row, eid)
    return dict(in_ptr=ptr, in_src=src, in_row=row, in_eid=eid, degree=deg, leaf=leaf, hub_last_slot=hub_last)


def chunked_in_ptr(n, ce, max_total):
    """in_ptr of the chunked-aggregate test for `n` >= 12 nodes and chunks of `ce` edges: lists that start on a chunk boundary,
    end exactly on one, lie inside one chunk, span three and four chunks, and empty lists -- one of them with `lo` on a boundary.
    Later nodes repeat the pattern while the total stays within `max_total`; the rest are empty."""
    pattern = [ce,            # 0: starts on a boundary (0), ends exactly on one
               0,             # 1: empty, lo on a boundary
               ce // 2,       # 2: starts on a boundary, inside one chunk
               ce // 4,       # 3: inside the same chunk
               0,             # 4: empty, lo inside a chunk
               2 * ce,        # 5: starts inside chunk 1, spans chunks 1, 2, 3 (three chunks)
               ce // 4,       # 6: ends exactly on the boundary 4 ce
               3 * ce,        # 7: boundary to boundary, three whole chunks
               1,             # 8: one edge, the first of a chunk
               3 * ce + 2,    # 9: four chunks
               0,             # 10: empty
               ce - 3]        # 11: ends exactly on a boundary: 1 + 3 ce + 2 + ce - 3 = 4 ce
    deg = np.zeros(n, dtype=np.int64)
    k = 0
    while k + len(pattern) <= n and deg.sum() + sum(pattern) <= max_total:
        deg[k:k + len(pattern)] = pattern
        k += len(pattern)
    assert k >= len(pattern), "the batch leaves no room for one round of the pattern"
    return np.concatenate([[0], np.cumsum(deg)])


def list_shapes(in_ptr, ce):
    """What the lists of `in_ptr` exercise: a set of names (tests/test_node_ref_cpu.py asserts the whole set)."""
    ip = np.asarray(in_ptr, dtype=np.int64)
    out = set()
    for lo, hi in zip(ip[:-1], ip[1:]):
        if hi == lo:
            out.add("empty on a boundary" if lo % ce == 0 else "empty inside a chunk")
            continue
        span = (hi - 1) // ce - lo // ce + 1
        out.add("spans %d" % span)
        if lo % ce == 0:
            out.add("starts on a boundary")
        if hi % ce == 0:
            out.add("ends on a boundary")
    return out


# ------------------------------------------------------------------------------------------------- launch shapes
TILE = 16
SPLIT_MAX_TILES = 320    # agdiff_params_t.tune_node_split_max_tiles
LDSW_MIN_TILES = 1536    # agdiff_params_t.tune_node_ldsw_min_tiles
CUS = 256


def _tune(tuning, key, default):
    v = int((tuning or {}).get(key, 0))
    return v if v != 0 else default


def _waves(tiles, ldsw_min):
    return 4 if tiles < ldsw_min else min(16, (tiles + 255) // 256)


def _tail(n, tiles, waves, wgs):
    """The last workgroup of a one-tile-per-wave launch: (waves with a tile, waves without one, valid nodes of the last tile)."""
    live = tiles - (wgs - 1) * waves
    return live, waves - live, n - (tiles - 1) * TILE


def node_stage_launch(n, tuning=None):
    """agdiff_schnet_node_stage_split's choice for `n` nodes: dict(variant = "split" | "stream" | "ldsw", tiles, waves per
    workgroup, workgroups, last_live / last_idle waves of the last workgroup, last_valid nodes of the last tile)."""
    tiles = (n + TILE - 1) // TILE
    if tiles <= _tune(tuning, "node_split_max_tiles", SPLIT_MAX_TILES):
        return dict(variant="split", tiles=tiles, waves=4, workgroups=tiles, last_live=4, last_idle=0, last_valid=n - (tiles - 1) * TILE)
    ldsw_min = _tune(tuning, "node_ldsw_min_tiles", LDSW_MIN_TILES)
    waves = _waves(tiles, ldsw_min)
    wgs = (tiles + waves - 1) // waves
    live, idle, valid = _tail(n, tiles, waves, wgs)
    return dict(variant="ldsw" if tiles >= ldsw_min else "stream", tiles=tiles, waves=waves, workgroups=wgs, last_live=live,
                last_idle=idle, last_valid=valid)


def gin_launch(n, precision_local, tuning=None):
    """agdiff_gin_encoder's choice: dict(variant = "stream" | "ldsw" | "persistent", tiles, waves, workgroups, rounds = the
    most tiles one wave walks, second_round_tiles, last_* as node_stage_launch, gather_workgroups)."""
    tiles = (n + TILE - 1) // TILE
    ldsw_min = _tune(tuning, "node_ldsw_min_tiles", LDSW_MIN_TILES)
    waves = _waves(tiles, ldsw_min)
    ldsw = tiles >= ldsw_min
    wgs = (tiles + waves - 1) // waves
    live, idle, valid = _tail(n, tiles, waves, wgs)
    persistent = ldsw and wgs > CUS and precision_local != "f32"
    out = dict(variant="persistent" if persistent else "ldsw" if ldsw else "stream", tiles=tiles, waves=waves, workgroups=wgs,
               rounds=1, second_round_tiles=0, last_live=live, last_idle=idle, last_valid=valid,
               gather_workgroups=((n + 7) // 8 + 7) // 8 * 8)
    if persistent:
        stride = CUS * waves
        out.update(workgroups=CUS, rounds=(tiles + stride - 1) // stride, second_round_tiles=max(0, min(tiles, 2 * stride) - stride))
    return out


def gather_passes(deg_even, deg_odd):
    """32-slot passes k_gin_gather makes for a half-wave pair: both halves walk the larger degree."""
    return (max(int(deg_even), int(deg_odd)) + 31) // 32


# ------------------------------------------------------------------------------------------------- batches
def tiled_batch(n, mol=8, seed=0):
    """`n` atoms as n // mol copies of one `mol`-atom molecule plus one molecule with the remaining atoms, raw bonds (no order
    extension: the lists stay short, so a float64 [L, 128] message array of 65,537 atoms stays in the low hundreds of MB).
    dict: atom_type (node_ref.atom_types), bond_index, bond_type, batch, num_graphs."""
    from agdiff_amd import synth
    rng = np.random.default_rng(8000 + seed)
    copies, rest = divmod(n, mol)
    rs, cs, ts, bs, off, g = [], [], [], [], 0, 0
    if copies:
        _, r, c, t = synth.random_molecule(rng, mol, raw_bonds=True)
        _, r2, c2, t2, b2 = synth.repeat_molecule(np.zeros(mol, dtype=np.int64), r, c, t, copies)
        rs.append(r2); cs.append(c2); ts.append(t2); bs.append(b2)
        off, g = copies * mol, copies
    if rest:
        if rest > 1:
            _, r, c, t = synth.random_molecule(rng, rest, raw_bonds=True)
            rs.append(r + off); cs.append(c + off); ts.append(t)
        bs.append(np.full(rest, g, dtype=np.int64))
        g += 1
    cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, dtype=np.int64)
    return dict(atom_type=atom_types(n), bond_index=np.stack([cat(rs), cat(cs)]), bond_type=cat(ts), batch=cat(bs), num_graphs=g)
