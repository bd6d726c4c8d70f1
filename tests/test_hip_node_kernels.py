"""GPU (MI355X): the dense per-node kernels of csrc/node.hip -- k_schnet_node_stage<MODE, LDSW>, k_schnet_node_stage_split<MODE,
FINISH, PREP>, k_gin_gather, k_gin_layer<MODE, LDSW>, k_gin_layer_persistent<MODE> -- each through its C-ABI entry point
(agdiff_schnet_node_stage_split, agdiff_gin_encoder) on a workspace the library sized, compared with the float64 restatement
of tests/node_ref.py (anchored on the CPU by tests/test_node_ref_cpu.py).

Inputs are injected, not network state: seeded unit-scale h / agg / agg_first (attribute rows at 0.3) are copied into ws.h,
ws.agg, ws.agg_first, ws.in_ptr, ws.agg_loc, ws.agg_first_loc, ws.h0 and ws.l_attr_rows; every output buffer starts at a
sentinel and every input the launch must not read at NaN; ws.variant_log is zeroed before and asserted after every launch.
The variants are selected through model.tuning (agdiff_params_t.tune_*), the shapes are those tests/test_node_ref_cpu.py checks
against the launchers' restated rules.  Atom types walk the whole embedding table.  Every comparison: helpers.check_close at the
mode's own gates with scale = 1.  (Every Workspace has agg_loc / agg_first_loc, whatever radius_poly says: the models here run
with radius_poly = "off", which packs fastest.)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import node_ref as NR
import step_ref as R
from helpers import check_close, t

pytestmark = pytest.mark.gpu
PRECISIONS = ["f32", "bf16x3", "f16x3"]
SENTINEL = -777.25
NAN = float("nan")
FORCE_STREAM = {"node_split_max_tiles": -1}
FORCE_LDSW = {"node_split_max_tiles": -1, "node_ldsw_min_tiles": 1}
# variant -> (model.tuning, the bit agdiff_schnet_node_stage_split must log)
STAGE_VARIANTS = {"split": ({}, "AGDIFF_VAR_NODE_SPLIT4"), "stream": (FORCE_STREAM, "AGDIFF_VAR_NODE_STREAM"),
                  "ldsw": (FORCE_LDSW, "AGDIFF_VAR_NODE_LDSW")}
GIN_VARIANTS = {"stream": {}, "ldsw": FORCE_LDSW}


# ------------------------------------------------------------------------------------------------- models and batches
@functools.lru_cache(maxsize=None)
def _model(precision, layers=4):
    """One model per (num_convs_local, precision) with the synthetic checkpoint of node_ref.state_dict; both branches in
    `precision` (the GIN layers run in agdiff_params_t.precision_local)."""
    from agdiff_amd import _lib, drugs_model_config, get_model
    cfg = drugs_model_config(num_convs_local=layers)
    m = get_model(cfg)
    m.precision, m.precision_local, m.radius_poly = precision, precision, "off"
    m.load_state_dict({k: v.clone() for k, v in NR.state_dict(cfg).items()}, strict=True)
    m = m.to("cuda:0").eval()
    pk = m.packed()
    assert (m.effective_precision, m.effective_precision_local) == (precision, precision)
    assert pk.struct.num_convs_local == layers and pk.struct.num_convs == cfg.num_convs
    return m, cfg, _lib.load()


@functools.lru_cache(maxsize=None)
def _sd64(layers=4):
    """The checkpoint in float64 (the embedding rows of encoder_global are the model's business: Case.sd64)."""
    from agdiff_amd import drugs_model_config
    return NR.to64(NR.state_dict(drugs_model_config(num_convs_local=layers)))


def _odd_batch():
    """85 atoms (odd), order extension: the dendrimer and a 32-atom molecule -- 864 local edges, room for the synthetic lists."""
    from agdiff_amd import synth
    at, r, c, ty = R.dendrimer()
    _, r2, c2, t2 = synth.random_molecule(np.random.default_rng(8100), 32, raw_bonds=True)
    n = at.shape[0] + 32
    return dict(atom_type=NR.atom_types(n), bond_index=np.stack([np.concatenate([r, r2 + 53]), np.concatenate([c, c2 + 53])]),
                bond_type=np.concatenate([ty, t2]), batch=np.repeat([0, 1], [53, 32]), num_graphs=2, extend_order=True)


@functools.lru_cache(maxsize=None)
def _batch(name):
    if name == "dendrimer":                  # step_ref's batch: 52-edge centre, order extension; 53 + 31 + 1 + 2 + 23 atoms
        b = dict(R.make_batch(name))
        b["atom_type"] = NR.atom_types(b["atom_type"].shape[0])
        return b
    if name == "odd":
        return _odd_batch()
    n = int(name[1:])                        # "n37": one molecule (n <= 64) or copies of an 8-atom molecule and a remainder
    return dict(NR.tiled_batch(n, mol=n if n <= 64 else 8), extend_order=False)


class Case:
    """One batch on the device in one arithmetic mode: topology, a fresh workspace, the float64 checkpoint as the device holds
    it (embedding rows after the max_norm renorm of this batch's types)."""

    def __init__(self, precision, name, layers=4):
        from agdiff_amd import _lib
        self.m, self.cfg, self.lib = _model(precision, layers)
        self.precision, self.name, self.layers = precision, name, layers
        b = self.b = _batch(name)
        at = t(b["atom_type"]).cuda()
        with torch.no_grad():
            self.m.tuning = {}
            self.m._renorm_embedding(at)
            self.topo, self.ws = self.m._batch(at, t(b["bond_index"]), t(b["bond_type"]), t(b["batch"]), b["num_graphs"], b["extend_order"])
        self.m._batch_cache = None           # (the topology may be edited below: nobody else gets to see it)
        self.N, self.L = self.topo.N, self.topo.L
        assert self.N == b["atom_type"].shape[0]
        self.T, self.W = ctypes.byref(self.topo.struct), ctypes.byref(self.ws.struct)
        self.z = b["atom_type"]
        self.sd64 = dict(_sd64(layers))
        emb = self.m.encoder_global.embedding.weight.detach().double().cpu()
        for k in ("encoder_global.embedding.weight", "model_global.1.embedding.weight"):
            self.sd64[k] = emb
        self.ce = _lib.TILE * self.lib.agdiff_conv_chunk_tiles(ctypes.c_int64(self.topo.max_edges))
        self.ce_loc = _lib.TILE * self.lib.agdiff_conv_chunk_tiles(ctypes.c_int64(self.topo.Lp))

    def params(self, tuning):
        self.m.tuning = dict(tuning)
        pk = self.m.packed()                 # (the cached pack: only the tune_* fields change)
        self.m.tuning = {}
        return pk

    # --------------------------------------------------------------------------------------------- node stage
    def stage(self, k, split, variant, *, h=None, agg=None, in_ptr=None, agg_first=None, agg_loc=None, agg_first_loc=None,
              h0=None, tuning=None):
        """One launch of agdiff_schnet_node_stage_split(k, split).  Arrays given are copied in, every other buffer of the stage
        is a sentinel (outputs) or NaN (inputs).  Returns dict(h, xs, h0, xs0) as float32 arrays."""
        from agdiff_amd import _lib
        ws, N = self.ws, self.N

        def put(buf, x, fill):
            buf.fill_(fill)
            if x is not None:
                assert x.size <= buf.numel()
                buf.view(-1)[: x.size].copy_(t(np.ascontiguousarray(x, dtype=np.float32)).cuda().view(-1))

        put(ws.h, h, SENTINEL)
        put(ws.xs, None, SENTINEL)
        put(ws.xs0, None, SENTINEL)
        put(ws.h0, h0, SENTINEL)
        put(ws.agg, agg, NAN)
        put(ws.agg_first, agg_first, NAN)
        put(ws.agg_loc, agg_loc, NAN)
        put(ws.agg_first_loc, agg_first_loc, NAN)
        ws.in_ptr.zero_()                    # (complete rows: not read; read by mistake, every list would be empty)
        if in_ptr is not None:
            assert in_ptr.shape[0] == N + 1 and 0 <= in_ptr.min() and in_ptr[-1] <= self.topo.max_edges
            assert (in_ptr[-1] - 1) // self.ce < ws.agg_first.numel() // 192
            ws.in_ptr.copy_(t(in_ptr.astype(np.int32)).cuda())
        agg_before = ws.agg.clone()
        tune, bit = STAGE_VARIANTS[variant] if tuning is None else (tuning, STAGE_VARIANTS[variant][1])
        pk = self.params(tune)
        ws.variant_log.zero_()
        rc = self.lib.agdiff_schnet_node_stage_split(ctypes.byref(pk.struct), self.T, self.W, k, split, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        assert int(ws.variant_log.item()) == _lib.DEFINES[bit], (variant, hex(int(ws.variant_log.item())))
        assert torch.equal(agg_before.view(torch.int32), ws.agg.view(torch.int32))              # inputs are read only
        out = {key: getattr(ws, key).view(N, -1).cpu().numpy().copy() for key in ("h", "xs", "h0", "xs0")}
        return out

    def check_stage(self, what, out, k, h_in, agg, h_key="h", xs_key="xs", ref=None):
        """h, h - h_in and xs of a launch against node_ref.stage (or `ref`, a result of it computed before); xs keeps its
        sentinel at k = num_convs."""
        h_ref, xs_ref = ref or NR.stage(self.sd64, self.cfg, k, h_in, agg, self.z)
        tag = "%s k=%d[%s]" % (what, k, self.name)
        assert np.isfinite(out[h_key]).all()
        check_close("node h " + tag, out[h_key], h_ref, self.precision)
        if k:
            h64 = np.asarray(h_in, dtype=np.float64)
            check_close("node h-h_in " + tag, out[h_key].astype(np.float64) - h64, h_ref.numpy() - h64, self.precision)
        if xs_ref is None:
            assert np.all(out[xs_key] == SENTINEL)
        else:
            check_close("node xs " + tag, out[xs_key], xs_ref, self.precision)

    # --------------------------------------------------------------------------------------------- GIN encoder
    def gin(self, rows, rows_per_canonical_edge, variant, named=None):
        """One call of agdiff_gin_encoder.  `rows` [R, 128] go to ws.l_attr_rows -- with `named` (row indices) only those rows,
        NaN everywhere else; ws.hl starts at the sentinel, ws.hl2 at NaN.  Returns ws.hl as a float32 array [N, 128]."""
        from agdiff_amd import _lib
        ws, N = self.ws, self.N
        ws.hl.fill_(SENTINEL)
        ws.hl2.fill_(NAN)
        buf = ws.l_attr_rows.view(-1, 128)
        assert rows.shape[0] <= buf.shape[0]
        buf.fill_(NAN)
        dev = t(np.ascontiguousarray(rows, dtype=np.float32)).cuda()
        if named is None:
            buf[: rows.shape[0]].copy_(dev)
        else:
            idx = torch.from_numpy(np.unique(named)).cuda()
            buf[idx] = dev[idx]
        pk = self.params(GIN_VARIANTS[variant])
        want = NR.gin_launch(N, self.precision, GIN_VARIANTS[variant])
        ws.variant_log.zero_()
        rc = self.lib.agdiff_gin_encoder(ctypes.byref(pk.struct), self.T, self.W, rows_per_canonical_edge, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        assert int(ws.variant_log.item()) == (_lib.DEFINES["AGDIFF_VAR_GIN_LDSW"] if want["variant"] != "stream" else 0)
        out = ws.hl.view(N, 128).cpu().numpy().copy()
        assert np.isfinite(out).all() and not np.any(out == SENTINEL)
        return out

    def own_lists(self):
        """The topology's in-lists as the kernel reads them: (in_ptr, in_src, {1: in_row, 0: in_eid})."""
        g = lambda x: x.cpu().numpy().astype(np.int64)
        return g(self.topo.loc_in_ptr), g(self.topo.loc_in_src), {1: g(self.topo.loc_in_row), 0: g(self.topo.loc_in_eid)}


@functools.lru_cache(maxsize=3)
def _case(precision, name, layers=4):
    return Case(precision, name, layers)


@functools.lru_cache(maxsize=None)
def _draws(name, n):
    """Seeded h and agg of batch `name` (returned arrays are not modified)."""
    return NR.draw("h:" + name, (n, 128)), NR.draw("agg:" + name, (n, 192))


@functools.lru_cache(maxsize=8)
def _drawn_reference(name, n, k):
    """node_ref.stage(k >= 1) on the seeded h and complete-row agg of batch `name`, computed once for the three modes (a stage
    past 0 does not read the embedding, the one tensor a model changes)."""
    from agdiff_amd import drugs_model_config
    assert k >= 1
    return NR.stage(_sd64(), drugs_model_config(), k, *_draws(name, n), _batch(name)["atom_type"])


# ------------------------------------------------------------------------------------------------- node stage
@pytest.mark.parametrize("n,k", [(37, k) for k in range(7)] + [(1, 3), (16, 3)])
@pytest.mark.parametrize("variant", list(STAGE_VARIANTS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_stage_in_every_variant(precision, variant, n, k):
    """1.  k = 0 .. num_convs with complete-row aggregates (split bit 1) on 37 atoms -- two full tiles and a 5-node tile; the
    streaming workgroup's fourth wave has no tile --, and k = 3 on 1 and 16 atoms.  Stages 2 to 6 select the packs of blocks
    1 to 5; the last stage is FINISH && !PREP and leaves ws.xs alone."""
    c = _case(precision, "n%d" % n)
    assert c.cfg.num_convs == 6
    assert NR.node_stage_launch(n, STAGE_VARIANTS[variant][0])["variant"] == variant
    h_in, agg = _draws(c.name, n)
    out = c.stage(k, 1 if k else 0, variant, h=h_in if k else None, agg=agg if k else None)
    c.check_stage(variant, out, k, h_in, agg)
    assert np.all(out["h0"] == SENTINEL) and np.all(out["xs0"] == SENTINEL)


@pytest.mark.parametrize("k", [3, 6])
@pytest.mark.parametrize("n", [4099, 65537])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_idle_waves_walk_the_staging_phases(precision, n, k):
    """2.  Forced LDS-shared: 257 tiles in two-wave workgroups -- the last one has a wave with 3 valid nodes and a wave without a
    tile --, and 4,097 tiles in sixteen-wave workgroups, the last with one live node and fifteen idle waves, which still
    take part in every copy and barrier of the three staging phases."""
    shape = NR.node_stage_launch(n, FORCE_LDSW)
    assert (shape["variant"], shape["last_live"], shape["last_idle"], shape["last_valid"]) == \
        (("ldsw", 1, 1, 3) if n == 4099 else ("ldsw", 1, 15, 1))
    c = _case(precision, "n%d" % n)
    h_in, agg = _draws(c.name, n)
    c.check_stage("ldsw", c.stage(k, 1, "ldsw", h=h_in, agg=agg), k, h_in, agg, ref=_drawn_reference(c.name, n, k))


@pytest.mark.parametrize("n,variant", [(5120, "split"), (5121, "stream"), (24561, "ldsw")])
def test_the_library_thresholds_select_the_variants(n, variant):
    """3.  tuning = {}: 320 tiles run four waves per tile, 321 stream, 1,536 share the weights through LDS (six waves)."""
    assert NR.node_stage_launch(n)["variant"] == variant
    c = _case("f16x3", "n%d" % n)
    h_in, agg = _draws(c.name, n)
    c.check_stage("natural " + variant, c.stage(3, 1, variant, h=h_in, agg=agg, tuning={}), 3, h_in, agg, ref=_drawn_reference(c.name, n, 3))


@pytest.mark.parametrize("variant", list(STAGE_VARIANTS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunked_aggregates(precision, variant):
    """4.  split = 0: a synthetic ws.in_ptr whose lists start on a chunk boundary, end exactly on one, lie inside one chunk, span
    three and four chunks, or are empty -- also with lo on a boundary; an empty list's agg row and every agg_first row no list
    refers to hold NaN."""
    c = _case(precision, "n37")
    n = c.N
    ptr = NR.chunked_in_ptr(n, c.ce, c.topo.max_edges)
    assert NR.list_shapes(ptr, c.ce) == {"empty on a boundary", "empty inside a chunk", "starts on a boundary", "ends on a boundary",
                                         "spans 1", "spans 3", "spans 4"}
    h_in, agg = _draws(c.name, n)
    chunks = c.ws.agg_first.numel() // 192
    first = NR.draw("agg_first:n37", (chunks, 192))
    read = NR.chunks_read(ptr, c.ce)
    first[np.setdiff1d(np.arange(chunks), read)] = NAN
    agg = agg.copy()
    agg[np.diff(ptr) == 0] = NAN
    total = NR.gathered_aggregate(ptr, agg, first, c.ce)
    assert bool(torch.isfinite(total).all()) and len(read) >= 10
    c.check_stage("chunked " + variant, c.stage(2, 0, variant, h=h_in, agg=agg, in_ptr=ptr, agg_first=first), 2, h_in, total)


@pytest.mark.parametrize("variant", list(STAGE_VARIANTS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_passes(precision, variant):
    """5.  split = 1 | 8: complete rows in ws.agg plus the local pass in ws.agg_loc / ws.agg_first_loc over the topology's own
    lp_ptr (order extension: padded lists of 8 to 52 entries, 49 later-chunk references at the library's 16-edge chunks).  The
    atom without a local edge has an empty list and a NaN row."""
    c = _case(precision, "dendrimer")
    n = c.N
    lp = c.topo.lp_ptr.cpu().numpy().astype(np.int64)
    read = NR.chunks_read(lp, c.ce_loc)
    assert len(read) >= 10 and (np.diff(lp) == 0).any() and lp[-1] == c.topo.Lp
    h_in, agg = _draws(c.name, n)
    agg_loc = NR.draw("agg_loc", (n, 192))
    agg_loc[np.diff(lp) == 0] = NAN
    chunks = c.ws.agg_first_loc.numel() // 192
    assert (lp[-1] - 1) // c.ce_loc < chunks
    first_loc = NR.draw("agg_first_loc", (chunks, 192))
    first_loc[np.setdiff1d(np.arange(chunks), read)] = NAN
    total = t(agg).double() + NR.gathered_aggregate(lp, agg_loc, first_loc, c.ce_loc)
    out = c.stage(4, 1 | 8, variant, h=h_in, agg=agg, agg_loc=agg_loc, agg_first_loc=first_loc)
    c.check_stage("two passes " + variant, out, 4, h_in, total)


@pytest.mark.parametrize("variant", list(STAGE_VARIANTS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_stage0_cache(precision, variant):
    """6.  k = 0 with split bit 4 writes ws.h0 / ws.xs0 and leaves ws.h / ws.xs alone; k = 1 with bit 2 takes the residual input
    from ws.h0 while writing ws.h."""
    c = _case(precision, "n37")
    h_in, agg = _draws(c.name, c.N)
    out = c.stage(0, 4, variant)
    assert np.all(out["h"] == SENTINEL) and np.all(out["xs"] == SENTINEL)
    c.check_stage("cache write " + variant, out, 0, None, None, h_key="h0", xs_key="xs0")
    out = c.stage(1, 1 | 2, variant, h0=h_in, agg=agg)          # (ws.h holds the sentinel: a residual read from it shows)
    assert np.array_equal(out["h0"], h_in) and np.all(out["xs0"] == SENTINEL)
    c.check_stage("cache read " + variant, out, 1, h_in, agg)


@pytest.mark.parametrize("variant", list(STAGE_VARIANTS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_stage_rows_are_independent_and_launches_repeat(precision, variant):
    """7.  With one node's h and agg changed exactly that node's rows of h / xs change, bit for bit (nodes of a full tile, of
    the partial tile, the first and the last); ws.agg is unchanged after every launch (Case.stage); two identical launches give
    identical bits."""
    c = _case(precision, "n37")
    h_in, agg = _draws(c.name, c.N)
    bits = lambda o: (o["h"].view(np.int32), o["xs"].view(np.int32))
    base = bits(c.stage(3, 1, variant, h=h_in, agg=agg))
    again = bits(c.stage(3, 1, variant, h=h_in, agg=agg))
    assert np.array_equal(base[0], again[0]) and np.array_equal(base[1], again[1])
    for node in (0, 21, 33, 36):
        h2, a2 = h_in.copy(), agg.copy()
        h2[node] = -1.5 * h2[node] + 0.25
        a2[node] = -1.5 * a2[node] + 0.25
        got = bits(c.stage(3, 1, variant, h=h2, agg=a2))
        other = np.arange(c.N) != node
        for b0, b1 in zip(base, got):
            assert np.array_equal(b0[other], b1[other]), node
            assert not np.array_equal(b0[node], b1[node]), node


# ------------------------------------------------------------------------------------------------- GIN encoder
@functools.lru_cache(maxsize=2)
def _synthetic(precision, layers):
    """A private batch whose in-lists are overwritten IN PLACE (the device pointers of agdiff_topo_t stay) with
    node_ref.synthetic_in_lists; not shared with any other test."""
    c = Case(precision, "odd", layers)
    topo = c.topo
    lists = NR.synthetic_in_lists(c.N, c.L)
    total = int(lists["in_ptr"][-1])
    assert c.N % 2 == 1 and total <= c.L == topo.loc_in_src.numel() == topo.loc_in_row.numel() == topo.loc_in_eid.numel()
    assert c.L <= c.ws.l_attr_rows.numel() // 128 and lists["in_src"].max() < c.N
    assert max(lists["in_row"].max(), lists["in_eid"].max()) < c.L
    dev = lambda x: t(np.ascontiguousarray(x).astype(np.int32)).cuda()
    topo.loc_in_ptr.copy_(dev(lists["in_ptr"]))
    for name, key in (("loc_in_src", "in_src"), ("loc_in_row", "in_row"), ("loc_in_eid", "in_eid")):
        buf = getattr(topo, name)
        buf.zero_()                           # (slots past the synthetic total: never read)
        buf[:total].copy_(dev(lists[key]))
    c.m._batch_cache = None
    return c, lists, NR.draw("rows:odd", (c.L, 128), NR.ATTR_STD)


@functools.lru_cache(maxsize=None)
def _synthetic_reference(layers, table):
    from agdiff_amd import drugs_model_config
    b = _batch("odd")
    n = b["atom_type"].shape[0]
    L = 864
    lists = NR.synthetic_in_lists(n, L)
    rows = NR.draw("rows:odd", (L, 128), NR.ATTR_STD)
    cfg = drugs_model_config(num_convs_local=layers)
    return NR.gin(_sd64(layers), cfg, b["atom_type"], lists["in_ptr"], lists["in_src"], lists[table], rows)


@pytest.mark.parametrize("table", ["in_row", "in_eid"])
@pytest.mark.parametrize("variant", list(GIN_VARIANTS))
@pytest.mark.parametrize("layers", [4, 3, 1])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gin_on_in_lists_written_as_data(precision, layers, variant, table):
    """8.  Half-wave pairs of k_gin_gather with degrees node_ref.PAIR_DEGREES -- a list past 32, 64 or 96 slots next to a short or
    an empty one, in both orders --, an odd node count, sources that repeat and include the node itself, different rows in
    the row and the eid table (rows_per_canonical_edge = 1 / 0), NaN in every attribute row the table in use does not name and
    in ws.hl2; 4, 3 and 1 layers: the ping-pong must end in ws.hl for odd and even counts."""
    c, lists, rows = _synthetic(precision, layers)
    assert c.L == 864
    out = c.gin(rows, 1 if table == "in_row" else 0, variant, named=lists[table])
    check_close("gin synthetic %d layers %s %s" % (layers, variant, table), out, _synthetic_reference(layers, table), precision)


@pytest.mark.parametrize("variant", list(GIN_VARIANTS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gin_rows_are_independent(precision, variant):
    """8, one layer (a change then reaches its receivers only).  The attribute row of the hub's 100th message changed: exactly the hub's
    row changes.  The atom type of the leaf that sends this message (and no other) changed: exactly the leaf's and the hub's rows
    change.  Two identical calls give identical bits."""
    c, lists, rows = _synthetic(precision, 1)
    bits = lambda rows_: c.gin(rows_, 1, variant, named=lists["in_row"]).view(np.int32)
    base = bits(rows)
    assert np.array_equal(base, bits(rows))
    r2 = rows.copy()
    r2[lists["in_row"][lists["hub_last_slot"]]] += 0.5
    got = bits(r2)
    changed = np.nonzero((got != base).any(axis=1))[0]
    assert changed.tolist() == [NR.HUB]
    leaf = lists["leaf"]
    old = c.topo.atom_type[leaf].item()
    try:
        c.topo.atom_type[leaf] = (old + 50) % 100
        got = bits(rows)
    finally:
        c.topo.atom_type[leaf] = old
    changed = np.nonzero((got != base).any(axis=1))[0]
    assert changed.tolist() == sorted([NR.HUB, leaf])
    assert np.array_equal(base, bits(rows))


@functools.lru_cache(maxsize=None)
def _own_reference(name, rpce, n_rows):
    """float64 GIN output of batch `name` on its topology's own lists (host build: the same lists as on the device)."""
    from agdiff_amd.topology import BatchTopology
    b = _batch(name)
    topo = BatchTopology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], num_graphs=b["num_graphs"],
                         extend_order=b["extend_order"], device="cpu")
    g = lambda x: x.numpy().astype(np.int64)
    table = g(topo.loc_in_row) if rpce else g(topo.loc_in_eid)
    rows = NR.draw("rows:" + name, (n_rows, 128), NR.ATTR_STD)
    from agdiff_amd import drugs_model_config
    return NR.gin(_sd64(4), drugs_model_config(), b["atom_type"], g(topo.loc_in_ptr), g(topo.loc_in_src), table, rows)


def _check_own_lists(c, rpce, variant):
    """agdiff_gin_encoder on the batch's untouched topology with random rows, against node_ref.gin on the lists read back."""
    ptr, src, tables = c.own_lists()
    n_rows = c.ws.l_attr_rows.numel() // 128
    assert tables[rpce].max() < n_rows
    rows = NR.draw("rows:" + c.name, (n_rows, 128), NR.ATTR_STD)
    out = c.gin(rows, rpce, variant, named=tables[rpce])
    ref = _own_reference(c.name, rpce, n_rows)
    check_close("gin %s rows_per_canonical_edge=%d %s" % (c.name, rpce, variant), out, ref, c.precision)
    return ptr


@pytest.mark.parametrize("rpce", [1, 0])
@pytest.mark.parametrize("variant", list(GIN_VARIANTS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gin_on_a_real_hub(precision, variant, rpce):
    """9.  step_ref's dendrimer batch, order extension: the centre has 52 in-edges in the lists topology.py builds."""
    c = _case(precision, "dendrimer")
    ptr = _check_own_lists(c, rpce, variant)
    assert ptr[1] - ptr[0] == 52


@pytest.mark.parametrize("n", [24561, 65537])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gin_large_shapes(precision, n):
    """10.  1,536 tiles: LDS-shared by the library's own threshold, six waves.  4,097 tiles in 257 sixteen-wave workgroups: the
    persistent kernel in the split modes -- 256 workgroups, one wave takes a second round, which holds a single node --,
    k_gin_layer<f32, true> with fifteen idle waves in exact fp32."""
    shape = NR.gin_launch(n, precision)
    if n == 24561:
        assert (shape["variant"], shape["waves"]) == ("ldsw", 6)
    else:
        assert shape["variant"] == ("ldsw" if precision == "f32" else "persistent")
        assert precision == "f32" or (shape["rounds"], shape["second_round_tiles"], shape["last_valid"]) == (2, 1, 1)
    c = _case(precision, "n%d" % n)
    _check_own_lists(c, 1, "stream")         # (tuning = {}: the library's own choice)
