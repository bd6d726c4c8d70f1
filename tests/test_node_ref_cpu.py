"""CPU: tests/node_ref.py (the float64 restatement tests/test_hip_node_kernels.py compares the node stage and the GIN encoder of
csrc/node.hip with) anchored against the oracle in float64 and against the reference project's recorded stage outputs; its
seeded inputs shown to be well conditioned (plain float32 stays within a quarter of the "f32" gates) and its comparisons shown
to be sensitive (every mutation listed below moves a compared tensor past ten times the loosest gate); the launch shapes of the
GPU tests against the launchers' restated rules."""
import functools

import numpy as np
import pytest
import torch

import node_ref as NR
from helpers import FORWARD_CASES, TOL_ELEM, TOL_NORM, check_close, elem_err, load_golden, rel_err, t
from oracle import agdiff_oracle as O
from test_hip_kernels import _agg_ref

TIGHT = 1e-12            # two float64 evaluations of the same sums, in different orders
N_COND = 1000


@functools.lru_cache(maxsize=None)
def _sd(kind="drugs", layers=4):
    from agdiff_amd import drugs_model_config, qm9_model_config
    cfg = (drugs_model_config if kind == "drugs" else qm9_model_config)(num_convs_local=layers)
    sd = NR.state_dict(cfg)
    return cfg, sd, NR.to64(sd)


def _random_graph(seed, n, edges_per_node=7):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, size=edges_per_node * n)
    dst = (src + rng.integers(1, n, size=src.shape[0])) % n
    keep = dst < n - 2                                               # (the last two nodes receive nothing)
    src, dst = src[keep], dst[keep]
    length = rng.uniform(0.5, 11.0, size=src.shape[0])              # some beyond the cutoff
    attr = rng.standard_normal((src.shape[0], 128)) * NR.ATTR_STD
    return dict(edge_index=np.stack([src, dst]), edge_length=length, edge_attr=attr), rng


# ------------------------------------------------------------------------------------------------- oracle parity
@pytest.mark.parametrize("kind", ["drugs", "qm9"])
def test_stage_equals_the_oracles_blocks_in_float64(kind):
    """Stage by stage along the whole encoder on a random graph: xs of stage k feeds the aggregate of block k (the host
    decomposition test_hip_kernels._agg_ref, float64), stage k + 1 finishes the block; every h against h + adaptive_scaling(
    interaction_block(h)) of the oracle, the last against schnet_encoder."""
    cfg, _, sd = _sd(kind)
    sd = {k: v.clone() for k, v in sd.items()}
    n = 61
    g, rng = _random_graph(3, n)
    z = NR.atom_types(n)
    ei, elen, ea = t(g["edge_index"]), t(g["edge_length"]).unsqueeze(-1), t(g["edge_attr"])      # ([E, 1], as the encoder gets it)
    want = O.schnet_encoder(sd, "encoder_global", t(z), ei, elen, ea, cfg)        # (renorms the embedding rows of sd in place)
    h, xs = NR.stage(sd, cfg, 0, None, None, z)
    assert torch.equal(h, sd["encoder_global.embedding.weight"][t(z)]) and float(h.norm(dim=1).max()) <= 10.0 + 1e-9
    for k in range(cfg.num_convs):
        blk = "encoder_global.interactions.%d" % k
        agg = _agg_ref(sd, cfg, blk, g, xs)
        ref = h + O.adaptive_scaling(sd, "encoder_global.scaling_modules.%d" % k,
                                     O.interaction_block(sd, blk, h, ei, elen, ea, cfg.cutoff, cfg.smooth_conv))
        h_new, xs = NR.stage(sd, cfg, k + 1, h, agg, z)
        assert rel_err(h_new - h, ref - h) < TIGHT and rel_err(h_new, ref) < TIGHT, k
        assert (xs is None) == (k + 1 == cfg.num_convs)
        h = h_new
    assert rel_err(h, want) < TIGHT


@pytest.mark.parametrize("layers", [4, 3, 1])
def test_gin_equals_the_oracles_encoder_in_float64(layers):
    cfg, _, sd = _sd("drugs", layers)
    assert [float(sd["encoder_local.convs.%d.eps" % k]) for k in range(layers)] == list(NR.GIN_EPS[:layers])
    assert "encoder_local.convs.%d.eps" % layers not in sd
    n = 61
    g, rng = _random_graph(4, n)
    z = NR.atom_types(n)
    src, dst = g["edge_index"]
    want = O.gin_encoder(sd, "encoder_local", t(z), t(g["edge_index"]), t(g["edge_attr"]), cfg)
    perm = rng.permutation(src.shape[0])                              # rows in another order than the edges
    rows = np.empty_like(g["edge_attr"])
    rows[perm] = g["edge_attr"]
    ptr, in_src, in_row = NR.in_lists(n, src, dst, perm)
    assert rel_err(NR.gin(sd, cfg, z, ptr, in_src, in_row, rows), want) < TIGHT


# ------------------------------------------------------------------------------------------------- recorded fixtures
@pytest.mark.parametrize("case", ["g3_forward_qm9_small", "g3_forward_smooth_sparse"])
def test_reference_reproduces_the_recorded_stage_outputs(case):
    """schnet_h0, scaled_b0, schnet_out and gin_out of the reference project's forward fixtures (its own checkpoint: eps = 0),
    from the fixture's edges, lengths and edge_attr."""
    g = load_golden(case)
    cfg = FORWARD_CASES[case]()
    sd = O.synth_state_dict_for(cfg)
    O.embedding_renorm_(sd["encoder_global.embedding.weight"], t(g["atom_type"]))
    sd = NR.to64(sd)
    z = g["atom_type"]
    h, xs = NR.stage(sd, cfg, 0, None, None, z)
    check_close("node_ref schnet_h0[%s]" % case, h, g["schnet_h0"], "f32")
    for k in range(cfg.num_convs):
        agg = _agg_ref(sd, cfg, "encoder_global.interactions.%d" % k, g, xs)
        h_new, xs = NR.stage(sd, cfg, k + 1, h, agg, z)
        if k == 0:
            check_close("node_ref scaled_b0[%s]" % case, h_new - h, g["scaled_b0"], "f32")
        h = h_new
    check_close("node_ref schnet_out[%s]" % case, h, g["schnet_out"], "f32")
    lm = g["edge_type"] > 0
    ei = g["edge_index"][:, lm]
    ptr, in_src, in_row = NR.in_lists(z.shape[0], ei[0], ei[1], np.arange(ei.shape[1]))
    check_close("node_ref gin_out[%s]" % case, NR.gin(sd, cfg, z, ptr, in_src, in_row, g["edge_attr"][lm]), g["gin_out"], "f32")


# ------------------------------------------------------------------------------------------------- conditioning
def _gin_inputs(n=85, num_rows=1360):
    lists = NR.synthetic_in_lists(n, num_rows)
    return lists, NR.draw("rows", (num_rows, 128), NR.ATTR_STD), NR.atom_types(n)


def _quarter(name, got, ref):
    rn, re_ = rel_err(got, ref), elem_err(got, ref)
    print("float32 vs float64 %-28s normwise %.2e  elementwise %.2e" % (name, rn, re_))
    assert rn < TOL_NORM["f32"] / 4 and re_ < TOL_ELEM["f32"] / 4, (name, rn, re_)


def test_plain_float32_stays_within_a_quarter_of_the_f32_gates():
    """The drawn inputs are fair to the project's gates: the same functions in plain float32 torch lie within a quarter of the
    "f32" gates of the float64 result -- h, h - h_in and xs at every k, and the GIN output of 4, 3 and 1 layers on the synthetic in-lists
    (degrees up to 100), through the row table and through the eid table."""
    cfg, sd32, sd64 = _sd()
    z = NR.atom_types(N_COND)
    h_in, agg = NR.draw("h", (N_COND, 128)), NR.draw("agg", (N_COND, 192))
    for k in range(cfg.num_convs + 1):
        h64, xs64 = NR.stage(sd64, cfg, k, h_in, agg, z)
        h32, xs32 = NR.stage(sd32, cfg, k, h_in, agg, z)
        assert h32.dtype == torch.float32 and h64.dtype == torch.float64
        _quarter("h k=%d" % k, h32, h64)
        if k:
            _quarter("h - h_in k=%d" % k, h32.double() - t(h_in).double(), h64 - t(h_in).double())
            assert float((h64 - t(h_in).double()).abs().max()) > 0.3           # the increment is of the order of h
        if xs64 is not None:
            _quarter("xs k=%d" % k, xs32, xs64)
    for layers in (4, 3, 1):
        cfg_l, sd32_l, sd64_l = _sd("drugs", layers)
        lists, rows, z85 = _gin_inputs()
        for table in ("in_row", "in_eid"):
            a = (z85, lists["in_ptr"], lists["in_src"], lists[table], rows)
            _quarter("gin %d layers %s" % (layers, table), NR.gin(sd32_l, cfg_l, *a), NR.gin(sd64_l, cfg_l, *a))


# ------------------------------------------------------------------------------------------------- sensitivity
LOOSEST = "bf16x3"


def _moved(name, got, ref):
    """A comparison of `got` with `ref` would fail at ten times the loosest gate."""
    rn, re_ = rel_err(got, ref), elem_err(got, ref)
    print("mutation %-44s normwise %.2e  elementwise %.2e" % (name, rn, re_))
    return rn > 10 * TOL_NORM[LOOSEST] or re_ > 10 * TOL_ELEM[LOOSEST]


def _stage_tensors(sd, cfg, k, h_in, agg, z, mutate=()):
    h, xs = NR.stage(sd, cfg, k, h_in, agg, z, mutate=mutate)
    out = {"h": h, "h - h_in": h - t(h_in).double()}
    if xs is not None:
        out["xs"] = xs
    return out


def _any_moved(name, got, ref):
    hits = [_moved("%s: %s" % (name, key), got[key], ref[key]) for key in ref]
    return any(hits)


def test_stage_mutations_move_a_compared_tensor_past_ten_times_the_loosest_gate():
    cfg, _, sd = _sd()
    n = 37
    z, h_in, agg = NR.atom_types(n), NR.draw("h", (n, 128)), NR.draw("agg", (n, 192))
    for k in range(1, cfg.num_convs + 1):
        ref = _stage_tensors(sd, cfg, k, h_in, agg, z)
        b = k - 1
        if b + 1 < cfg.num_convs:                                     # block b's fc.2 replaced by block b + 1's
            m = dict(sd)
            m["encoder_global.scaling_modules.%d.fc.2.weight" % b] = sd["encoder_global.scaling_modules.%d.fc.2.weight" % (b + 1)]
            assert _any_moved("fc.2 of block %d from block %d" % (b, b + 1), _stage_tensors(m, cfg, k, h_in, agg, z), ref)
        m = dict(sd)                                                  # the gate's second bias dropped
        m["encoder_global.interactions.%d.attention.2.bias" % b] = torch.zeros(1, dtype=torch.float64)
        assert _any_moved("gate bias of block %d dropped" % b, _stage_tensors(m, cfg, k, h_in, agg, z), ref)
        a2 = agg.copy()                                               # conv2's 64 aggregate columns zeroed
        a2[:, 128:] = 0.0
        assert _any_moved("conv2 columns zeroed, block %d" % b, _stage_tensors(sd, cfg, k, h_in, a2, z), ref)
        assert _any_moved("residual skipped on the last node, stage %d" % k,
                          _stage_tensors(sd, cfg, k, h_in, agg, z, mutate=("no_residual_last_node",)), ref)
    # one agg_first chunk left out (the chunked lists of the GPU test, stage 2)
    ce = 16
    ptr = NR.chunked_in_ptr(n, ce, 600)
    first = NR.draw("agg_first", (ptr[-1] // ce + 1, 192))
    ref = _stage_tensors(sd, cfg, 2, h_in, NR.gathered_aggregate(ptr, agg, first, ce), z)
    for c in NR.chunks_read(ptr, ce):
        f2 = first.copy()
        f2[c] = 0.0
        assert _any_moved("agg_first chunk %d left out" % c, _stage_tensors(sd, cfg, 2, h_in, NR.gathered_aggregate(ptr, agg, f2, ce), z), ref)


@pytest.mark.parametrize("layers", [4, 3, 1])
def test_gin_mutations_move_the_output_past_ten_times_the_loosest_gate(layers):
    cfg, _, sd = _sd("drugs", layers)
    lists, rows, z = _gin_inputs()
    a = (z, lists["in_ptr"], lists["in_src"], lists["in_row"], rows)
    ref = NR.gin(sd, cfg, *a)
    # the 33rd message of a 33-edge node dropped (node 13: the odd half of the pair (32, 33))
    node = 13
    assert lists["degree"][node] == 33 and lists["degree"][node - 1] == 32
    ptr = lists["in_ptr"].copy()
    ptr[node + 1:] -= 1
    drop = lists["in_ptr"][node + 1] - 1
    got = NR.gin(sd, cfg, z, ptr, np.delete(lists["in_src"], drop), np.delete(lists["in_row"], drop), rows)
    assert _moved("33rd message dropped", got, ref)
    assert _moved("33rd message dropped, its row alone", got[node], ref[node])
    m = dict(sd)                                                      # (1 + eps) replaced by 1
    for k in range(layers):
        m["encoder_local.convs.%d.eps" % k] = torch.zeros(1, dtype=torch.float64)
    assert _moved("(1 + eps) -> 1", NR.gin(m, cfg, *a), ref)
    assert _moved("relu after the last layer", NR.gin(sd, cfg, *a, mutate=("relu_last",)), ref)
    assert _moved("residual skipped on the last node", NR.gin(sd, cfg, *a, mutate=("no_residual_last_node",)), ref)
    # the row table and the eid table name different rows
    assert _moved("eid table for row table", NR.gin(sd, cfg, z, lists["in_ptr"], lists["in_src"], lists["in_eid"], rows), ref)


# ------------------------------------------------------------------------------------------------- aggregate sources
@pytest.mark.parametrize("ce", [16, 48, 128])
def test_gathered_aggregate_equals_a_per_edge_sum(ce):
    """agg / agg_first as the chunked CFConv leaves them, built from per-edge values: a chunk's edges of the list that started
    in an earlier chunk go to agg_first[chunk], every other edge to agg[its node]; gathered_aggregate must give back the per-node
    sums.  Rows nothing writes hold NaN."""
    rng = np.random.default_rng(100 + ce)
    n = 200
    deg = rng.choice([0, 0, 1, 3, ce // 2, ce, ce + 1, 2 * ce, 3 * ce + 5], size=n)
    ptr = np.concatenate([[0], np.cumsum(deg)])
    e = int(ptr[-1])
    val = rng.standard_normal((e, 192))
    owner = np.repeat(np.arange(n), deg)
    want = np.zeros((n, 192))
    np.add.at(want, owner, val)
    agg = np.full((n, 192), np.nan)
    agg[deg > 0] = 0.0
    first = np.full((e // ce + 2, 192), np.nan)
    first[NR.chunks_read(ptr, ce)] = 0.0
    for k in range(e):
        i = owner[k]
        if k // ce == ptr[i] // ce:
            agg[i] += val[k]
        else:
            first[k // ce] += val[k]
    got = NR.gathered_aggregate(ptr, agg, first, ce).numpy()
    assert not np.isnan(got).any() and rel_err(got, want) < TIGHT
    assert np.all(got[deg == 0] == 0.0)


def test_the_chunked_lists_cover_every_case():
    for ce in (16, 32):
        ptr = NR.chunked_in_ptr(37, ce, 40 * ce)
        assert NR.list_shapes(ptr, ce) == {"empty on a boundary", "empty inside a chunk", "starts on a boundary", "ends on a boundary",
                                           "spans 1", "spans 3", "spans 4"}
        unread = set(range(int(ptr[-1]) // ce + 1)) - set(NR.chunks_read(ptr, ce))
        assert unread and 0 in unread                                 # rows of agg_first that stay NaN in the GPU test


# ------------------------------------------------------------------------------------------------- launch shapes
FORCE_STREAM = {"node_split_max_tiles": -1}
FORCE_LDSW = {"node_split_max_tiles": -1, "node_ldsw_min_tiles": 1}


def test_the_shapes_reach_every_variant_and_every_tail():
    """The sizes of tests/test_hip_node_kernels.py against the launchers' rules (csrc/node.hip: agdiff_schnet_node_stage_split,
    agdiff_gin_encoder), restated in node_ref."""
    S, G = NR.node_stage_launch, NR.gin_launch
    pick = lambda d, *keys: tuple(d[k] for k in keys)
    # N = 37: two full tiles and a 5-node tile; the fourth wave of the streaming workgroup is idle
    assert pick(S(37), "variant", "tiles", "workgroups", "last_valid") == ("split", 3, 3, 5)
    assert pick(S(37, FORCE_STREAM), "variant", "waves", "workgroups", "last_live", "last_idle", "last_valid") == ("stream", 4, 1, 3, 1, 5)
    assert pick(S(37, FORCE_LDSW), "variant", "waves", "workgroups", "last_idle") == ("ldsw", 1, 3, 0)
    assert pick(S(1), "tiles", "last_valid") == (1, 1) and pick(S(16), "tiles", "last_valid") == (1, 16)
    # idle waves under barriers: 257 and 4,097 tiles, forced LDS-shared
    assert pick(S(4099, FORCE_LDSW), "variant", "tiles", "waves", "workgroups", "last_live", "last_idle", "last_valid") == \
        ("ldsw", 257, 2, 129, 1, 1, 3)
    assert pick(S(65537, FORCE_LDSW), "variant", "tiles", "waves", "workgroups", "last_live", "last_idle", "last_valid") == \
        ("ldsw", 4097, 16, 257, 1, 15, 1)
    assert S(65537)["variant"] == "ldsw" and S(65537) == S(65537, FORCE_LDSW)
    # natural thresholds
    assert pick(S(5120), "variant", "tiles") == ("split", 320)
    assert pick(S(5121), "variant", "tiles", "waves") == ("stream", 321, 4)
    assert pick(S(24561), "variant", "tiles", "waves", "workgroups") == ("ldsw", 1536, 6, 256)
    assert S(24560)["variant"] == "stream"
    # GIN: streaming and forced LDS-shared on the synthetic lists, natural LDS-shared with six waves, the persistent kernel
    assert pick(G(85, "f16x3"), "variant", "waves") == ("stream", 4)
    assert pick(G(85, "f16x3", FORCE_LDSW), "variant", "waves", "workgroups") == ("ldsw", 1, 6)
    assert pick(G(24561, "f16x3"), "variant", "waves", "workgroups") == ("ldsw", 6, 256)
    for prec in ("f16x3", "bf16x3"):
        assert pick(G(65537, prec), "variant", "tiles", "waves", "workgroups", "rounds", "second_round_tiles", "last_valid") == \
            ("persistent", 4097, 16, 256, 2, 1, 1)
    assert pick(G(65537, "f32"), "variant", "workgroups", "rounds", "last_live", "last_idle") == ("ldsw", 257, 1, 1, 15)
    assert G(65536, "f16x3")["variant"] == "ldsw"                     # (256 workgroups: not persistent)
    # k_gin_gather: 32 slots per pass, both halves of a pair walk the larger degree
    passes = [NR.gather_passes(*p) for p in NR.PAIR_DEGREES]
    assert passes == [0, 1, 1, 1, 1, 1, 2, 2, 2, 3, 3, 4]
    lists = NR.synthetic_in_lists(85, 1360)
    assert tuple(map(tuple, lists["degree"][:24].reshape(-1, 2))) == NR.PAIR_DEGREES and lists["degree"][NR.HUB] == 100
    assert 85 % 2 == 1 and lists["degree"][84] == 5                   # the last node: its half-wave partner does not exist
    assert lists["hub_last_slot"] - lists["in_ptr"][NR.HUB] == 99     # the leaf's message: the hub's fourth pass
    assert np.count_nonzero(lists["in_src"] == lists["leaf"]) == 1 and lists["in_src"][lists["hub_last_slot"]] == lists["leaf"]
    dst = np.repeat(np.arange(85), lists["degree"])
    assert (lists["in_src"] == dst).any()                             # self messages
    assert all(np.all(np.diff(lists["in_src"][a:b]) >= 0) for a, b in zip(lists["in_ptr"][:-1], lists["in_ptr"][1:]))


def test_tiled_batches_have_the_size_they_are_asked_for():
    for n in (37, 1, 16, 4099):
        b = NR.tiled_batch(n)
        assert b["atom_type"].shape[0] == n == b["batch"].shape[0] and b["batch"][-1] == b["num_graphs"] - 1
        assert np.all(np.diff(b["batch"]) >= 0)
        if n > 1:
            assert 0 <= b["bond_index"].min() and b["bond_index"].max() < n
            assert np.all(b["batch"][b["bond_index"][0]] == b["batch"][b["bond_index"][1]])
    assert set(NR.atom_types(100)) == set(range(100)) and tuple(NR.atom_types(3)) == (99, 0, 1)
