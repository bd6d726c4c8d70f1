"""CPU: tests/fused_ref.py (the float64 restatement tests/test_hip_fused_kernels.py compares k_cfconv_fused of csrc/edge.hip with)
anchored against the reference project's recorded CFConv outputs and against the oracle in float64; its comparison shown to be
sensitive (every wrong kernel listed below moves the aggregate past the "f32" gates); frag against unfrag; split against
gathered_aggregate; and the list designs shown to reach every tile path, chunk case and launch shape the GPU tests claim."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fused_ref as FR
import node_ref as NR
from helpers import FORWARD_CASES, TOL_ELEM, TOL_NORM, elem_err, load_golden, rel_err, t
from oracle import agdiff_oracle as O
from test_hip_kernels import _agg_ref, _bn, _lin, _xs_ref
from test_hip_parity import unfrag

BLK0 = "encoder_global.interactions.0"


@functools.lru_cache(maxsize=None)
def _sd():
    from agdiff_amd import drugs_model_config
    cfg = drugs_model_config()
    return cfg, NR.to64(NR.state_dict(cfg))


def _scales(sd, cfg, blk, d):
    """lw(d) C(d) of conv1 and conv2 of a block, as test_hip_kernels._agg_ref computes them (float64)."""
    import math
    import torch.nn.functional as F
    out = []
    for c in (1, 2):
        p = "%s.conv%d" % (blk, c)
        lw = torch.sigmoid(_lin(sd, p + ".distance_weighting.layer2",
                                F.relu(_lin(sd, p + ".distance_weighting.layer1", d.view(-1, 1))))).view(-1)
        if cfg.smooth_conv:
            C = 0.5 * (torch.cos(d * math.pi / cfg.cutoff) + 1.0)
        else:
            C = torch.exp(-((d - cfg.cutoff) ** 2) / (2 * cfg.cutoff ** 2))
        out.append(lw * C * (d <= cfg.cutoff) * (d >= 0.0))
    return out


# ------------------------------------------------------------------------------------------------- anchor
@pytest.mark.parametrize("case", ["g3_forward_qm9_small", "g3_forward_smooth_sparse"])
def test_reference_reproduces_the_recorded_cfconv_outputs(case):
    """The fixture's edges, lengths and edge_attr through fused_ref.cfconv_fused, then lin2 and norm2: cfconv1_b0 and cfconv2_b0 as
    the reference project recorded them, to the 5e-6 tests/test_hip_kernels.py holds its own host decomposition to -- and that
    decomposition itself to float64 rounding."""
    g = load_golden(case)
    cfg = FORWARD_CASES[case]()
    sd = O.synth_state_dict_for(cfg)
    O.embedding_renorm_(sd["encoder_global.embedding.weight"], t(g["atom_type"]))
    sd = NR.to64(sd)
    xs = _xs_ref(sd, BLK0, t(g["schnet_h0"]).double())
    s1, s2 = _scales(sd, cfg, BLK0, t(g["edge_length"]).double().view(-1))
    agg = FR.cfconv_fused(sd, cfg, 0, g["edge_attr"], s1, s2, g["edge_index"][0], g["edge_index"][1], xs)
    assert rel_err(agg, _agg_ref(sd, cfg, BLK0, g, xs)) < 1e-12
    for c, lo, hi, key in ((1, 0, 128, "cfconv1_b0"), (2, 128, 192, "cfconv2_b0")):
        p = "%s.conv%d" % (BLK0, c)
        post = _bn(sd, p + ".norm2", _lin(sd, p + ".lin2", agg[:, lo:hi])).float().numpy()
        err = rel_err(post, g[key])
        print("anchor %s %s: %.2e" % (case, key, err))
        assert err < 5e-6


def test_reference_equals_the_oracle_on_the_capped_drugs_graph():
    """g3_forward_drugs_capped (graphs at the 32-neighbour cap) records no stage outputs and no edge_attr: its edges, lengths and
    types go through the oracle's edge encoder and the oracle's CFConv in float64, block 0 and block 3 (every block has its own
    filter weights), and fused_ref.cfconv_fused must give the same to rounding."""
    case = "g3_forward_drugs_capped"
    g = load_golden(case)
    cfg = FORWARD_CASES[case]()
    sd = O.synth_state_dict_for(cfg)
    O.embedding_renorm_(sd["encoder_global.embedding.weight"], t(g["atom_type"]))
    sd = NR.to64(sd)
    ei, d = t(g["edge_index"]).long(), t(g["edge_length"]).double().view(-1)
    ea = O.mlp_edge_encoder(sd, "edge_encoder_global", d.view(-1, 1), t(g["edge_type"]).long())
    h = sd["encoder_global.embedding.weight"][t(g["atom_type"]).long()]
    for k in (0, 3):
        blk = "encoder_global.interactions.%d" % k
        xs = _xs_ref(sd, blk, h)
        s1, s2 = _scales(sd, cfg, blk, d)
        agg = FR.cfconv_fused(sd, cfg, k, ea, s1, s2, ei[0], ei[1], xs)
        for c, lo, hi in ((1, 0, 128), (2, 128, 192)):
            p = "%s.conv%d" % (blk, c)
            post = _bn(sd, p + ".norm2", _lin(sd, p + ".lin2", agg[:, lo:hi]))
            want = O.cfconv(sd, p, h, ei, d.view(-1, 1), ea, cfg.cutoff, cfg.smooth_conv)
            assert rel_err(post, want) < 1e-12


# ------------------------------------------------------------------------------------------------- sensitivity
def _moved(name, got, ref):
    """A comparison of `got` with `ref` fails at the "f32" gates of helpers.py."""
    rn, re_ = rel_err(got, ref), elem_err(got, ref)
    print("mutation %-28s normwise %.2e  elementwise %.2e" % (name, rn, re_))
    return rn > TOL_NORM["f32"] or re_ > TOL_ELEM["f32"]


@pytest.mark.parametrize("k", [0, 5])
def test_every_wrong_kernel_moves_the_aggregate_past_the_f32_gates(k):
    """Left out: the bias of either layer, the shift of the softplus, beta, one conv's scale, one edge, one chunk of agg_first;
    swapped: scale1 and scale2; src used for dst.  On the mod15 variant of the shapes list."""
    cfg, sd = _sd()
    ip = FR.shapes("mod15")
    d = FR.inputs("shapes:mod15", ip)
    E = d["E"]
    a = (d["attr"][:E], d["planes"][2 * k][:E], d["planes"][2 * k + 1][:E], d["src"], d["dst"], d["xs"])
    ref = FR.cfconv_fused(sd, cfg, k, *a)
    assert float(ref.abs().max()) > 0.1
    for m in ({"no_bias1": 1}, {"no_bias2": 1}, {"no_shift": 1}, {"no_beta": 1}, {"no_scale1": 1}, {"no_scale2": 1}, {"scales_swapped": 1},
              {"src_for_dst": 1}, {"edge_dropped": 200}):
        assert _moved(next(iter(m)), FR.cfconv_fused(sd, cfg, k, *a, mutate=m), ref), m
    sp = FR.split(ip, FR.messages(sd, cfg, k, *a[:4], d["xs"]), 128)
    assert rel_err(NR.gathered_aggregate(ip, sp["agg"], sp["agg_first"], 128), ref) < 1e-12
    for c in sp["rows_first"]:
        first = sp["agg_first"].clone()
        first[c] = 0.0
        assert _moved("chunk %d of agg_first" % c, NR.gathered_aggregate(ip, sp["agg"], first, 128), ref)
    other = FR.cfconv_fused(sd, cfg, (k + 1) % 6, *a)                 # (the next block's filters: every block has its own)
    assert _moved("next block's weights", other, ref)


# ------------------------------------------------------------------------------------------------- frag / unfrag
@pytest.mark.parametrize("precision", FR.MODES)
def test_frag_is_the_inverse_of_unfrag(precision):
    """unfrag(frag(x)) == hi + lo bit for bit (f32: x itself), for 37 rows (two full tiles and five rows: the pad rows are zero) of
    magnitudes from 1e-6 to 40; and the split is a split: |x - (hi + lo)| <= 2^-16 |x| in bf16x3, 2^-21 |x| + 2^-25 in f16x3."""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((37, 128)) * np.exp(rng.uniform(np.log(1e-6), np.log(40.0), size=(37, 128)))).astype(np.float32)
    f = FR.frag(x, precision)
    assert f.dtype == torch.float32 and f.numel() == 3 * 16 * 128
    back = unfrag(f, 37, precision)
    want = FR.operands(x, precision)
    assert np.array_equal(back.numpy().astype(np.float64), want)
    full = unfrag(f, 48, precision).numpy()
    assert np.all(full[37:] == 0.0)
    if precision == "f32":
        assert np.array_equal(back.numpy().view(np.int32), x.view(np.int32))
    else:
        bound = 2.0 ** -16 * np.abs(x) if precision == "bf16x3" else 2.0 ** -21 * np.abs(x) + 2.0 ** -25
        assert np.all(np.abs(x.astype(np.float64) - want) <= bound)


# ------------------------------------------------------------------------------------------------- split / gather
@pytest.mark.parametrize("ce", FR.CHUNK_EDGES)
def test_split_is_inverted_by_gathered_aggregate(ce):
    ip = FR.chunks(ce)
    E, n = int(ip[-1]), ip.shape[0] - 1
    msg = torch.from_numpy(np.random.default_rng(ce).standard_normal((E, 192)))
    sp = FR.split(ip, msg, ce)
    dst = torch.from_numpy(np.repeat(np.arange(n), np.diff(ip)))
    want = torch.zeros(n, 192, dtype=torch.float64).index_add_(0, dst, msg)
    assert rel_err(NR.gathered_aggregate(ip, sp["agg"], sp["agg_first"], ce), want) < 1e-13
    assert list(sp["rows_first"]) == NR.chunks_read(ip, ce) and 0 not in sp["rows_first"]
    assert np.array_equal(sp["rows_agg"], np.nonzero(np.diff(ip) > 0)[0])
    # a part in the wrong buffer: the sum stays, the separate comparison does not
    c = int(sp["rows_first"][0])
    owner = int(dst[c * ce])
    moved_agg, moved_first = sp["agg"].clone(), sp["agg_first"].clone()
    moved_agg[owner] += moved_first[c]
    moved_first[c] = 0.0
    assert rel_err(moved_agg, sp["agg"]) > 1e-3 and rel_err(moved_first, sp["agg_first"]) > 1e-3


# ------------------------------------------------------------------------------------------------- reach
def _tile_classes(cl):
    out = set()
    for tl in cl["tiles"]:
        out.add(tl["path"])
        for key in ("flush", "carry", "big", "partial", "first_from_earlier_chunk"):
            if tl[key]:
                out.add(key)
                out.add(key + "+" + tl["path"])
    return out


ALWAYS = {"one", "two", "general", "big", "partial"}
MULTI_TILE = {"flush", "carry", "carry+one", "carry+two", "carry+general", "flush+one", "flush+two"}
CHUNKED = {"first_from_earlier_chunk", "first_from_earlier_chunk+one", "first_from_earlier_chunk+two", "first_from_earlier_chunk+general"}
LIST_CLASSES = {"spans 1", "spans 2", "spans 3", "spans 4", "starts on a boundary after another list", "starts one edge before a boundary",
                "a chunk inside one hub"}


def test_chunk_tiles_rule_is_the_librarys():
    from agdiff_amd import _lib
    lib = _lib.load()
    caps = [FR.smallest_capacity(c) for c in (1, 2, 4, 8)]
    for cap in [1, 15, 16, 17, 384, 1024, 40000] + caps + [c - 1 for c in caps[1:]] + [1 << 26]:
        assert lib.agdiff_conv_chunk_tiles(ctypes.c_int64(cap)) == FR.conv_chunk_tiles(cap), cap
    assert _lib.DEFINES["AGDIFF_MAX_CHUNK_TILES"] == FR.MAX_CHUNK_TILES and _lib.TILE == FR.TW
    assert [FR.conv_chunk_tiles(c) for c in caps] == [1, 2, 4, 8] and caps[0] == 1


def test_the_designs_reach_what_they_claim():
    """The test that keeps a later edit of a design from silently dropping a path.  One tile per chunk has no previous tile: no
    flush and no carry at 16 edges per chunk."""
    for ct in (1, 2, 8):
        ce, cap = FR.TW * ct, max(FR.smallest_capacity(ct), 2048)
        # shapes
        seen = set()
        for v in FR.SHAPES:
            ip = FR.shapes(v)
            cl = FR.classify(ip, ip[-1], ct, cap)
            assert cl["chunk_tiles"] == ct == FR.conv_chunk_tiles(cap)
            seen |= _tile_classes(cl)
            if v in ("mod0", "mod1", "mod15"):
                assert int(ip[-1]) % 16 == int(v[3:]) and cl["zeroed"].size >= 71
        want = ALWAYS | (MULTI_TILE if ct > 1 else set())
        assert want <= seen, (ct, sorted(want - seen))
        assert int(FR.shapes("one")[-1]) == 1 and int(FR.shapes("none")[-1]) == 0
        assert FR.classify(FR.shapes("none"), 0, ct, cap)["tiles"] == []
        # chunks
        ip = FR.chunks(ce)
        cl = FR.classify(ip, ip[-1], ct, cap)
        seen = _tile_classes(cl)
        want = ALWAYS | CHUNKED | (MULTI_TILE if ct > 1 else set())
        assert want <= seen, (ct, sorted(want - seen))
        lists = FR.list_classes(ip, ce)
        want = LIST_CLASSES | ({"entered list ends on a tile end inside a chunk"} if ct > 1 else set())
        assert want <= lists, (ct, sorted(want - lists))
        assert cl["grid"] == (16 if ct == 1 else 256)
    # the degrees of the shapes list
    deg = np.diff(FR.shapes("mod0"))
    starts = {int(d): int(o) % 16 for d, o in zip(deg, FR.shapes("mod0")[:-1]) if d in (33, 40, 64, 100)}
    assert starts == {33: 0, 40: 1, 64: 15, 100: 0}
    ip = FR.shapes("mod0")
    nz = np.nonzero(deg)[0]
    assert deg[0] == 0 and deg[-1] == 0 and nz[0] > 0 and nz[-1] < deg.shape[0] - 1
    assert any(deg[i] == 0 and ip[i] % 16 == 0 and 0 < ip[i] < ip[-1] for i in range(deg.shape[0]))          # between two tiles
    assert any(deg[i] == 0 and ip[i] % 16 != 0 for i in range(deg.shape[0]))                                 # inside a tile
    # rounds, and the launch shapes of tests/test_hip_fused_kernels.py
    ip = FR.rounds()
    E = int(ip[-1])
    assert E > 2048 * 16
    big = FR.classify(ip, E, 1, 40000)
    assert FR.conv_chunk_tiles(40000) == 1 and big["grid"] == 256 and big["remap"] and big["rounds"] == 2
    for cap, grid, remap in ((384, 3, False), (1024, 8, True), (2048, 16, True)):
        cut = FR.prefix(ip, cap)
        cl = FR.classify(cut, cut[-1], FR.conv_chunk_tiles(cap), cap)
        assert (cl["grid"], cl["remap"], cl["rounds"], cl["chunk_tiles"]) == (grid, remap, 1, 1)
        assert cap - 64 < cut[-1] <= cap
    assert {"one", "two", "general"} <= _tile_classes(big)


def test_the_inputs_are_what_they_claim():
    """Twelve planes of their own in [0, 1] with about one entry in ten exactly 0; valid sources; unit-scale xs; attributes at 0.3."""
    ip = FR.chunks(128)
    d = FR.inputs("chunks:128", ip)
    E = d["E"]
    pl = d["planes"][:, :E]
    assert pl.shape[0] == 12 and pl.min() == 0.0 and pl.max() <= 1.0
    zero = (pl == 0.0).mean(axis=1)
    assert np.all(zero > 0.05) and np.all(zero < 0.2)
    for i in range(12):
        for j in range(i):
            assert np.abs(pl[i] - pl[j]).mean() > 0.2
    assert np.all(d["planes"][:, E:] == 0.75) and d["src"].min() >= 0 and d["src_pad"].max() < d["N"]
    assert abs(float(d["xs"].std()) - 1.0) < 0.05 and abs(float(d["attr"].std()) - 0.3) < 0.02
    assert np.array_equal(d["dst"], np.repeat(np.arange(d["N"]), np.diff(ip))) and np.isfinite(d["attr"]).all()


def test_the_star_batch_has_the_local_in_degrees():
    """Local in-degrees 1, 7, 8, 9, 33 and 64; every list padded to eight entries or more; three bond types."""
    from agdiff_amd.topology import BatchTopology
    b = FR.star_batch()
    tp = BatchTopology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], num_graphs=b["num_graphs"], extend_order=False, device="cpu")
    deg = np.bincount(tp.loc_dst.numpy(), minlength=tp.N)
    assert set(deg.tolist()) == {1, 7, 8, 9, 33, 64}
    lp = tp.lp_ptr.numpy().astype(np.int64)
    assert np.array_equal(np.diff(lp), np.maximum(deg, 8)) and tp.Lp == lp[-1]
    real = tp.lp_row.numpy() >= 0
    assert real.sum() == tp.L and np.array_equal(tp.lp_src.numpy()[~real], tp.lp_dst.numpy()[~real])
    assert set(np.unique(tp.lp_type.numpy()[real]).tolist()) == set(FR.STAR_TYPES)
    assert tp.Lp % 16 != 0                                            # (a partial last tile)
