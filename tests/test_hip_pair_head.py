"""GPU (MI355X): the two pair heads (csrc/edge.hip k_pair_head, k_pair_head_poly) through their own C-ABI entry points --
agdiff_pair_head, agdiff_pair_head_poly, agdiff_pair_head_poly_rows -- against the float64 restatement tests/pair_head_ref.py, on
inputs the tests make themselves (their design is checked without a GPU in tests/test_pair_head_ref_cpu.py):
  A  every activation of ag_head_act (csrc/common.hpp) at exact arguments: breakpoints and their float32 neighbours, both tails to +-40
  B  random weights, the 256-wide first layer under every activation, pre-activations from 1e-3 to beyond +-20
  C  edge counts around the 16-edge tile, a count far below 16 * max_tiles, the XCD remap (16 workgroups) and a wave's second tile
  D  operand-form attributes, the pos_index / mir_index scatter, attr_rows next to the index arrays
  E  the split-fp16 range flag at range_rows[src]
  F  the polynomial global head, stand-alone (also under the XCD remap) and over the canonical radius list of agdiff_sampler_front
All gates are helpers.check_close at its own tolerances; float32 torch meets them against float64 on these inputs for every activation
(worst: hardsigmoid 2.1e-6 normwise, 9.8e-4 element-wise), so no call site passes a scale."""
import ctypes

import numpy as np
import pytest
import torch

import pair_head_ref as R
from helpers import check_close, t

pytestmark = pytest.mark.gpu
PRECISIONS = ["f32", "bf16x3", "f16x3"]
_MODELS, _REFS = {}, {}


def _model(act, weights, precision, radius_poly="off"):
    """(model, packed weights, state dict, config): one construction per (activation, weights), repacked per arithmetic mode"""
    from agdiff_amd import get_model, qm9_model_config
    from oracle import agdiff_oracle as O
    key = (act, weights, radius_poly)
    if key not in _MODELS:
        while len(_MODELS) >= 4:
            _MODELS.pop(next(iter(_MODELS)))
        cfg = qm9_model_config(mlp_act=act)
        sd = O.synth_state_dict_for(cfg, head_scale=1.0)
        if weights == "pass_through":
            sd = R.pass_through_state_dict(sd, act)
        m = get_model(cfg)
        m.radius_poly = radius_poly
        m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
        _MODELS[key] = (m.to("cuda:0").eval(), sd, cfg)
    m, sd, cfg = _MODELS[key]
    m.precision = m.precision_local = precision
    pk = m.packed()
    assert (pk.precision, pk.precision_local) == (precision, precision)          # no fall-back to another mode
    return m, pk, sd, cfg


def _ref(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _head(pk, head, range_rows=None):
    """a copy of the packed agdiff_head_params_t, optionally with a range-flag array of the test's own"""
    from agdiff_amd import _lib
    hp = _lib.HeadParams.from_buffer_copy(getattr(pk.struct, "head_" + head))
    if range_rows is not None:
        hp.range_rows = _lib.ptr(range_rows)
    return hp


def _dev(x, cap, dtype):
    """`x` on the device in a buffer of `cap` leading entries (zero beyond it): no launch is handed a null or short array"""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    buf = torch.zeros((max(cap, 1),) + tuple(x.shape[1:]), dtype=dtype, device="cuda")
    buf[: x.shape[0]].copy_(x)
    return buf


def _launch(hp, n_edges, max_tiles, src, dst, h, out, frag=None, rows=None, pos=None, mir=None):
    from agdiff_amd import _lib
    lib = _lib.load()
    cap = 16 * max_tiles
    # every array covers what a launch of max_tiles tiles may touch, every index stays inside the array it addresses
    assert src.numel() >= cap and dst.numel() >= cap
    assert rows is None or rows.shape[0] >= cap
    assert frag is None or pos is not None or frag.numel() >= cap * 128
    assert 0 <= int(src.min()) and int(src.max()) < h.shape[0]
    assert 0 <= int(dst.min()) and int(dst.max()) < h.shape[0]
    if pos is not None:
        live = torch.cat([pos[:n_edges], mir[:n_edges]])
        assert pos.numel() >= cap and mir.numel() >= cap and int(live.max()) < out.numel() and int(pos[:n_edges].min()) >= 0
        assert frag is None or int(pos[:n_edges].max()) * 128 < frag.numel()
    else:
        assert out.numel() >= n_edges
    n_dev = torch.tensor([n_edges], dtype=torch.int32, device="cuda")
    rc = lib.agdiff_pair_head(ctypes.byref(hp), _lib.ptr(n_dev), ctypes.c_int64(max_tiles), _lib.ptr(src), _lib.ptr(dst), _lib.ptr(h),
                              _lib.ptr(frag), _lib.ptr(rows), _lib.ptr(pos), _lib.ptr(mir), _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _plain_run(pk, head, n_edges, src, dst, h, attr, extra_tiles=0, range_rows=None):
    """attr_rows, no index arrays: out [16 * max_tiles] pre-filled with the payload"""
    tiles = (n_edges + 15) // 16 + extra_tiles
    cap = 16 * tiles
    out = R.payload(max(cap, 1), "cuda")
    rc = _launch(_head(pk, head, range_rows), n_edges, tiles, _dev(src[:n_edges], cap, torch.int32), _dev(dst[:n_edges], cap, torch.int32),
                 h, out, rows=_dev(attr[:n_edges], cap, torch.float32))
    assert rc == 0
    return out


# ------------------------------------------------------------------------------------------------ A, B: the activation switch
def _sweep_inputs():
    src, dst = R.edges(R.E_SWEEP, R.N_SWEEP)
    return src, dst, R.node_rows(R.N_SWEEP)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act", R.ACTS)
def test_activation_sweep_with_exact_arguments(act, precision):
    """A: layers.0 = [0 | I] hands the attribute row to the first activation unchanged, so the kernel evaluates ag_head_act at exactly
    the sweep's values: a wrong tail, clamp or breakpoint of one activation shows in the scores of the edges that hold those values."""
    m, pk, sd, cfg = _model(act, "pass_through", precision)
    src, dst, h = _sweep_inputs()
    rows = R.sweep_rows()
    flags = torch.zeros(R.N_SWEEP, dtype=torch.int32, device="cuda")
    for head in ("global", "local"):
        ref, pre1, pre2 = _ref(("A", act, head), lambda: R.pair_head(sd, head, act, h, src, dst, rows))
        R.check_sweep_hit(pre1)
        R.check_hidden((pre1, R.activation(act)(pre1), pre2, R.activation(act)(pre2)))
        R.check_scores(ref)
        out = _plain_run(pk, head, R.E_SWEEP, src, dst, h.cuda(), rows, range_rows=flags)
        check_close("pair_head sweep %s %s" % (act, head), out[: R.E_SWEEP], ref, precision)
        assert torch.equal(R.bits(out[R.E_SWEEP:]), R.bits(R.payload(out.numel() - R.E_SWEEP)))
    assert int(flags.sum()) == 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act", R.ACTS)
def test_random_weights_under_every_activation(act, precision):
    """B: the synthetic checkpoint's heads (all 256 x 128 first-layer weights live: MFMA lane maps, k-tile order), N(0, 1) node rows,
    attribute rows scaled per edge from 1e-3 to 64 -- first-layer pre-activations in every range of the switch on both signs."""
    m, pk, sd, cfg = _model(act, "synthetic", precision)
    src, dst, h = _sweep_inputs()
    rows = R.scaled_rows()
    for head in ("global", "local"):
        ref, pre1, pre2 = _ref(("B", act, head), lambda: R.pair_head(sd, head, act, h, src, dst, rows))
        R.check_bins(pre1)
        R.check_hidden((pre1, R.activation(act)(pre1), pre2, R.activation(act)(pre2)))
        out = _plain_run(pk, head, R.E_SWEEP, src, dst, h.cuda(), rows)
        check_close("pair_head random %s %s" % (act, head), out[: R.E_SWEEP], ref, precision)


# ------------------------------------------------------------------------------------------------ C: edge counts, the tile walk
E_COUNTS = [0, 1, 15, 16, 17, 16 * 64 + 3]
# 252 tiles + 4 = 256 = 16 workgroups of 16 waves: workgroup b walks the tiles of (b % 8) * 2 + b / 8, a permutation that is not the
# identity (with 8 workgroups it is)
E_REMAP = 16 * 251 + 7
# 4131 tiles + 4 > 256 workgroups x 16 waves: the last 39 tiles are a wave's SECOND tile.  The one case of this file beyond a few
# hundred edges -- nothing smaller reaches a second round; inputs and the float64 reference are built once and shared by the modes.
E_ROUNDS = 16 * 4130 + 3


def _count_inputs(n_max):
    src, dst = R.edges(n_max, 61, seed=81)
    rows = R.scaled_rows(n_max, seed=37, top=8.0)
    rows[3] = rows[2]                     # edges 2 and 3: the same pair of nodes with the same attributes
    return src, dst, R.node_rows(61, seed=31), rows


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n_edges", E_COUNTS + [E_REMAP])
@pytest.mark.parametrize("act", ["relu", "gelu"])
def test_edge_counts_and_partial_tiles(act, n_edges, precision):
    """C: *n_edges_dev (a device word) against max_tiles four tiles larger than needed; entries [0, E) meet the gate, everything from E on
    keeps its NaN payload bit for bit; E = 0 returns 0 and writes nothing.  Edge 1 has src == dst, edges 2 and 3 are identical."""
    m, pk, sd, cfg = _model(act, "synthetic", precision)
    n_max = max(E_COUNTS + [E_REMAP])
    src, dst, h, rows = _ref(("C in",), lambda: _count_inputs(n_max))
    assert src[1] == dst[1] and (src[2], dst[2]) == (src[3], dst[3])
    for head in ("global", "local"):
        ref, _, pre2 = _ref(("C", act, head), lambda: R.pair_head(sd, head, act, h, src, dst, rows))
        # (E = 1 divides by edge 0's score alone: the seed of the edges was chosen, on the reference, so that this score is not
        # a cancelled value -- at least a fifth of what its last layer adds up)
        assert abs(float(ref[0])) >= 0.2 * float(R.score_weight(sd, head, act, pre2[:1])[0])
        out = _plain_run(pk, head, n_edges, src, dst, h.cuda(), rows, extra_tiles=4)
        assert out.numel() >= n_edges + 64
        if n_edges:
            check_close("pair_head E=%d %s %s" % (n_edges, act, head), out[:n_edges], ref[:n_edges], precision)
        assert torch.equal(R.bits(out[n_edges:]), R.bits(R.payload(out.numel() - n_edges)))
        if n_edges > 3:
            assert torch.equal(R.bits(out[2:3]), R.bits(out[3:4]))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_tile_walk_beyond_one_round(precision):
    """C: more tiles than the 256 x 16 waves of one persistent launch -- a wave's second tile, under the XCD remap -- and, with the same
    max_tiles, a live count of 17: the walk ends at *n_edges_dev wherever max_tiles would let it go."""
    act = "relu"
    m, pk, sd, cfg = _model(act, "synthetic", precision)
    src, dst, h, rows = _ref(("C big in",), lambda: _count_inputs(E_ROUNDS))
    ref = _ref(("C big", act), lambda: R.pair_head(sd, "global", act, h, src, dst, rows)[0])
    tiles = (E_ROUNDS + 15) // 16 + 4
    assert tiles > 256 * 16
    cap = 16 * tiles
    args = (_dev(src, cap, torch.int32), _dev(dst, cap, torch.int32), h.cuda())
    rows_d = _dev(rows, cap, torch.float32)
    for n_edges in (E_ROUNDS, 17):
        out = R.payload(cap, "cuda")
        assert _launch(_head(pk, "global"), n_edges, tiles, *args, out, rows=rows_d) == 0
        check_close("pair_head E=%d of %d tiles" % (n_edges, tiles), out[:n_edges], ref[:n_edges], precision)
        assert torch.equal(R.bits(out[n_edges:]), R.bits(R.payload(cap - n_edges)))


# ------------------------------------------------------------------------------------------------ D: operand form, scatter
@pytest.mark.parametrize("precision", PRECISIONS)
def test_operand_form_attributes_and_the_scatter(precision):
    """D: attr_frag and attr_rows of the same edges from agdiff_edge_encoder; the fragments read back (the layout test_hip_parity.py's
    unfrag documents) are the reference's attributes.  Plain; scattered through pos_index / mir_index (a random injection into
    [0, 2E), a mirror for two edges in three, position 0 among the mirrors); and attr_rows next to the index arrays, where edge e reads
    row e whatever pos_index says."""
    from agdiff_amd import _lib
    from test_hip_parity import unfrag
    act = "gelu"
    m, pk, sd, cfg = _model(act, "synthetic", precision)
    lib, st, P = _lib.load(), _lib.stream_ptr(), ctypes.byref(pk.struct)
    E = R.E_SWEEP
    tiles, tiles2 = (E + 15) // 16, (2 * E + 15) // 16
    src, dst, h = _sweep_inputs()
    gen = torch.Generator().manual_seed(41)
    length = (torch.rand(E, generator=gen) * (cfg.cutoff - 1e-3) + 1e-3).clamp(max=cfg.cutoff).float()
    length[-1] = cfg.cutoff
    etype = torch.tensor([0, 1, 2, 3, 12, 23, 24])[torch.randint(0, 7, (E,), generator=gen)]
    pos, mir = R.scatter_indices(E)
    cap = 16 * tiles
    src_d, dst_d, h_d = _dev(src, cap, torch.int32), _dev(dst, cap, torch.int32), h.cuda()
    len_d, typ_d = _dev(length, cap, torch.float32), _dev(etype, cap, torch.int32)
    pos_d, mir_d = _dev(pos, cap, torch.int32), _dev(mir, cap, torch.int32)
    n_dev = torch.tensor([E], dtype=torch.int32, device="cuda")
    frag, rows = torch.zeros(cap * 128, device="cuda"), torch.zeros(cap, 128, device="cuda")
    frag2 = torch.zeros(16 * tiles2 * 128, device="cuda")
    assert lib.agdiff_edge_encoder(P, _lib.ptr(n_dev), ctypes.c_int64(tiles), _lib.ptr(len_d), _lib.ptr(typ_d), _lib.ptr(frag), _lib.ptr(rows),
                                   None, None, None, st) == 0
    assert lib.agdiff_edge_encoder(P, _lib.ptr(n_dev), ctypes.c_int64(tiles), _lib.ptr(len_d), _lib.ptr(typ_d), _lib.ptr(frag2), None,
                                   None, _lib.ptr(pos_d), _lib.ptr(mir_d), st) == 0
    torch.cuda.synchronize()
    attr = unfrag(frag, E, precision).cpu()
    assert torch.equal(unfrag(frag2, 2 * E, precision).cpu()[torch.from_numpy(pos).long()], attr)      # stored at pos_index[e]
    check_close("pair_head D rows vs fragments", rows[:E], attr, precision)
    ref = R.pair_head(sd, "global", act, h, src, dst, attr)[0]
    R.check_hidden(R.pair_head(sd, "global", act, h, src, dst, attr)[1:])

    out = R.payload(cap, "cuda")
    assert _launch(_head(pk, "global"), E, tiles, src_d, dst_d, h_d, out, frag=frag) == 0
    check_close("pair_head D attr_frag", out[:E], ref, precision)
    assert torch.equal(R.bits(out[E:]), R.bits(R.payload(cap - E)))
    plain = out[:E].clone()

    def scattered(out2, what):
        p, q = torch.from_numpy(pos).long(), torch.from_numpy(mir).long()
        has = q >= 0
        check_close("pair_head D %s out[pos]" % what, out2[p.cuda()], what_ref[what], precision)
        assert torch.equal(R.bits(out2[q[has].cuda()]), R.bits(out2[p[has].cuda()]))                    # the mirror: the same bits
        named = torch.zeros(2 * E, dtype=torch.bool)
        named[p] = True
        named[q[has]] = True
        assert named[0] and int(named.sum()) == E + int(has.sum())
        rest = out2.cpu()[~named]
        assert torch.equal(R.bits(rest), R.bits(R.payload(rest.numel())))
        return out2[p.cuda()]

    what_ref = {"attr_frag": ref, "attr_rows": R.pair_head(sd, "local", act, h, src, dst, rows[:E].cpu())[0]}
    out2 = R.payload(2 * E, "cuda")
    assert _launch(_head(pk, "global"), E, tiles, src_d, dst_d, h_d, out2, frag=frag2, pos=pos_d, mir=mir_d) == 0
    assert torch.equal(R.bits(scattered(out2, "attr_frag")), R.bits(plain))          # the same arithmetic on the same operands
    out3 = R.payload(2 * E, "cuda")
    assert _launch(_head(pk, "local"), E, tiles, src_d, dst_d, h_d, out3, rows=rows, pos=pos_d, mir=mir_d) == 0
    scattered(out3, "attr_rows")


# ------------------------------------------------------------------------------------------------ E: the range flag
@pytest.mark.parametrize("precision", PRECISIONS)
def test_hidden_layer_beyond_the_split_fp16_range_flags_the_source_node(precision):
    """E: one edge's attribute row blown up so that its hidden layer passes 65000 (pass-through first layer, relu: the hidden value IS
    the attribute): split-fp16 sets exactly range_rows[src of that edge], the other modes set nothing, and every other edge's score
    still meets the gate -- tile-mates of the hot edge included."""
    act = "relu"
    m, pk, sd, cfg = _model(act, "pass_through", precision)
    src, dst, h = _sweep_inputs()
    rows = R.sweep_rows().copy()
    hot = 16 * 5 + 9
    rows[hot, 77] = 7.0e4
    for head in ("global", "local"):
        ref = R.pair_head(sd, head, act, h, src, dst, rows)[0]
        flags = torch.zeros(R.N_SWEEP, dtype=torch.int32, device="cuda")
        out = _plain_run(pk, head, R.E_SWEEP, src, dst, h.cuda(), rows, range_rows=flags)
        flagged = torch.nonzero(flags).flatten().cpu().tolist()
        assert flagged == ([int(src[hot])] if precision == "f16x3" else []), (precision, flagged)
        keep = np.arange(R.E_SWEEP) != hot
        check_close("pair_head range flag, other edges %s" % head, out[: R.E_SWEEP].cpu()[keep], ref[keep], precision)
        if precision != "f16x3":
            check_close("pair_head range flag, hot edge %s" % head, out[: R.E_SWEEP], ref, precision)


# ------------------------------------------------------------------------------------------------ F: the polynomial global head
def _encoder64(sd, length):
    from oracle import agdiff_oracle as O
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith("edge_encoder_global.")}
    d = torch.as_tensor(length).double().view(-1, 1)
    return O.mlp_edge_encoder(sd64, "edge_encoder_global", d, torch.zeros(d.shape[0], dtype=torch.long))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act", ["relu", "gelu", "softplus", "tanh"])
def test_polynomial_head_against_the_encoder_in_float64(act, precision):
    """F: agdiff_pair_head_poly on lengths from 1e-3 up to exactly the cutoff: the reference's attributes are the float64 MLP edge
    encoder of (length, type 0).  (The fit is accepted at <= 1e-6 of the layer it replaces: inside the gates.)"""
    from agdiff_amd import _lib
    m, pk, sd, cfg = _model(act, "synthetic", precision, radius_poly="auto")
    if pk.poly_kt < 1:
        pytest.skip("no polynomial fit accepted for these weights")
    lib = _lib.load()
    E = R.E_SWEEP
    src, dst, h = _sweep_inputs()
    length = torch.logspace(-3.0, float(np.log10(cfg.cutoff)), E).float()
    length[-1] = cfg.cutoff
    ref = _ref(("F", act), lambda: R.pair_head(sd, "global", act, h, src, dst, _encoder64(sd, length))[0])
    tiles = (E + 15) // 16 + 4
    cap = 16 * tiles
    out = R.payload(cap, "cuda")
    n_dev = torch.tensor([E], dtype=torch.int32, device="cuda")
    src_d, dst_d, len_d, h_d = _dev(src, cap, torch.int32), _dev(dst, cap, torch.int32), _dev(length, cap, torch.float32), h.cuda()
    assert lib.agdiff_pair_head_poly(ctypes.byref(pk.struct), _lib.ptr(n_dev), ctypes.c_int64(tiles), _lib.ptr(src_d), _lib.ptr(dst_d),
                                     _lib.ptr(len_d), _lib.ptr(h_d), None, None, _lib.ptr(out), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    check_close("pair_head_poly %s" % act, out[:E], ref, precision)
    assert torch.equal(R.bits(out[E:]), R.bits(R.payload(cap - E)))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_polynomial_head_under_the_xcd_remap(precision):
    """F: k_pair_head_poly has its own copy of the tile walk: 256 tiles = 16 workgroups, where the XCD remap is a permutation that is
    not the identity, and with the same max_tiles a live count of 17."""
    from agdiff_amd import _lib
    act = "relu"
    m, pk, sd, cfg = _model(act, "synthetic", precision, radius_poly="auto")
    if pk.poly_kt < 1:
        pytest.skip("no polynomial fit accepted for these weights")
    lib = _lib.load()
    E = E_REMAP
    src, dst, h, _ = _ref(("C in",), lambda: _count_inputs(E_REMAP))
    length = torch.logspace(-3.0, float(np.log10(cfg.cutoff)), E).float()
    length[-1] = cfg.cutoff
    ref = _ref(("F remap", act), lambda: R.pair_head(sd, "global", act, h, src, dst, _encoder64(sd, length))[0])
    tiles = (E + 15) // 16 + 4
    assert tiles == 256
    cap = 16 * tiles
    src_d, dst_d, len_d, h_d = _dev(src, cap, torch.int32), _dev(dst, cap, torch.int32), _dev(length, cap, torch.float32), h.cuda()
    assert int(src_d.max()) < h_d.shape[0] and int(dst_d.max()) < h_d.shape[0]
    for n_edges in (E, 17):
        out = R.payload(cap, "cuda")
        n_dev = torch.tensor([n_edges], dtype=torch.int32, device="cuda")
        assert lib.agdiff_pair_head_poly(ctypes.byref(pk.struct), _lib.ptr(n_dev), ctypes.c_int64(tiles), _lib.ptr(src_d), _lib.ptr(dst_d),
                                         _lib.ptr(len_d), _lib.ptr(h_d), None, None, _lib.ptr(out), _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        check_close("pair_head_poly E=%d of %d tiles" % (n_edges, tiles), out[:n_edges], ref[:n_edges], precision)
        assert torch.equal(R.bits(out[n_edges:]), R.bits(R.payload(cap - n_edges)))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act", ["relu", "gelu", "softplus", "tanh"])
def test_polynomial_head_over_the_canonical_radius_list(act, precision):
    """F: agdiff_pair_head_poly_rows after agdiff_sampler_front, for both step parities: every canonical entry's radius row meets the
    gate against the reference built from c_src / c_dst / c_len, the mirror row holds the same bits, every other entry of inv_r --
    the rows beyond rad_cnt among them -- keeps its payload."""
    from agdiff_amd import _lib, synth
    m, pk, sd, cfg = _model(act, "synthetic", precision, radius_poly="auto")
    if pk.poly_kt < 1:
        pytest.skip("no polynomial fit accepted for these weights")
    lib, st = _lib.load(), _lib.stream_ptr()
    RS = _lib.DEFINES["AGDIFF_RAD_STRIDE"]
    b = synth.make_packed_batch("qm9", 3, 2, seed=43)
    at, bi, bt, ba = [t(b[k]).cuda() for k in ("atom_type", "bond_index", "bond_type", "batch")]
    with torch.no_grad():
        pk = m._renorm_embedding(at)
        topo, ws = m._batch(at, bi, bt, ba, None, False)
    N = topo.N
    P, Tp, Wp = ctypes.byref(pk.struct), ctypes.byref(topo.struct), ctypes.byref(ws.struct)
    pos = (torch.randn(N, 3, generator=torch.Generator().manual_seed(47)) * 1.5).cuda().contiguous()
    ws.h.copy_(torch.randn(ws.h.shape, generator=torch.Generator().manual_seed(53)).cuda())
    h = ws.h.view(-1, 128).cpu()
    for parity in (0, 1):
        sa = _lib.StepArgs()
        sa.pos_in = _lib.ptr(pos)
        ws.canon_counter.zero_()
        ws.range_rows.zero_()
        assert lib.agdiff_sampler_front(P, Tp, Wp, ctypes.byref(sa), 2 | 4 | (16 * parity), ctypes.c_float(cfg.cutoff), st) == 0
        ws.inv_r.copy_(R.payload(ws.inv_r.numel(), "cuda"))
        assert lib.agdiff_pair_head_poly_rows(P, Tp, Wp, parity, st) == 0
        torch.cuda.synchronize()
        n_c = int(ws.canon_counter[parity].item())
        cnt = ws.rad_cnt.cpu().long()
        assert n_c > 0
        c_src, c_dst, c_len = ws.c_src[:n_c].cpu(), ws.c_dst[:n_c].cpu(), ws.c_len[:n_c].cpu()
        p, q = ws.c_pos[:n_c].cpu().long(), ws.c_mir[:n_c].cpu().long()
        has = q >= 0
        ref = R.pair_head(sd, "global", act, h, c_src.numpy(), c_dst.numpy(), _encoder64(sd, c_len))[0]
        inv_r = ws.inv_r[: N * RS].cpu()
        check_close("pair_head_poly_rows %s parity %d" % (act, parity), inv_r[p], ref, precision)
        assert bool(has.any()) and torch.equal(R.bits(inv_r[q[has]]), R.bits(inv_r[p[has]]))
        named = torch.zeros(N * RS, dtype=torch.bool)
        named[p] = True
        named[q[has]] = True
        assert int(named.sum()) == n_c + int(has.sum())                                   # no row named twice
        live = (torch.arange(RS)[None, :] < cnt[:, None]).reshape(-1)
        assert bool((live | ~named).all())                                                # every named row is a live radius row
        rest = ws.inv_r.cpu()[: N * RS][~named]
        assert torch.equal(R.bits(rest), R.bits(R.payload(rest.numel())))
        assert int(ws.range_rows.sum()) == 0
