"""GPU (MI355X): the per-edge producers -- the distance-weighting scale lw(d) C(d) (csrc/common.hpp cf_dist_weight x cf_envelope) in
all six places that evaluate it, the MLP edge encoder k_edge_encoder and the Gaussian one k_edge_gaussian (csrc/edge.hip) -- through
the C ABI, against the float64 restatement tests/edge_ref.py on inputs the tests make themselves (their design is checked without a
GPU in tests/test_edge_ref_cpu.py): twelve distance-weighting networks with kinks at chosen float32 values, lengths on every kink
and its two float32 neighbours, at +-0, at the cutoff and its neighbours and far beyond it.
  A  k_edge_scales: agdiff_edge_scales per edge and per canonical edge, agdiff_edge_scales_split(1 | 2), the slotted types' zeros
  B  k_rad_scales: agdiff_edge_scales_split(0) on radius counts 0, 1, 15, 16, 17, 32, 33 with their pad rows
  C  the fill passes of agdiff_graph_build_scaled and agdiff_graph_build_large and both forms of agdiff_sampler_front (union table at
     K = 512 and at K = 64, and without a union table), on a molecule whose radius lengths ARE the kinks
  D  k_edge_encoder: rows, operand form and both; row_index with missing and shared rows; the pos_index / mir_index scatter; a
     count past one persistent round; a second weight set that drives the first GELU into both tails
  E  the flagged tiles of agdiff_local_edge_rows: hard-row masks 0x0001, 0x8000 and a whole partial tile
  F  k_edge_gaussian up to lengths where every Gaussian underflows
Gates: encoder outputs helpers.check_close at its own tolerances per mode, no scale (rows at 100 rc, a thousand times larger, are
judged apart from the others); scales check_close(.., "f32") plus an absolute bound per element, the larger of 1e-6 (the figure
csrc/common.hpp documents for these factors) and four times what the plain-float32 restatement of the tables misses float64 by on
the same lengths (measured 1.15e-7 wide / 1.33e-7 narrow under the Gaussian envelope, 7.0e-8 / 7.3e-8 under the smooth one: the
bound is 1e-6 everywhere; the factor 4 is for the hardware's exp2, rcp and cos, one ulp each and chained).  Exact zeros, pad rows,
payload and bit-equalities are exact.
Measured on an MI355X (worst over sets and envelopes; normwise / element-wise / absolute): k_edge_scales and k_rad_scales 2.5e-7 /
3.0e-6 / 1.9e-7, the graph builds and both forms of the front 2.7e-7 / 3.0e-6 / 2.1e-7 (a fifth of the absolute bound, a twentieth
of the normwise gate); k_edge_encoder normwise 8.4e-7 f32, 1.2e-5 bf16x3, 9.9e-7 f16x3 and element-wise 3.1e-4 / 6.7e-3 / 5.9e-4
(bf16x3 normwise at 0.41 of its gate is the closest any figure comes); k_edge_gaussian 5.2e-8 / 8.3e-7 in every mode.
Left out: the far sets of k_edge_attr_poly (tests/test_hip_poly.py has them); NaN lengths (csrc/edge.hip is built with
-fno-honor-nans, NaN positions are nan_flag's business); edge types >= 100 (the tables have 100 rows)."""
import ctypes

import numpy as np
import pytest
import torch

import edge_ref as R
from helpers import TOL_ELEM, TOL_NORM, check_close, elem_err, rel_err, t
from pair_head_ref import bits, payload
from test_hip_pair_head import _dev

pytestmark = pytest.mark.gpu
PRECISIONS = ["f32", "bf16x3", "f16x3"]
_MODELS, _REFS, _SDS = {}, {}, {}


def _state_dict(kind, nets, weights):
    from agdiff_amd import drugs_model_config, qm9_model_config
    from oracle import agdiff_oracle as O
    key = (kind, nets, weights)
    if key not in _SDS:
        cfg = {"qm9": qm9_model_config, "drugs": drugs_model_config}[kind.split("-")[0]](
            edge_encoder="gaussian" if kind.endswith("gaussian") else "mlp")
        sd = O.synth_state_dict_for(cfg, head_scale=1.0)
        if nets is not None:
            sd = R.with_networks(sd, R.networks(nets))
        if weights == "expanded":
            sd = R.scaled_feature_expansion(sd)
        _SDS[key] = (sd, cfg)
    return _SDS[key]


def _model(kind, nets, precision, weights="synthetic", radius_poly="off", refuse=()):
    """(model, packed weights, state dict, config) as tests/test_hip_pair_head.py builds them: one construction per weight set, repacked
    per arithmetic mode.  kind: "qm9" (Gaussian envelope), "drugs" (smooth), "qm9-gaussian" (the Gaussian edge encoder)."""
    from agdiff_amd import get_model
    key = (kind, nets, weights, radius_poly, tuple(refuse))
    if key not in _MODELS:
        while len(_MODELS) >= 3:
            _MODELS.pop(next(iter(_MODELS)))
        sd, cfg = _state_dict(kind, nets, weights)
        m = get_model(cfg)
        m.radius_poly = radius_poly
        m.poly_refuse_types = tuple(refuse)
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


def _batch(m, b):
    """(topology, workspace, packed weights) of batch dict `b`, as the model itself makes them"""
    at, bi, bt, ba = [t(b[k]).cuda() for k in ("atom_type", "bond_index", "bond_type", "batch")]
    with torch.no_grad():
        pk = m._renorm_embedding(at)
        topo, ws = m._batch(at, bi, bt, ba, None, False)
    return topo, ws, pk


def _drugs_batch():
    from agdiff_amd import synth
    return synth.make_packed_batch("drugs", 3, 2, seed=43)


def _planes(buf, stride, n=R.NPLANES):
    """[12, stride] of a scale buffer of AGDIFF_MAX_CONVS x 2 planes (the planes beyond the model's twelve come back separately)"""
    v = buf.view(-1, stride)
    return v[:n], v[n:]


def _is_payload(x):
    return torch.equal(bits(x).view(-1), bits(payload(x.numel())))


def _abs_bound(which, d, smooth):
    """max(1e-6, 4 x the plain-float32 restatement's worst absolute error on these lengths)"""
    nets = R.networks(which)
    t32 = R.segment_tables(nets)[1]
    with np.errstate(over="ignore"):
        err = np.abs(R.table_scales(t32, d, R.RC, smooth, dtype=np.float32) - R.scales64(nets, d, R.RC, smooth)).max()
    return max(1e-6, 4.0 * float(err)), float(err)


def _scale_ref(which, d, smooth):
    with np.errstate(over="ignore"):
        return R.scales64(R.networks(which), np.asarray(d, dtype=np.float32), R.RC, smooth)


def _check_scales(name, got, ref, bound):
    """got, ref [12, n]: the "f32" gates over all planes and per plane, the absolute bound, and exact zeros where the reference is 0
    (outside [0, rc])"""
    got = got.detach().cpu().double().numpy() if hasattr(got, "detach") else np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), name
    check_close(name, got, ref, "f32")
    worst = float(np.abs(got - ref).max())
    print("absolute %-48s %.2e (bound %.2e)" % (name, worst, bound))
    assert worst <= bound, (name, worst)
    for p in range(ref.shape[0]):
        assert rel_err(got[p], ref[p]) < TOL_NORM["f32"] and elem_err(got[p], ref[p]) < TOL_ELEM["f32"], (name, p)
    assert np.all(got[ref == 0.0] == 0.0), name


def _take(d, n):
    """n of the lengths `d`: all of them (then repeated) when n >= len(d), else an even subset that keeps 0, -0, the cutoff's
    neighbourhood, 1.5 rc and 100 rc"""
    if n >= d.size:
        return np.resize(d, n)
    keep = np.nonzero((d == 0) | ((d >= np.float32(9.9999)) & (d <= np.float32(10.0001))) | (d >= 15.0))[0]
    rest = np.setdiff1d(np.arange(d.size), keep)
    pick = rest[np.linspace(0, rest.size - 1, n - keep.size).astype(np.int64)]
    return d[np.sort(np.concatenate([keep, pick]))]


# ------------------------------------------------------------------------------------------------ A: k_edge_scales
@pytest.mark.parametrize("which", ["wide", "narrow"])
@pytest.mark.parametrize("kind", ["qm9", "drugs"])
def test_edge_scales_per_edge_per_canonical_edge_and_split(kind, which):
    """A: the test's own lengths in ws.e_len / c_len / lc_len, the live counts in the device words.  Every plane against float64 in
    both envelope modes; a canonical entry's mirror position holds the bits of its own; entries beyond the live count, positions
    nothing names and the planes beyond the model's twelve keep the payload."""
    from agdiff_amd import _lib
    lib, st = _lib.load(), _lib.stream_ptr()
    m, pk, sd, cfg = _model(kind, which, "f32")
    smooth = int(cfg.smooth_conv)
    assert pk.struct.smooth == smooth and pk.struct.cutoff == R.RC
    topo, ws, pk = _batch(m, _drugs_batch())
    P, T, W = ctypes.byref(pk.struct), ctypes.byref(topo.struct), ctypes.byref(ws.struct)
    d = R.lengths(which)
    n = d.size
    ref = _scale_ref(which, d, smooth)
    bound, _ = _abs_bound(which, d, smooth)
    epad = ws.e_len.numel()
    assert n <= topo.max_edges and 2 * n <= epad and ws.e_scale.numel() % epad == 0
    dd = torch.from_numpy(d).cuda()
    # per edge
    ws.e_len[:n].copy_(dd)
    ws.num_edges.fill_(n)
    ws.e_scale.copy_(payload(ws.e_scale.numel(), "cuda"))
    assert lib.agdiff_edge_scales(P, T, W, 0, st) == 0
    torch.cuda.synchronize()
    mine, beyond = _planes(ws.e_scale, epad)
    _check_scales("edge_scales per edge %s %s" % (kind, which), mine[:, :n], ref, bound)
    assert _is_payload(mine[:, n:]) and _is_payload(beyond)
    per_edge = mine[:, :n].clone()
    # per canonical edge: one evaluation, two positions
    pos, mir = R.scatter_indices(n)
    has = torch.from_numpy(mir >= 0)
    p_, q_ = torch.from_numpy(pos).long().cuda(), torch.from_numpy(mir).long().cuda()
    ws.c_len[:n].copy_(dd)
    ws.c_pos[:n].copy_(torch.from_numpy(pos).cuda())
    ws.c_mir[:n].copy_(torch.from_numpy(mir).cuda())
    ws.num_canon.fill_(n)
    ws.e_scale.copy_(payload(ws.e_scale.numel(), "cuda"))
    assert lib.agdiff_edge_scales(P, T, W, 1, st) == 0
    torch.cuda.synchronize()
    mine, beyond = _planes(ws.e_scale, epad)
    assert torch.equal(bits(mine[:, p_]), bits(per_edge))                                   # the same routine on the same length
    assert torch.equal(bits(mine[:, q_[has.cuda()]]), bits(mine[:, p_[has.cuda()]]))        # the mirror: the same bits
    named = torch.zeros(epad, dtype=torch.bool)
    named[p_.cpu()] = True
    named[q_.cpu()[has]] = True
    assert int(named.sum()) == n + int(has.sum()) and named[0]
    assert _is_payload(mine[:, (~named).cuda()]) and _is_payload(beyond)
    # the local edges: the padded list (which = 1) and the quad tiles (which = 2), through the topology's own positions
    Lc = topo.Lc
    nl = min(n, Lc)
    dl = _take(d, nl)
    refl = _scale_ref(which, dl, smooth)
    ws.lc_len[:nl].copy_(torch.from_numpy(dl).cuda())
    ws.num_local_canon.fill_(nl)
    assert lib.agdiff_local_poly_enabled(P, T, W) == 0                                      # (radius_poly off: nothing is zeroed)
    for sel, out, lp, lm in ((1, ws.l_scale, topo.lc_ppos, topo.lc_pmir), (2, ws.lt_scale, topo.lc_tpos, topo.lc_tmir)):
        stride = out.numel() // (2 * _lib.DEFINES["AGDIFF_MAX_CONVS"])
        p_, q_ = lp[:nl].long(), lm[:nl].long()
        has = q_ >= 0
        assert int(p_.min()) >= 0 and int(torch.cat([p_, q_]).max()) < stride and bool(has.any())
        out.copy_(payload(out.numel(), "cuda"))
        assert lib.agdiff_edge_scales_split(P, T, W, sel, st) == 0
        torch.cuda.synchronize()
        mine, beyond = _planes(out, stride)
        _check_scales("edge_scales_split(%d) %s %s" % (sel, kind, which), mine[:, p_], refl, bound)
        assert torch.equal(bits(mine[:, q_[has]]), bits(mine[:, p_[has]]))
        named = torch.zeros(stride, dtype=torch.bool, device="cuda")
        named[p_] = True
        named[q_[has]] = True
        assert int(named.sum()) == nl + int(has.sum())
        assert _is_payload(mine[:, ~named]) and _is_payload(beyond)


def test_edge_scales_split_zeroes_the_slotted_types_of_a_mixed_batch():
    """A: with one local type refused its polynomial slot (agdiff_local_poly_enabled == 2), which = 1 leaves every entry of a slotted
    type at exactly 0 in all planes -- agdiff_cfconv_local must not count it a second time -- and gives the refused type its scale;
    which = 2 (the quad tiles, read by the polynomial kernel) zeroes nothing."""
    from agdiff_amd import _lib
    lib, st = _lib.load(), _lib.stream_ptr()
    which = "wide"
    m, pk, sd, cfg = _model("qm9", which, "f16x3", radius_poly="auto", refuse=(R.UNSLOTTED_TYPE,))
    topo, ws, pk = _batch(m, _drugs_batch())
    P, T, W = ctypes.byref(pk.struct), ctypes.byref(topo.struct), ctypes.byref(ws.struct)
    assert lib.agdiff_local_poly_enabled(P, T, W) == 2
    d = R.lengths(which)
    nl = min(d.size, topo.Lc)
    dl = _take(d, nl)
    ref = _scale_ref(which, dl, 0)
    bound, _ = _abs_bound(which, dl, 0)
    ty = topo.lc_type[:nl].cpu().numpy()
    slot = pk.slot_table.cpu().numpy()
    slotted = slot[ty] >= 0
    assert slot[R.UNSLOTTED_TYPE] < 0 and slotted.any() and (~slotted).sum() >= 100
    inside = (dl >= 0) & (dl <= R.RC32)
    assert (inside & ~slotted).sum() >= 50
    ws.lc_len[:nl].copy_(torch.from_numpy(dl).cuda())
    ws.num_local_canon.fill_(nl)
    for sel, out, lp, lm in ((1, ws.l_scale, topo.lc_ppos, topo.lc_pmir), (2, ws.lt_scale, topo.lc_tpos, topo.lc_tmir)):
        stride = out.numel() // (2 * _lib.DEFINES["AGDIFF_MAX_CONVS"])
        p_, q_ = lp[:nl].long(), lm[:nl].long()
        has = q_ >= 0
        out.copy_(payload(out.numel(), "cuda"))
        assert lib.agdiff_edge_scales_split(P, T, W, sel, st) == 0
        torch.cuda.synchronize()
        mine, beyond = _planes(out, stride)
        want = np.where(slotted[None, :], 0.0, ref) if sel == 1 else ref
        _check_scales("edge_scales_split(%d) mixed" % sel, mine[:, p_], want, bound)
        assert torch.equal(bits(mine[:, q_[has]]), bits(mine[:, p_[has]]))
        if sel == 1:
            z = mine[:, p_][:, torch.from_numpy(slotted).cuda()]
            assert torch.equal(bits(z), torch.zeros_like(bits(z)))                          # +0, bit for bit


# ------------------------------------------------------------------------------------------------ B: k_rad_scales
@pytest.mark.parametrize("which", ["wide", "narrow"])
@pytest.mark.parametrize("kind", ["qm9", "drugs"])
def test_rad_scales_live_rows_pad_rows_and_payload(kind, which):
    """B: rad_cnt / rad_len filled by the test, counts 0, 1, 15, 16, 17, 32, 33 in turn.  Live rows against float64; rows [cnt,
    roundup16(cnt)) get source = the target, length 0 and scale exactly 0; rows beyond keep what they held."""
    from agdiff_amd import _lib
    lib, st = _lib.load(), _lib.stream_ptr()
    RS = _lib.DEFINES["AGDIFF_RAD_STRIDE"]
    m, pk, sd, cfg = _model(kind, which, "f32")
    smooth = int(cfg.smooth_conv)
    topo, ws, pk = _batch(m, _drugs_batch())
    P, T, W = ctypes.byref(pk.struct), ctypes.byref(topo.struct), ctypes.byref(ws.struct)
    N = topo.N
    cnt = np.asarray(R.RAD_COUNTS)[np.arange(N) % len(R.RAD_COUNTS)]
    assert cnt.max() == _lib.RADIUS_CAP and int(R.r16(cnt).max()) == RS
    live = np.arange(RS)[None, :] < cnt[:, None]
    d = R.lengths(which)
    assert int(live.sum()) >= d.size
    lens = np.zeros((N, RS), dtype=np.float32)
    lens[live] = np.resize(d, int(live.sum()))
    ref_rows = _scale_ref(which, lens.reshape(-1), smooth).reshape(R.NPLANES, N, RS)
    want, written = R.rad_expected(cnt, lens, ref_rows, RS)
    bound, _ = _abs_bound(which, d, smooth)
    other = (np.arange(N)[:, None] + 1) % N * np.ones((1, RS), dtype=np.int64)              # a valid atom that is not the target
    len_in = torch.where(torch.from_numpy(live), torch.from_numpy(lens), payload(N * RS).view(N, RS))
    ws.rad_cnt.copy_(torch.from_numpy(cnt.astype(np.int32)).cuda())
    ws.rad_len.copy_(len_in.reshape(-1).cuda())
    ws.rad_src.copy_(torch.from_numpy(other.astype(np.int32)).reshape(-1).cuda())
    ws.r_scale.copy_(payload(ws.r_scale.numel(), "cuda"))
    assert lib.agdiff_edge_scales_split(P, T, W, 0, st) == 0
    torch.cuda.synchronize()
    mine, beyond = _planes(ws.r_scale, N * RS)
    mine = mine.view(R.NPLANES, N, RS).cpu()
    lv, wr = torch.from_numpy(live), torch.from_numpy(written)
    pad = wr & ~lv
    _check_scales("rad_scales %s %s" % (kind, which), mine[:, lv], ref_rows[:, live], bound)
    z = mine[:, pad]
    assert pad.sum() > 0 and torch.equal(bits(z), torch.zeros_like(bits(z)))                # pad rows: +0 in every plane
    assert _is_payload(mine[:, ~wr]) and _is_payload(beyond)
    got_len, got_src = ws.rad_len.view(N, RS).cpu(), ws.rad_src.view(N, RS).cpu().long()
    assert torch.equal(bits(got_len[lv]), bits(len_in[lv])) and torch.equal(bits(got_len[pad]), torch.zeros_like(bits(got_len[pad])))
    assert _is_payload(got_len[~wr])
    me = torch.arange(N)[:, None].expand(N, RS)
    assert torch.equal(got_src[pad], me[pad]) and torch.equal(got_src[~pad], torch.from_numpy(other)[~pad])
    assert np.isnan(want[:, ~written]).all() and np.all(want[:, pad.numpy()] == 0.0)        # (what edge_ref.rad_expected describes)


# ------------------------------------------------------------------------------------------------ C: the other producers
def _standalone_radius(lib, P, T, W, ws, st):
    """k_rad_scales on the rad_cnt / rad_len the workspace holds: r_scale [12, N, RS] with the payload wherever it does not write"""
    ws.r_scale.copy_(payload(ws.r_scale.numel(), "cuda"))
    assert lib.agdiff_edge_scales_split(P, T, W, 0, st) == 0
    torch.cuda.synchronize()
    return ws.r_scale.clone()


@pytest.mark.parametrize("which", ["wide", "narrow"])
@pytest.mark.parametrize("kind", ["qm9", "drugs"])
def test_graph_builds_and_sampler_front_write_the_same_scales(kind, which):
    """C: agdiff_graph_build_scaled, agdiff_graph_build_large and agdiff_sampler_front(2 | 4) -- with the union table (K = 512 wide,
    64 narrow) and without one -- on edge_ref.producer_batch: molecule A's radius row 0 -> j has length kink_j exactly.  Each
    producer's r_scale on its live rows meets float64 and holds the bits of the stand-alone launch (B) on the same rad_len; the builds'
    pad rows are exactly 0; the front's lt_scale meets float64 on the lengths it wrote to lc_len."""
    from agdiff_amd import _lib
    lib, st = _lib.load(), _lib.stream_ptr()
    RS = _lib.DEFINES["AGDIFF_RAD_STRIDE"]
    m, pk, sd, cfg = _model(kind, which, "f32")
    smooth = int(cfg.smooth_conv)
    b = R.producer_batch(which)
    topo, ws, pk = _batch(m, b)
    assert pk.struct.dist_union and pk.struct.dist_union_kinks == (512 if which == "wide" else 64)
    N = topo.N
    P, T, W = ctypes.byref(pk.struct), ctypes.byref(topo.struct), ctypes.byref(ws.struct)
    no_union = _lib.Params.from_buffer_copy(pk.struct)
    no_union.dist_union = None
    pos = torch.from_numpy(b["pos"]).cuda().contiguous()
    rc = ctypes.c_float(cfg.cutoff)
    sa = _lib.StepArgs()
    sa.pos_in = _lib.ptr(pos)

    def front(params):
        ws.canon_counter.zero_()
        return lib.agdiff_sampler_front(params, T, W, ctypes.byref(sa), 2 | 4, rc, st)

    producers = [("graph_build_scaled", True, lambda: lib.agdiff_graph_build_scaled(P, T, W, _lib.ptr(pos), rc, 1, st)),
                 ("graph_build_large", True, lambda: lib.agdiff_graph_build_large(P, T, W, _lib.ptr(pos), rc, 1, st)),
                 ("sampler_front union", False, lambda: front(P)),
                 ("sampler_front tables", False, lambda: front(ctypes.byref(no_union)))]
    first = None
    for name, pads, run in producers:
        ws.r_scale.copy_(payload(ws.r_scale.numel(), "cuda"))
        ws.rad_len.copy_(payload(ws.rad_len.numel(), "cuda"))
        ws.rad_cnt.zero_()
        ws.lt_scale.copy_(payload(ws.lt_scale.numel(), "cuda"))
        assert run() == 0, name
        torch.cuda.synchronize()
        cnt = ws.rad_cnt.cpu().numpy().astype(np.int64)
        lens = ws.rad_len.view(N, RS).cpu()
        got = _planes(ws.r_scale.clone(), N * RS)[0].view(R.NPLANES, N, RS).cpu()
        live = np.arange(RS)[None, :] < cnt[:, None]
        lv = torch.from_numpy(live)
        assert 0 <= cnt.min() and cnt.max() == _lib.RADIUS_CAP
        nA = b["sizes"][0]
        assert cnt[nA:nA + 2].tolist() == [0, 0] and cnt[nA + 2:nA + 4].tolist() == [1, 1]
        assert cnt[-40:].min() >= _lib.RADIUS_CAP - 3 and np.all(cnt[-6:] == _lib.RADIUS_CAP)         # (the cap keeps the first 33 in reach, self and bonded atoms among them)
        src = ws.rad_src.view(N, RS).cpu().numpy()
        # molecule A: the first row of target j >= 1 comes from atom 0 (but for 1 <-> 2, bonded) and its length is kink_j, bit for bit
        j = np.arange(3, nA)
        assert np.all(src[j, 0] == 0) and np.array_equal(lens[j, 0].numpy(), b["kinks"][2:])
        d = lens[lv].numpy()
        ref = _scale_ref(which, d, smooth)
        bound, _ = _abs_bound(which, d, smooth)
        _check_scales("%s %s %s" % (name, kind, which), got[:, lv], ref, bound)
        if first is None:
            first = (cnt, lens.clone(), got.clone())
        else:       # every producer builds the same rows and scales
            assert np.array_equal(cnt, first[0]) and torch.equal(bits(lens[lv]), bits(first[1][lv]))
            assert torch.equal(bits(got[:, lv]), bits(first[2][:, lv]))
        alone = _planes(_standalone_radius(lib, P, T, W, ws, st), N * RS)[0].view(R.NPLANES, N, RS).cpu()
        assert torch.equal(bits(got[:, lv]), bits(alone[:, lv])), name
        if pads:
            pad = torch.from_numpy((np.arange(RS)[None, :] < R.r16(cnt)[:, None]) & ~live)
            z = got[:, pad]
            assert pad.sum() > 0 and torch.equal(bits(z), torch.zeros_like(bits(z))), name
        if name.startswith("sampler_front"):
            Lc = topo.Lc
            stride = ws.lt_scale.numel() // (2 * _lib.DEFINES["AGDIFF_MAX_CONVS"])
            dl = ws.lc_len[:Lc].cpu().numpy()
            tp, tm = topo.lc_tpos[:Lc].long(), topo.lc_tmir[:Lc].long()
            mine = _planes(ws.lt_scale, stride)[0]
            _check_scales("%s lt_scale %s %s" % (name, kind, which), mine[:, tp], _scale_ref(which, dl, smooth),
                          _abs_bound(which, dl, smooth)[0])
            assert torch.equal(bits(mine[:, tm[tm >= 0]]), bits(mine[:, tp[tm >= 0]]))


# ------------------------------------------------------------------------------------------------ D: k_edge_encoder
def _encoder_inputs(n):
    return _ref(("D in", n), lambda: (R.edge_lengths(n), R.edge_types(n), R.scatter_indices(n), R.row_index_case(n)))


def _unit_is_payload(frag, n_pos):
    """bool [n_pos]: position p of an operand-form buffer still holds the payload in all of its 128 words -- in every mode a
    position's words are [tile][t][half][edge][16 words] (tests/test_hip_parity.py: unfrag)"""
    w = bits(frag).view(-1, 4, 2, 16, 16) == R.PAYLOAD_BITS
    every = w.all(dim=4).all(dim=2).all(dim=1).reshape(-1)
    some = w.any(dim=4).any(dim=2).any(dim=1).reshape(-1)
    assert torch.equal(every, some)                       # a position is written whole or not at all
    return every[:n_pos]


def _check_rows(name, got, ref, length, precision):
    for what, part in (("near", R.near(length)), ("far", ~R.near(length))):
        if part.any():
            check_close("%s %s" % (name, what), got[torch.from_numpy(part)], ref[part], precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("weights", ["synthetic", "expanded"])
@pytest.mark.parametrize("n", R.E_COUNTS + (R.E_ROUNDS,))
def test_edge_encoder_rows_operand_form_row_index_and_scatter(n, weights, precision):
    """D: agdiff_edge_encoder with max_tiles two tiles beyond the live count.  Rows and operand form together, each alone (the same
    bits), twice (the same bits); the rows against the float64 encoder; unfrag(operand form) the rows' values (bit for bit in f32,
    to the split's rounding otherwise); row_index without and with the scatter; payload wherever no edge writes.
    E = 65,537 is 4097 tiles: one more than the 256 workgroups x 16 waves the launcher caps the grid at -- a wave's second tile."""
    from agdiff_amd import _lib
    from test_hip_parity import unfrag
    lib, st = _lib.load(), _lib.stream_ptr()
    m, pk, sd, cfg = _model("qm9", None, precision, weights=weights)
    P = ctypes.byref(pk.struct)
    length, etype, (pos, mir), (ri, n_rows) = _encoder_inputs(n)
    ref = _ref(("D ref", n, weights), lambda: R.mlp_encoder(sd, length, etype).numpy())
    live_tiles = (n + 15) // 16
    tiles = live_tiles + 2
    cap = 16 * tiles
    assert (tiles > 256 * 16) == (n == R.E_ROUNDS) and 0 <= etype.min() and etype.max() < 100
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    len_d, typ_d = _dev(length, cap, torch.float32), _dev(etype, cap, torch.int32)

    def launch(frag, rows, row_index=None, p=None, q=None):
        rc = lib.agdiff_edge_encoder(P, _lib.ptr(n_dev), ctypes.c_int64(tiles), _lib.ptr(len_d), _lib.ptr(typ_d), _lib.ptr(frag),
                                     _lib.ptr(rows), _lib.ptr(row_index), _lib.ptr(p), _lib.ptr(q), st)
        torch.cuda.synchronize()
        return rc

    new_frag = lambda positions: payload((positions + 15) // 16 * 16 * 128, "cuda")
    new_rows = lambda count: payload(count * 128, "cuda").view(count, 128)
    # rows and operand form together
    frag, rows = new_frag(cap), new_rows(cap)
    assert launch(frag, rows) == 0
    _check_rows("edge_encoder E=%d %s" % (n, weights), rows[:n].cpu(), ref, length, precision)
    assert _is_payload(rows[n:]) and _is_payload(frag[live_tiles * 16 * 128:])
    attr = unfrag(frag, n, precision)
    if precision == "f32":
        assert torch.equal(bits(attr), bits(rows[:n]))
    else:
        _check_rows("edge_encoder E=%d %s rows vs operand form" % (n, weights), attr.cpu(), rows[:n].cpu().double().numpy(), length, precision)
    for again in range(2):              # twice more: alone, and the same bits every time
        frag_b, rows_b = new_frag(cap), new_rows(cap)
        assert launch(frag_b, None) == 0 and launch(None, rows_b) == 0
        assert torch.equal(bits(frag_b), bits(frag)) and torch.equal(bits(rows_b), bits(rows))
    # row_index without the scatter: edge e's row is row_index[e]
    plain = np.where(np.arange(n) % 5 == 4, -1, np.random.default_rng(n).permutation(n + 3)[:n]).astype(np.int32)
    assert n < 5 or (plain < 0).any()
    rows_c = new_rows(n + 3)
    assert launch(None, rows_c, row_index=_dev(plain, cap, torch.int32)) == 0
    ok = torch.from_numpy(plain >= 0)
    where = torch.from_numpy(plain).long()[ok]
    assert torch.equal(bits(rows_c[where.cuda()]), bits(rows[:n][ok.cuda()]))
    rest = torch.ones(n + 3, dtype=torch.bool)
    rest[where] = False
    assert _is_payload(rows_c[rest.cuda()])
    # the scatter: operand form at pos_index[e] and mir_index[e], rows through row_index of those positions
    pos_d, mir_d, ri_d = _dev(pos, cap, torch.int32), _dev(mir, cap, torch.int32), _dev(ri, max(cap, 2 * n), torch.int32)
    assert pos.min() >= 0 and max(pos.max(), mir.max()) < 2 * n and ri.max() < n_rows and ri.shape[0] == 2 * n
    frag2, rows2 = new_frag(2 * n), new_rows(n_rows)
    assert launch(frag2, rows2, row_index=ri_d, p=pos_d, q=mir_d) == 0
    has = mir >= 0
    attr2 = unfrag(frag2, 2 * n, precision)
    pl, ml = torch.from_numpy(pos).long().cuda(), torch.from_numpy(mir[has]).long().cuda()
    assert torch.equal(bits(attr2[pl]), bits(attr))
    assert torch.equal(bits(attr2[ml]), bits(attr[torch.from_numpy(has).cuda()]))           # mirrors: bit-equal
    named = torch.zeros(2 * n, dtype=torch.bool)
    named[pl.cpu()] = True
    named[ml.cpu()] = True
    assert named[0] or n < 2                                                                # position 0 is a mirror position
    assert torch.equal(_unit_is_payload(frag2, 2 * n).cpu(), ~named)
    owner, written = R.scatter_expected(np.arange(n, dtype=np.float64)[:, None], n_rows, pos, mir, row_index=ri)
    wr = torch.from_numpy(written)
    who = torch.from_numpy(owner[written, 0].astype(np.int64))
    assert torch.equal(bits(rows2[wr.cuda()]), bits(rows[:n][who.cuda()]))
    assert _is_payload(rows2[(~wr).cuda()]) and int((~wr).sum()) >= 3
    # ... and the operand form alone under the scatter: the same bits
    frag3 = new_frag(2 * n)
    assert launch(frag3, None, p=pos_d, q=mir_d) == 0
    assert torch.equal(bits(frag3), bits(frag2))


# ------------------------------------------------------------------------------------------------ E: flagged tiles
@pytest.mark.parametrize("precision", PRECISIONS)
def test_local_edge_rows_flagged_tiles_row_by_row(precision):
    """E: agdiff_local_edge_rows on edge_ref.flagged_case written into ws.lc_len / topo.lc_type: enc_flags[0] counts the three
    flagged tiles and every mask is as designed (0x0001, 0x8000, all eleven live rows of the last tile; rows hard through a length
    beyond every far set or through the type refused its slot); hard rows are the MLP's and meet the float64 encoder; every other
    row -- tile-mates of a hard row included -- keeps the bits of a run in which the hard rows were soft."""
    from agdiff_amd import _lib
    lib, st = _lib.load(), _lib.stream_ptr()
    m, pk, sd, cfg = _model("qm9", None, precision, radius_poly="auto", refuse=(R.UNSLOTTED_TYPE,))
    topo, ws, pk = _batch(m, _drugs_batch())
    P, T, W = ctypes.byref(pk.struct), ctypes.byref(topo.struct), ctypes.byref(ws.struct)
    c = R.flagged_case()
    E = c["length"].shape[0]
    n_tiles = c["masks"].shape[0]
    slot = pk.slot_table.cpu().numpy()
    assert E <= topo.Lc and pk.struct.poly_kt == 1 and pk.struct.poly_num_slots > 0
    assert slot[R.UNSLOTTED_TYPE] < 0 and np.all(slot[list(R.SLOTTED_TYPES)] >= 0)
    assert not pk.struct.attr_poly_far_slots or float(pk.struct.attr_poly_far_hi) < float(c["length"][c["hard"]].max())
    far_hi = float(pk.struct.attr_poly_far_hi) if pk.struct.attr_poly_far_slots else R.RC
    assert np.all(c["length"][c["length"] > R.RC32] > far_hi)
    ws.num_local_canon.fill_(E)
    out = ws.l_attr_rows.view(-1, 128)

    def run(length, etype):
        ws.lc_len[:E].copy_(torch.from_numpy(length).cuda())
        topo.lc_type[:E].copy_(torch.from_numpy(etype).cuda())
        ws.l_attr_rows.copy_(payload(ws.l_attr_rows.numel(), "cuda"))
        ws.enc_flags.fill_(-1)
        assert lib.agdiff_local_edge_rows(P, T, W, st) == 0
        torch.cuda.synchronize()
        assert _is_payload(out[E:])
        return out[:E].clone(), ws.enc_flags.cpu().numpy()

    soft, flags = run(c["soft_length"], c["soft_type"])
    assert flags[0] == 0 and np.all(flags[1:1 + n_tiles] == 0)
    got, flags = run(c["length"], c["etype"])
    assert flags[0] == 3 and flags[1:1 + n_tiles].tolist() == c["masks"].tolist()
    hard = torch.from_numpy(c["hard"]).cuda()
    ref = R.mlp_encoder(sd, c["length"], c["etype"]).numpy()
    for what, part in (("near", c["hard"] & R.near(c["length"])), ("far", c["hard"] & ~R.near(c["length"]))):
        assert part.any()
        check_close("local_edge_rows hard rows %s" % what, got[torch.from_numpy(part).cuda()], ref[part], precision)
    assert torch.equal(bits(got[~hard]), bits(soft[~hard]))
    assert not torch.equal(bits(got[hard]), bits(soft[hard]))


# ------------------------------------------------------------------------------------------------ F: k_edge_gaussian
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [1, 17, 16 * 13 + 5])
def test_gaussian_edge_encoder(n, precision):
    """F: agdiff_edge_encoder of a Gaussian-encoder model: lengths 0, -0, across [0, 2 rc] and out to 100 rc, where all 64 Gaussians
    underflow to exactly 0; types 0 and 99; rows, operand form and the scatter."""
    from agdiff_amd import _lib
    from test_hip_parity import unfrag
    lib, st = _lib.load(), _lib.stream_ptr()
    m, pk, sd, cfg = _model("qm9-gaussian", None, precision)
    assert pk.struct.edge_encoder == 1
    P = ctypes.byref(pk.struct)
    length, etype = R.gaussian_lengths(n), R.edge_types(n)
    ref = R.gaussian_encoder(sd, length, etype).numpy()
    pos, mir = R.scatter_indices(n)
    tiles = (n + 15) // 16 + 2
    cap = 16 * tiles
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    len_d, typ_d = _dev(length, cap, torch.float32), _dev(etype, cap, torch.int32)
    frag, rows = payload(cap * 128, "cuda"), payload(cap * 128, "cuda").view(cap, 128)
    assert lib.agdiff_edge_encoder(P, _lib.ptr(n_dev), ctypes.c_int64(tiles), _lib.ptr(len_d), _lib.ptr(typ_d), _lib.ptr(frag),
                                   _lib.ptr(rows), None, None, None, st) == 0
    torch.cuda.synchronize()
    check_close("edge_gaussian E=%d" % n, rows[:n], ref, precision)
    assert _is_payload(rows[n:]) and _is_payload(frag[(n + 15) // 16 * 16 * 128:])
    far = torch.from_numpy(length >= np.float32(3.0 * R.RC))
    assert n < 5 or (bool(far.any()) and torch.equal(bits(rows[:n][far.cuda(), :64]), torch.zeros_like(bits(rows[:n][far.cuda(), :64]))))
    emb = sd["edge_encoder_global.bond_emb.weight"][torch.from_numpy(etype).long()]
    assert torch.equal(rows[:n, 64:].cpu(), emb)                                            # the embedding half: copied
    attr = unfrag(frag, n, precision)
    if precision == "f32":
        assert torch.equal(bits(attr), bits(rows[:n]))
    else:
        check_close("edge_gaussian E=%d rows vs operand form" % n, attr, rows[:n].cpu().double().numpy(), precision)
    frag2 = payload((2 * n + 15) // 16 * 16 * 128, "cuda")
    pos_d, mir_d = _dev(pos, cap, torch.int32), _dev(mir, cap, torch.int32)
    assert lib.agdiff_edge_encoder(P, _lib.ptr(n_dev), ctypes.c_int64(tiles), _lib.ptr(len_d), _lib.ptr(typ_d), _lib.ptr(frag2), None,
                                   None, _lib.ptr(pos_d), _lib.ptr(mir_d), st) == 0
    torch.cuda.synchronize()
    has = mir >= 0
    attr2 = unfrag(frag2, 2 * n, precision)
    pl, ml = torch.from_numpy(pos).long().cuda(), torch.from_numpy(mir[has]).long().cuda()
    assert torch.equal(bits(attr2[pl]), bits(attr)) and torch.equal(bits(attr2[ml]), bits(attr[torch.from_numpy(has).cuda()]))
    named = torch.zeros(2 * n, dtype=torch.bool)
    named[pl.cpu()] = True
    named[ml.cpu()] = True
    w = bits(frag2).view(-1, 4, 2, 16, 16) == R.PAYLOAD_BITS
    assert torch.equal(w.all(dim=4).all(dim=2).all(dim=1).reshape(-1)[:2 * n].cpu(), ~named)
