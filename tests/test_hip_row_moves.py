"""GPU (MI355X): the coalesced row moves of csrc/common.hpp (piece layout <-> operand layout: ag_load_slice_pieces, ag_load_row_pieces,
ag_permute4, ag_store_row_pieces) in the kernels that use them -- k_pair_head (h and attr_rows slices), k_pair_head_poly (h slices),
k_edge_attr_poly (row stores), k_schnet_node_stage<f16x3, true> (h_in in, h and xs out) -- through their C-ABI entry points, against
the float64 references the kernels' own test files use (tests/pair_head_ref.py, the float64 MLP edge encoder, tests/node_ref.py) at
helpers.check_close's own tolerances, in the three arithmetic modes.
The lists are the smallest at which a lane map can go wrong (tests/row_moves_cases.py): 1, 15, 16, 17 and 33 entries; pairs on node 0
and node N - 1 with N as small as 2; every row of a tile naming the same nodes; rows whose elements encode (row, feature); with and
without pos_index / mir_index.  Every launch runs twice and the two results hold the same bits; nothing outside the list is written.
For the reference alone every case stays inside the tolerance: float32 against float64 on these inputs, tests/test_row_moves_cases_cpu.py.
Not here: the kernel's segmented walk (HeadPolyArgs.seg_tile_live) -- no entry point reaches it, every launcher passes null, so
agdiff_pair_head_poly_rows is tested on the canonical radius list of agdiff_sampler_front instead; k_gin_layer_persistent -- it runs
only above 65,536 nodes, where tests/test_hip_node_kernels.py::test_gin_large_shapes holds it to the reference (a lone node in a
wave's second round included); the output paths of k_edge_encoder (rows, operand form, row_index, the pos_index / mir_index scatter, a
wave's second tile) -- tests/test_hip_edge_kernels.py."""
import ctypes

import numpy as np
import pytest
import torch

import pair_head_ref as R
import row_moves_cases as C
from helpers import check_close, t
from test_hip_pair_head import PRECISIONS, _dev, _encoder64, _head, _launch, _model

pytestmark = pytest.mark.gpu


def _twice(run):
    """run() -> tensor, two times: the same bits (a lane map that reads a stale or foreign register rarely repeats itself)"""
    a, b = run(), run()
    assert torch.equal(R.bits(a), R.bits(b))
    return a


def _check_scatter(name, out2, pos, mir, ref, precision):
    p, q = torch.from_numpy(pos).long(), torch.from_numpy(mir).long()
    has = q >= 0
    check_close(name, out2[p.cuda()], ref, precision)
    assert torch.equal(R.bits(out2[q[has].cuda()]), R.bits(out2[p[has].cuda()]))
    named = torch.zeros(out2.numel(), dtype=torch.bool)
    named[p] = True
    named[q[has]] = True
    rest = out2.cpu()[~named]
    assert torch.equal(R.bits(rest), R.bits(R.payload(rest.numel())))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", C.PAIRS)
def test_pair_head_rows(kind, precision):
    """k_pair_head on attr_rows: both heads, plain and scattered through pos_index / mir_index"""
    m, pk, sd, cfg = _model(C.ACT, "synthetic", precision)
    for e in C.COUNTS:
        tiles = (e + 15) // 16 + 1
        cap = 16 * tiles
        pos, mir = R.scatter_indices(e)
        pos_d, mir_d = _dev(pos, cap, torch.int32), _dev(mir, cap, torch.int32)
        for head in ("global", "local"):
            src, dst, h, attr, ref = C.head_case(sd, kind, e, head)
            src_d, dst_d, h_d, rows_d = _dev(src, cap, torch.int32), _dev(dst, cap, torch.int32), h.cuda(), _dev(attr, cap, torch.float32)

            def plain():
                out = R.payload(cap, "cuda")
                assert _launch(_head(pk, head), e, tiles, src_d, dst_d, h_d, out, rows=rows_d) == 0
                return out

            def scattered():
                out = R.payload(2 * e, "cuda")
                assert _launch(_head(pk, head), e, tiles, src_d, dst_d, h_d, out, rows=rows_d, pos=pos_d, mir=mir_d) == 0
                return out

            out = _twice(plain)
            check_close("row moves pair_head %s %s E=%d" % (kind, head, e), out[:e], ref, precision)
            assert torch.equal(R.bits(out[e:]), R.bits(R.payload(cap - e)))
            out2 = _twice(scattered)
            _check_scatter("row moves pair_head %s %s E=%d scattered" % (kind, head, e), out2, pos, mir, ref, precision)
            assert torch.equal(R.bits(out2[torch.from_numpy(pos).long().cuda()]), R.bits(out[:e]))      # the same arithmetic


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", C.PAIRS)
def test_pair_head_poly_rows_of_a_plain_list(kind, precision):
    """k_pair_head_poly through agdiff_pair_head_poly, plain and scattered"""
    from agdiff_amd import _lib
    m, pk, sd, cfg = _model(C.ACT, "synthetic", precision, radius_poly="auto")
    assert pk.poly_kt >= 1
    lib = _lib.load()
    for e in C.COUNTS:
        src, dst, h, length, ref = C.head_case(sd, kind, e, "global", encoder=lambda d: _encoder64(sd, d), cutoff=cfg.cutoff)
        tiles = (e + 15) // 16 + 1
        cap = 16 * tiles
        src_d, dst_d, h_d, len_d = _dev(src, cap, torch.int32), _dev(dst, cap, torch.int32), h.cuda(), _dev(length, cap, torch.float32)
        pos, mir = R.scatter_indices(e)
        pos_d, mir_d = _dev(pos, cap, torch.int32), _dev(mir, cap, torch.int32)
        n_dev = torch.tensor([e], dtype=torch.int32, device="cuda")

        def run(n_out, pos_t, mir_t):
            out = R.payload(n_out, "cuda")
            assert lib.agdiff_pair_head_poly(ctypes.byref(pk.struct), _lib.ptr(n_dev), ctypes.c_int64(tiles), _lib.ptr(src_d), _lib.ptr(dst_d),
                                             _lib.ptr(len_d), _lib.ptr(h_d), _lib.ptr(pos_t), _lib.ptr(mir_t), _lib.ptr(out),
                                             _lib.stream_ptr()) == 0
            torch.cuda.synchronize()
            return out

        out = _twice(lambda: run(cap, None, None))
        check_close("row moves pair_head_poly %s E=%d" % (kind, e), out[:e], ref, precision)
        assert torch.equal(R.bits(out[e:]), R.bits(R.payload(cap - e)))
        out2 = _twice(lambda: run(2 * e, pos_d, mir_d))
        _check_scatter("row moves pair_head_poly %s E=%d scattered" % (kind, e), out2, pos, mir, ref, precision)
        assert torch.equal(R.bits(out2[torch.from_numpy(pos).long().cuda()]), R.bits(out[:e]))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pair_head_poly_over_the_canonical_radius_list_with_coded_rows(precision):
    """agdiff_pair_head_poly_rows after agdiff_sampler_front (c_pos / c_mir: mirrors present), node rows coded by (node, feature)"""
    from agdiff_amd import _lib, synth
    m, pk, sd, cfg = _model(C.ACT, "synthetic", precision, radius_poly="auto")
    assert pk.poly_kt >= 1
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
    h = C.coded_rows(N, C.H_LO)
    ws.h.view(-1, 128)[:N].copy_(h.cuda())
    sa = _lib.StepArgs()
    sa.pos_in = _lib.ptr(pos)
    ws.canon_counter.zero_()
    ws.range_rows.zero_()
    assert lib.agdiff_sampler_front(P, Tp, Wp, ctypes.byref(sa), 2 | 4, ctypes.c_float(cfg.cutoff), st) == 0

    def run():
        ws.inv_r.copy_(R.payload(ws.inv_r.numel(), "cuda"))
        assert lib.agdiff_pair_head_poly_rows(P, Tp, Wp, 0, st) == 0
        torch.cuda.synchronize()
        return ws.inv_r[: N * RS].clone()

    inv_r = _twice(run)
    n_c = int(ws.canon_counter[0].item())
    assert n_c > 16
    c_src, c_dst, c_len = ws.c_src[:n_c].cpu(), ws.c_dst[:n_c].cpu(), ws.c_len[:n_c].cpu()
    p, q = ws.c_pos[:n_c].cpu().numpy(), ws.c_mir[:n_c].cpu().numpy()
    assert (q >= 0).any()
    ref = R.pair_head(sd, "global", C.ACT, h, c_src.numpy(), c_dst.numpy(), _encoder64(sd, c_len))[0]
    _check_scatter("row moves pair_head_poly_rows", inv_r, p, q, ref, precision)
    assert int(ws.range_rows.sum()) == 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_local_edge_attr_rows_element_by_element(precision):
    """k_edge_attr_poly through agdiff_local_edge_rows on a canonical local list of 1, 16 and 17 edges of mixed types (the live count is
    the device word num_local_canon; lengths and types are this test's): every element of every live row against the float64 MLP edge
    encoder, rows beyond the list untouched.  With 17 edges one row lies far beyond the cutoff: the polynomial kernel leaves it to
    the encoder MLP (a flagged row), whose result meets the same gate."""
    from agdiff_amd import _lib, drugs_model_config, synth
    from oracle import agdiff_oracle as O
    from test_hip_poly import _model as poly_model
    lib = _lib.load()
    cfg = drugs_model_config(num_diffusion_timesteps=20, beta_end=2e-5)
    m = poly_model(cfg, "auto", precision=precision)
    b = synth.make_packed_batch("drugs", 3, 1, seed=31)
    at, bi, bt, ba = [t(b[k]).cuda() for k in ("atom_type", "bond_index", "bond_type", "batch")]
    pos = torch.randn(at.shape[0], 3, generator=torch.Generator().manual_seed(8)) * 1.5
    m(at, pos.cuda(), bi, bt, ba, None, extend_order=False)
    topo, ws, pk = m._batch_cache[1], m._batch_cache[2], m.packed()
    assert pk.struct.poly_num_slots > 0 and topo.Lc >= 32
    sd64 = {k: v.detach().cpu().double() for k, v in m.state_dict().items() if k.startswith("edge_encoder_global.")}
    present = np.unique(topo.lc_type[: topo.Lc].cpu().numpy())
    assert present.size >= 2
    P, T, W, st = ctypes.byref(pk.struct), ctypes.byref(topo.struct), ctypes.byref(ws.struct), _lib.stream_ptr()
    rows_all = ws.l_attr_rows.view(-1, 128)
    for e in (1, 16, 17):
        types = present[(np.arange(e) * 5 + 1) % present.size]                      # mixed within every tile
        length = C.lengths(e, cfg.cutoff).clone()
        if e == 17:
            length[5] = 100.0 * cfg.cutoff
        ws.num_local_canon.fill_(e)
        ws.lc_len[:e].copy_(length.cuda())
        topo.lc_type[:e].copy_(torch.from_numpy(types).to(torch.int32).cuda())
        ref = O.mlp_edge_encoder(sd64, "edge_encoder_global", length.double().view(-1, 1), torch.from_numpy(types).long())

        def run():
            rows_all.view(-1).copy_(R.payload(rows_all.numel(), "cuda"))
            assert lib.agdiff_local_edge_rows(P, T, W, st) == 0
            torch.cuda.synchronize()
            return rows_all.clone()

        got = _twice(run)
        flags = ws.enc_flags.cpu().numpy()
        assert flags[0] == (1 if e == 17 else 0) and flags[1] == (1 << 5 if e == 17 else 0)
        check_close("row moves local_edge_rows E=%d" % e, got[:e], ref, precision)
        assert torch.equal(R.bits(got[e:].reshape(-1)), R.bits(R.payload(got[e:].numel())))


@pytest.mark.parametrize("n", C.NODE_COUNTS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_node_stage_rows(precision, n):
    """k_schnet_node_stage<MODE, true> (weights shared through LDS, forced at these sizes) on 1, 16 and 17 nodes with coded rows, against
    tests/node_ref.py: in split fp16 h_in comes in and h and xs go out through the piece layout, the other two modes keep the
    operand-layout rows and are held to the same reference.  (k_gin_layer_persistent runs only
    above 65,536 nodes: tests/test_hip_node_kernels.py::test_gin_large_shapes is its test, a lone node in a wave's second round
    included.)"""
    from test_hip_node_kernels import SENTINEL, _case
    c = _case(precision, "n%d" % n)
    h_in, agg = C.node_case(n)
    out = c.stage(C.NODE_STAGE, 1, "ldsw", h=h_in, agg=agg)
    again = c.stage(C.NODE_STAGE, 1, "ldsw", h=h_in, agg=agg)
    for key in ("h", "xs"):
        assert np.array_equal(out[key].view(np.int32), again[key].view(np.int32))
    c.check_stage("row moves ldsw", out, C.NODE_STAGE, h_in, agg)
    assert np.all(out["h0"] == SENTINEL) and np.all(out["xs0"] == SENTINEL)
