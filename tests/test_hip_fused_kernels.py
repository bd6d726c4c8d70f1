"""GPU (MI355X): k_cfconv_fused (csrc/edge.hip) through its two C-ABI entries, agdiff_cfconv_fused and agdiff_cfconv_local, against the
float64 restatement of tests/fused_ref.py (anchored on the CPU by tests/test_fused_ref_cpu.py).

Everything the kernel reads is DATA written here: in_ptr, e_src, e_dst and num_edges; the twelve scale planes at the plane stride the
launcher derives from the capacity (NaN wherever a launch may not read, 0.75 in the pad of the last tile, where it must select 0);
e_attr through fused_ref.frag (finite decoy rows in the pad of the last tile); xs.  The reference consumes the operands the kernel
gets (hi + lo of the mode).  Capacities come from byte copies of agdiff_topo_t (max_edges) and agdiff_ws_t (pointers to test-owned
buffers of the size the header states for that capacity) next to a BatchTopology / Workspace of the library's.  agg and agg_first
start out as pair_head_ref.payload: every row outside fused_ref.split's write sets must keep it bit for bit -- except the empty
lists strictly inside a tile of three or more targets, whose zero sums the general reduction stores (payload or zeros there).
ws.variant_log is asserted after every launch.  Every comparison: helpers.check_close at the mode's gates, scale 1.

  A  shapes (E = 368, 369, 383, 1, 0) x blocks 0, 2, 5, eight tiles per chunk: one / two / three / sixteen / 76 targets per tile,
     flush, carry over six whole tiles, hubs from offsets 0, 1, 15, partial last tiles
  B  chunks at 1, 2 and 8 tiles per chunk (capacities searched with agdiff_conv_chunk_tiles): agg and agg_first SEPARATELY
  C  rounds: 33,900 edges on 256 workgroups (two rounds, remap on); its prefixes on 3, 8 and 16 workgroups; bitwise equal lists
  D  two launches, the same bits
  E  agdiff_cfconv_local on the padded local list of stars with local in-degrees 1, 7, 8, 9, 33, 64; one type's scales zeroed

Which case fails if the kernel is off by one:
  the `run_t != t0` flush      A and B at two or more tiles per chunk: the lists that end exactly on a tile end inside a chunk (the
                               16-edge targets of tiles 0 and 1, the lists ending on 128, 176, 256) lose their row or get the next
                               target's sum; the payload stays in a row of split's write set, which is not finite.
  the `lo >= e_begin` test     B: the lists that start exactly on a chunk boundary (`>` sends them to agg_first: agg keeps its
                               payload, agg_first[c] is written outside its write set); with `e_begin + 1` the list that starts one
                               edge before a boundary lands in agg_first.  The separate comparison sees either.
  the `i >= 64` form of bound  A and B: the tile with 76 targets has four one-edge lists at indices 72..75; a bound taken one entry
                               off gives them an empty or a doubled mask: rows 0 or twice the reference.
  the `2k + 1` plane           every case at blocks 2 and 5: the planes are independent draws with their own zeros, so channels
                               128..191 come out with another plane's scales (the CPU mutation "scales_swapped": normwise 0.7).
  the cross-chunk prefetch     C on 256 workgroups: the second-round chunks 2048.. would run on the attributes, sources and scales of
                               a neighbouring chunk; their lists miss the reference (first-round lists stay right).  The prefixes on
                               small grids never take that branch and keep agreeing, which tells the two apart.

Expectation, before any run: about 2^-20 per product in the split modes, sums of at most 100 rows x 128 terms -- well inside the
gates.  Measured on MI355X (worst over the group; normwise / element-wise, in brackets the share of TOL_NORM / TOL_ELEM):
       f32                               bf16x3                            f16x3
  A    1.9e-6 / 6.2e-4  (0.39 / 0.31)    8.6e-6 / 2.3e-3  (0.29 / 0.08)    4.6e-6 / 7.2e-4  (0.23 / 0.14)
  B    1.8e-6 / 1.1e-3  (0.36 / 0.54)    7.7e-6 / 3.6e-3  (0.26 / 0.12)    4.4e-6 / 1.2e-3  (0.22 / 0.24)
  C    1.6e-6 / 6.9e-4  (0.31 / 0.35)    5.7e-6 / 3.2e-3  (0.19 / 0.11)    3.5e-6 / 2.2e-3  (0.17 / 0.43)
  E    1.3e-6 / 6.9e-4  (0.25 / 0.34)    6.4e-6 / 1.6e-3  (0.21 / 0.05)    1.8e-6 / 6.0e-4  (0.09 / 0.12)
  D    bit for bit
One figure is past half its gate: the element-wise one of B in f32 (0.54, agg of the chunks list at one tile per chunk, block 5).
The errors grow with the square root of the list length in every mode and do not depend on the tile path.
Found by A, B and C: split-bf16 missed its normwise gate on the lists of 64 to 100 edges -- 3.1e-5 (A, shapes mod0, block 5),
5.8e-5 (B, chunks at two tiles per chunk, block 5), 3.3e-5 (C, the 2,048-edge prefix) against 3e-5, E at 2.8e-5 -- because the second
filter layer took s = softplus / ln 2 (near 1) as its split operand, with the shift folded into the bias; it now takes s - 1 in that
mode (csrc/edge.hip: ag_conv_ssp).  f32 and f16x3 run the instructions they ran before."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fused_ref as FR
import node_ref as NR
from helpers import check_close, t
from pair_head_ref import bits, payload

pytestmark = pytest.mark.gpu
PRECISIONS = ["f32", "bf16x3", "f16x3"]
BLOCKS = (0, 2, 5)
EXTRA = 8                                          # rows of agg / agg_first past what the launch owns
NAN = float("nan")


# ------------------------------------------------------------------------------------------------- model, rig
@functools.lru_cache(maxsize=None)
def _model(precision):
    from agdiff_amd import _lib, drugs_model_config, get_model
    cfg = drugs_model_config()
    m = get_model(cfg)
    m.precision, m.precision_local, m.radius_poly = precision, precision, "off"
    m.load_state_dict({k: v.clone() for k, v in NR.state_dict(cfg).items()}, strict=True)
    m = m.to("cuda:0").eval()
    pk = m.packed()
    assert m.effective_precision == precision and pk.struct.num_convs == 6
    return m, cfg, _lib.load()


@functools.lru_cache(maxsize=None)
def _sd64():
    from agdiff_amd import drugs_model_config
    return NR.to64(NR.state_dict(drugs_model_config()))


def _i32(a):
    return t(np.ascontiguousarray(a).astype(np.int32)).cuda().view(-1)


def _f32(a):
    return t(np.ascontiguousarray(a, dtype=np.float32)).cuda().view(-1)


def _chunk_tiles(lib, cap):
    return int(lib.agdiff_conv_chunk_tiles(ctypes.c_int64(int(cap))))


def _smallest_capacity(lib, ct):
    return FR.smallest_capacity(ct, rule=lambda cap: _chunk_tiles(lib, cap))


class Rig:
    """A model in one mode and the library's topology / workspace of `n` atoms (copies of an 8-atom molecule): ws.in_ptr, ws.xs and
    ws.num_edges are the library's own buffers; the edge-sized ones are the test's, sized for the capacity of each launch."""

    def __init__(self, precision, n):
        from agdiff_amd.topology import Workspace
        self.m, self.cfg, self.lib = _model(precision)
        self.precision, self.N = precision, n
        b = NR.tiled_batch(n)
        self.topo = self.m.prepare_topology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], b["num_graphs"], False, device="cuda:0")
        self.ws = Workspace(self.topo)
        assert self.topo.N == n and self.ws.in_ptr.numel() == n + 1 and self.ws.xs.numel() == n * 192

    def launch(self, ip, d, cap, k):
        """One agdiff_cfconv_fused(k) over the list `ip` with the data `d` (fused_ref.inputs) at capacity `cap`.
        dict(agg [N + EXTRA, 192], first [chunks + EXTRA, 192] float32 arrays, ct, ce, chunks)."""
        from agdiff_amd import _lib
        ws, N, E, epad = self.ws, self.N, d["E"], d["epad"]
        assert ip.shape[0] == N + 1 and E <= cap and d["N"] == N
        ct = _chunk_tiles(self.lib, cap)
        max_tiles = (cap + FR.TW - 1) // FR.TW
        stride = max_tiles * FR.TW
        chunks = (max_tiles + ct - 1) // ct
        ws.in_ptr.copy_(_i32(ip))
        ws.num_edges.fill_(E)
        ws.xs.copy_(_f32(d["xs"]))
        live = min(epad, stride)                                          # (E = 0: one decoy tile, if the capacity has one)
        dst = np.zeros(epad, dtype=np.int64)
        dst[:E] = d["dst"]
        e_src, e_dst = _i32(d["src_pad"]), _i32(dst)
        e_attr = FR.frag(d["attr"], self.precision).cuda()
        planes = torch.full((FR.NPLANES, stride), NAN, dtype=torch.float32, device="cuda:0")
        planes[:, :live].copy_(_f32(d["planes"][:, :live]).view(FR.NPLANES, live))
        agg = payload((N + EXTRA) * 192, "cuda:0")
        first = payload((chunks + EXTRA) * 192, "cuda:0")
        T = type(self.topo.struct).from_buffer_copy(self.topo.struct)
        T.max_edges = cap
        W = type(ws.struct).from_buffer_copy(ws.struct)
        W.e_src, W.e_dst, W.e_attr, W.e_scale = _lib.ptr(e_src), _lib.ptr(e_dst), _lib.ptr(e_attr), _lib.ptr(planes.view(-1))
        W.agg, W.agg_first = _lib.ptr(agg), _lib.ptr(first)
        pk = self.m.packed()
        ws.variant_log.zero_()
        rc = self.lib.agdiff_cfconv_fused(ctypes.byref(pk.struct), ctypes.byref(T), ctypes.byref(W), k, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        assert int(ws.variant_log.item()) == _lib.DEFINES["AGDIFF_VAR_CFCONV_FUSED"]
        return dict(agg=agg.view(-1, 192).cpu().numpy(), first=first.view(-1, 192).cpu().numpy(), ct=ct, ce=FR.TW * ct, chunks=chunks)


@functools.lru_cache(maxsize=2)
def _rig(precision, n):
    return Rig(precision, n)


@functools.lru_cache(maxsize=None)
def _list(name):
    """(in_ptr, inputs) of a design: "shapes:mod15", "chunks:32", "rounds", "rounds:384" (the prefix within 384 edges)."""
    kind, _, arg = name.partition(":")
    if kind == "shapes":
        ip = FR.shapes(arg)
    elif kind == "chunks":
        ip = FR.chunks(int(arg))
    else:
        ip = FR.rounds()
        if arg:
            ip = FR.prefix(ip, int(arg))
    ip.setflags(write=False)
    d = FR.inputs("rounds" if kind == "rounds" else name, FR.rounds() if kind == "rounds" else ip)
    if kind == "rounds" and arg:                                          # the same data, cut to the prefix
        E = int(ip[-1])
        epad = max((E + FR.TW - 1) // FR.TW, 1) * FR.TW
        d = dict(d, src=d["src"][:E], src_pad=d["src_pad"][:epad], dst=d["dst"][:E], attr=d["attr"][:epad], planes=d["planes"][:, :epad].copy(),
                 E=E, epad=epad)
        d["planes"][:, E:] = 0.75
    return ip, d


@functools.lru_cache(maxsize=64)
def _reference(name, precision, k, ce):
    """fused_ref.split of the float64 messages of design `name`, block k, on the operands of `precision`, for chunks of ce edges;
    plus the aggregate itself."""
    ip, d = _list(name)
    E = d["E"]
    ops = FR.operands(d["attr"][:E], precision)
    msg = FR.messages(_sd64(), None, k, ops, d["planes"][2 * k][:E], d["planes"][2 * k + 1][:E], d["src"], d["xs"])
    sp = FR.split(ip, msg, ce)
    sp["ref"] = NR.gathered_aggregate(ip, sp["agg"], sp["agg_first"], ce)
    return sp


def _close(fails, name, got, ref, precision):
    """helpers.check_close (prints and records both figures, asserts the mode's gates); a miss is kept in `fails` and raised at the
    end of the test, so that one run measures every case of it."""
    try:
        check_close(name, got, ref, precision)
    except AssertionError as e:
        fails.append(str(e))


def _payload_rows(a):
    """Rows of a float32 array that hold the payload bit for bit."""
    return (a.view(np.int32) == bits(payload(1)).item()).all(axis=1)


def _check_write_sets(out, ip, sp, cl):
    """Rows outside split's write sets keep the payload; the empty lists inside a general tile hold the payload or zeros; written
    rows are finite; nothing past the buffers' ends."""
    agg, first = out["agg"], out["first"]
    keep = _payload_rows(agg)
    may = np.zeros(agg.shape[0], dtype=bool)
    may[sp["rows_agg"]] = True
    zero_ok = np.zeros(agg.shape[0], dtype=bool)
    zero_ok[cl["zeroed"]] = True
    assert not (may & zero_ok).any()
    assert np.all(keep[~may & ~zero_ok]), np.nonzero(~keep & ~may & ~zero_ok)[0][:8]
    z = zero_ok & ~keep
    assert np.all(agg[z].view(np.int32) == 0)
    assert np.isfinite(agg[may]).all(), np.nonzero(may & ~np.isfinite(agg).all(axis=1))[0][:8]
    keep_f = _payload_rows(first)
    may_f = np.zeros(first.shape[0], dtype=bool)
    may_f[sp["rows_first"]] = True
    assert keep_f[0] and np.all(keep_f[~may_f]), np.nonzero(~keep_f & ~may_f)[0][:8]
    assert np.isfinite(first[may_f]).all()


def _check(fails, group, rig, name, cap, k, separate=False):
    ip, d = _list(name)
    out = rig.launch(ip, d, cap, k)
    sp = _reference(name, rig.precision, k, out["ce"])
    cl = FR.classify(ip, d["E"], out["ct"], cap)
    assert cl["chunks"] == out["chunks"]
    _check_write_sets(out, ip, sp, cl)
    tag = "fused %s %s k%d ct%d" % (group, name, k, out["ct"])
    if d["E"]:
        got = NR.gathered_aggregate(ip, out["agg"][: rig.N], out["first"], out["ce"])
        _close(fails, tag, got, sp["ref"], rig.precision)
    if separate:
        ra, rf = sp["rows_agg"], sp["rows_first"]
        _close(fails, tag + " agg", out["agg"][ra], sp["agg"][ra], rig.precision)
        _close(fails, tag + " agg_first", out["first"][rf], sp["agg_first"][rf], rig.precision)
    return out, sp, cl


# ------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_shapes_every_tile_path(precision):
    """A.  The five variants of the shapes list x blocks 0, 2, 5 at the smallest capacity with eight tiles per chunk."""
    rig = _rig(precision, FR.N_SMALL)
    cap = _smallest_capacity(rig.lib, FR.MAX_CHUNK_TILES)
    fails = []
    for v in FR.SHAPES:
        for k in BLOCKS:
            out, sp, cl = _check(fails, "A", rig, "shapes:" + v, cap, k)
            assert out["ct"] == FR.MAX_CHUNK_TILES and cl["grid"] == 256
            if v == "none":                                               # E = 0 writes nothing
                assert _payload_rows(out["agg"]).all() and _payload_rows(out["first"]).all()
            if v == "one":
                assert (~_payload_rows(out["agg"])).sum() == 1
    assert not fails, fails


# ------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("ct", [1, 2, FR.MAX_CHUNK_TILES])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_b_chunks_agg_and_agg_first_separately(precision, ct):
    """B.  The chunks list of 16 ct edges per chunk at the smallest capacity for which agdiff_conv_chunk_tiles returns ct (found by
    bisection; at one tile per chunk the capacity is the live count itself).  agg and agg_first each against fused_ref.split."""
    rig = _rig(precision, FR.N_SMALL)
    name = "chunks:%d" % (FR.TW * ct)
    cap = max(_smallest_capacity(rig.lib, ct), int(_list(name)[0][-1]))
    fails = []
    for k in (2, 5):
        out, sp, cl = _check(fails, "B", rig, name, cap, k, separate=True)
        assert out["ct"] == ct and sp["rows_first"].size >= 7
    assert not fails, fails


# ------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("precision", PRECISIONS)
def test_c_rounds_and_small_grids(precision):
    """C.  33,900 live edges at one tile per chunk on 256 workgroups: 2,119 chunks for 2,048 waves, so 71 waves walk a second chunk
    whose first tile the cross-chunk prefetch fetched; XCD remap on.  A capacity bounds the live count, so the grids of 3, 8 and 16
    workgroups (remap off / on / on) run the prefix of the same list that fits them.  Every launch against float64; every list that
    lies in whole tiles of a prefix has the same bits in all launches that contain it (one summation order)."""
    rig = _rig(precision, FR.N_ROUNDS)
    k, fails = 2, []
    big, sp, cl = _check(fails, "C", rig, "rounds", 40000, k)
    assert (cl["grid"], cl["remap"], cl["rounds"], big["ct"]) == (256, True, 2, 1)
    for cap, grid, remap in ((384, 3, False), (1024, 8, True), (2048, 16, True)):
        out, sp_c, cl_c = _check(fails, "C", rig, "rounds:%d" % cap, cap, k)
        assert (cl_c["grid"], cl_c["remap"], cl_c["rounds"], out["ct"]) == (grid, remap, 1, 1)
        ip = _list("rounds:%d" % cap)[0]
        whole = int(ip[-1]) // FR.TW * FR.TW
        rows = np.asarray([i for i in sp_c["rows_agg"] if ip[i + 1] <= whole], dtype=np.int64)
        firsts = np.asarray([c for c in sp_c["rows_first"] if (c + 1) * FR.TW <= whole], dtype=np.int64)
        assert rows.size > 20 and firsts.size > 3
        assert np.array_equal(out["agg"][rows].view(np.int32), big["agg"][rows].view(np.int32))
        assert np.array_equal(out["first"][firsts].view(np.int32), big["first"][firsts].view(np.int32))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("precision", PRECISIONS)
def test_d_two_launches_give_the_same_bits(precision):
    """D.  agg and agg_first of two launches on the same inputs, at eight and at two tiles per chunk."""
    rig = _rig(precision, FR.N_SMALL)
    for name, ct in (("shapes:mod15", FR.MAX_CHUNK_TILES), ("chunks:32", 2)):
        ip, d = _list(name)
        cap = _smallest_capacity(rig.lib, ct)
        a, b = rig.launch(ip, d, cap, 5), rig.launch(ip, d, cap, 5)
        assert a["ct"] == ct
        assert np.array_equal(a["agg"].view(np.int32), b["agg"].view(np.int32))
        assert np.array_equal(a["first"].view(np.int32), b["first"].view(np.int32))


# ------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("precision", PRECISIONS)
def test_e_local_list_with_pads_and_a_slotted_type(precision):
    """E.  agdiff_cfconv_local on the library's padded local list of fused_ref.star_batch (local in-degrees 1, 7, 8, 9, 33, 64; lists
    padded to eight entries; a partial last tile): l_attr_frag through frag with finite decoy rows at the pads, l_scale 0 at every
    pad and drawn elsewhere, against the float64 sum over the REAL local edges.  Then type 2 "slotted": its scales 0 in all planes --
    the reference without its edges, and the same bits whatever its attribute rows hold."""
    from agdiff_amd import _lib
    from agdiff_amd.topology import Workspace
    m, cfg, lib = _model(precision)
    b = FR.star_batch()
    topo = m.prepare_topology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], b["num_graphs"], False, device="cuda:0")
    ws = Workspace(topo)
    N, Lp = topo.N, topo.Lp
    g = lambda x: x.cpu().numpy().astype(np.int64)
    lp_ptr, lp_src, lp_dst, lp_type, real = g(topo.lp_ptr), g(topo.lp_src), g(topo.lp_dst), g(topo.lp_type), g(topo.lp_row) >= 0
    assert set(np.bincount(lp_dst[real], minlength=N).tolist()) == {1, 7, 8, 9, 33, 64} and Lp % FR.TW != 0
    ptiles = (Lp + FR.TW - 1) // FR.TW
    stride = ptiles * FR.TW
    ct = _chunk_tiles(lib, Lp)
    ce = FR.TW * ct
    assert ws.l_scale.numel() >= FR.NPLANES * stride and ws.agg_first_loc.numel() == (ptiles + ct - 1) // ct * 192
    d = FR.inputs("stars", lp_ptr)
    assert d["E"] == Lp and d["N"] == N
    pad = np.nonzero(~real)[0]
    planes = d["planes"].copy()
    planes[:, pad] = 0.0
    attr = d["attr"]                                                      # (drawn rows everywhere: the pads' are the finite decoys)
    ws.xs.copy_(_f32(d["xs"]))
    ws.l_scale.fill_(NAN)
    ws.l_scale.view(-1, stride)[: FR.NPLANES].copy_(_f32(planes).view(FR.NPLANES, stride))
    P, T, W = ctypes.byref(m.packed().struct), ctypes.byref(topo.struct), ctypes.byref(ws.struct)
    cl = FR.classify(lp_ptr, Lp, ct, Lp)
    assert {tl["path"] for tl in cl["tiles"]} == {"one", "two", "general"} and max(tl["ntg"] for tl in cl["tiles"]) == 3

    def run(k, attr_rows, plane_rows):
        ws.l_attr_frag.copy_(FR.frag(attr_rows, precision).cuda())
        ws.l_scale.view(-1, stride)[: FR.NPLANES].copy_(_f32(plane_rows).view(FR.NPLANES, stride))
        ws.agg_loc.copy_(payload(ws.agg_loc.numel(), "cuda:0"))
        ws.agg_first_loc.copy_(payload(ws.agg_first_loc.numel(), "cuda:0"))
        ws.variant_log.zero_()
        rc = lib.agdiff_cfconv_local(P, T, W, k, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and int(ws.variant_log.item()) == _lib.DEFINES["AGDIFF_VAR_CFCONV_LOCAL_MLP"]
        return dict(agg=ws.agg_loc.view(-1, 192).cpu().numpy(), first=ws.agg_first_loc.view(-1, 192).cpu().numpy())

    def reference(k, plane_rows, live):
        e = np.nonzero(live)[0]
        ops = FR.operands(attr[e], precision)
        return FR.cfconv_fused(_sd64(), cfg, k, ops, plane_rows[2 * k][e], plane_rows[2 * k + 1][e], lp_src[e], lp_dst[e], d["xs"])

    fails = []
    for k in BLOCKS:
        out = run(k, attr, planes)
        msg = FR.messages(_sd64(), cfg, k, FR.operands(attr[:Lp], precision), planes[2 * k][:Lp], planes[2 * k + 1][:Lp], lp_src, d["xs"])
        _check_write_sets(out, lp_ptr, FR.split(lp_ptr, msg, ce), cl)
        got = NR.gathered_aggregate(lp_ptr, out["agg"], out["first"], ce)
        _close(fails, "fused E stars k%d" % k, got, reference(k, planes, real), precision)
    # one local type "slotted": 0 in all planes (what agdiff_edge_scales_split(1) writes in a mixed batch)
    k, slotted = 2, (lp_type == 2) & real
    assert slotted.sum() > 30
    planes2 = planes.copy()
    planes2[:, : Lp][:, slotted] = 0.0
    out = run(k, attr, planes2)
    got = NR.gathered_aggregate(lp_ptr, out["agg"], out["first"], ce)
    _close(fails, "fused E slotted type k%d" % k, got, reference(k, planes2, real & ~slotted), precision)
    attr2 = attr.copy()
    attr2[: Lp][slotted] = NR.draw("attr:stars:other", (int(slotted.sum()), 128), NR.ATTR_STD)
    again = run(k, attr2, planes2)
    assert np.array_equal(out["agg"].view(np.int32), again["agg"].view(np.int32))
    assert np.array_equal(out["first"].view(np.int32), again["first"].view(np.int32))
    assert not fails, fails
