"""GPU (MI355X): the radius-graph rule in all five places that implement it -- k_graph, k_lg_thr / k_lg_count / k_lg_fill
(csrc/graph.hip) and the graph phase of k_sampler_front (csrc/front.hip) -- through every entry point, bit for bit against the NumPy
restatement tests/graph_ref.py on inputs that take the rule to its limits (their design is proved without a GPU in
tests/test_graph_ref_cpu.py): pairs within an ulp of the cutoff and exact ties, the cap on either side of a ballot boundary, self as
the 33rd and 34th candidate, every launch shape of the LDS build and the scan over more than 1024 graphs, a batch without any edge
and an empty molecule.
  A  agdiff_graph_build, _ex(0 | 1), _scaled(0 | 1): every output buffer over its live range, nothing written beyond it (buffers
     start as a sentinel), with and without the count -> fill hand-over (ws.g_inbits), two builds bitwise equal
  B  agdiff_graph_build_large forced on the same batches, with and without scales
  C  agdiff_sampler_front(2 | 4), quads and single targets (pad rows off / on), both parities: radius rows, the canonical radius
     list per molecule, canon_counter
  D  one length in all five copies: e_len, agdiff_local_lengths' l_len / lc_len / l_len_p / lt_len, the front's, rad_len
No gate is new: indices and lengths are exact; r_scale meets float64 at the gates of tests/test_hip_edge_kernels.py, whose model
(distance-weighting networks with chosen kinks), reference and checks are used as they are.  The envelope takes the model's cutoff
(10) whatever cutoff the graph is built with, so the 3.7 batches are compared too."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import graph_ref as GR
import test_hip_edge_kernels as EK
from helpers import t

pytestmark = pytest.mark.gpu

SENT_I, SENT_F = -77777, -777.25
INT_OUT = ("num_edges", "graph_edge_cnt", "graph_edge_ptr", "in_ptr", "out_ptr", "e_src", "e_dst", "e_type", "ref2dst", "e_loc",
           "num_canon", "graph_canon_cnt", "graph_canon_ptr", "c_type", "c_src", "c_dst", "c_pos", "c_mir", "rad_cnt", "rad_src",
           "canon_counter")
FLT_OUT = ("e_len", "c_len", "rad_len", "r_scale", "l_len", "lc_len", "l_len_p", "lt_len")
KIND, WHICH = "drugs", "wide"          # the model of tests/test_hip_edge_kernels.py: smooth envelope, twelve networks with wide kinks
SMALL = [n for n in GR.BATCHES if max(GR.make_batch(n)["sizes"]) <= 512]
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
SENT_BITS = int(bits([SENT_F])[0])


@functools.lru_cache(maxsize=None)
def _setup(name, gt=4):
    """(batch, topology grouped gt targets per wave, packed weights, positions on the device, library)"""
    from agdiff_amd import _lib
    from agdiff_amd.topology import BatchTopology
    m, _, _, cfg = EK._model(KIND, WHICH, "f32")
    assert cfg.cutoff == EK.R.RC
    b = GR.make_batch(name)
    topo = BatchTopology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], b["num_graphs"], device="cuda", group_targets=gt)
    assert topo.group_targets == gt and topo.large == (max(b["sizes"]) > _lib.MAX_ATOMS_PER_GRAPH)
    with torch.no_grad():
        pk = m._renorm_embedding(t(b["atom_type"]).cuda())
    return b, topo, pk, t(b["pos"]).cuda().contiguous(), _lib.load()


def _workspace(topo):
    from agdiff_amd.topology import Workspace
    ws = Workspace(topo)
    for k in INT_OUT:
        getattr(ws, k).fill_(SENT_I)
    for k in FLT_OUT:
        getattr(ws, k).fill_(SENT_F)
    return ws


def _snap(ws):
    torch.cuda.synchronize()
    return {k: getattr(ws, k).cpu().numpy() for k in INT_OUT + FLT_OUT}


def _same(a, b, keys=INT_OUT + FLT_OUT):
    for k in keys:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def _build(name, entry, ronly, ws=None, handover=True):
    """One build into a sentinel-filled workspace; returns its buffers.  handover=False: the same workspace struct with g_inbits
    null (the fill pass then repeats the count pass's work instead of reading its masks)."""
    from agdiff_amd import _lib
    b, topo, pk, pos, lib = _setup(name)
    ws = _workspace(topo) if ws is None else ws
    w = ws.struct
    if not handover:
        assert ws.g_inbits is not None
        w = _lib.Workspace.from_buffer_copy(ws.struct)
        w.g_inbits = None
    T, W, P = ctypes.byref(topo.struct), ctypes.byref(w), ctypes.byref(pk.struct)
    c, st, p = ctypes.c_float(b["cutoff"]), _lib.stream_ptr(), _lib.ptr(pos)
    ws.variant_log.zero_()
    if entry == "plain":
        rc = lib.agdiff_graph_build(T, W, p, c, st)
    elif entry == "ex":
        rc = lib.agdiff_graph_build_ex(T, W, p, c, ronly, st)
    elif entry == "scaled":
        rc = lib.agdiff_graph_build_scaled(P, T, W, p, c, ronly, st)
    else:
        rc = lib.agdiff_graph_build_large(P if entry == "large_scaled" else None, T, W, p, c, ronly, st)
    assert rc == 0, (name, entry, ronly, rc)
    out = _snap(ws)
    took_large = bool(int(ws.variant_log.item()) & _lib.DEFINES["AGDIFF_VAR_GRAPH_LARGE"])
    assert took_large == (entry.startswith("large") or topo.large), (name, entry)
    return out


def _live_and_rest(got, want, sentinel, what):
    """got[: len(want)] == want bit for bit and everything behind it still the sentinel"""
    n = want.shape[0]
    if want.dtype == np.float32:
        assert np.array_equal(bits(got[:n]), bits(want)), what
        assert np.all(bits(got[n:]) == SENT_BITS), what + ": written past its end"
    else:
        assert np.array_equal(got[:n].astype(np.int64), want), what
        assert np.all(got[n:] == sentinel), what + ": written past its end"


def _check_scales(what, got, lens):
    """r_scale rows got [12, n] on the lengths the device wrote: the float64 reference and gates of tests/test_hip_edge_kernels.py"""
    if lens.size == 0:
        return
    smooth = int(EK._model(KIND, WHICH, "f32")[3].smooth_conv)
    EK._check_scales(what, got, EK._scale_ref(WHICH, lens, smooth), EK._abs_bound(WHICH, lens, smooth)[0])


def _check_rows(what, out, ref, N, pads, scaled):
    """rad_cnt / rad_src / rad_len against the reference; pads: rows [cnt, roundup16(cnt)) hold (src = target, length +0, scale +0);
    every other row past a target's count is untouched.  scaled: r_scale written (live rows against float64), else untouched."""
    RS = GR.RS
    cnt = ref["rad_cnt"]
    assert np.array_equal(out["rad_cnt"].astype(np.int64), cnt), what
    live = np.arange(RS)[None, :] < cnt[:, None]
    pad = (np.arange(RS)[None, :] < ((cnt + GR.TW - 1) // GR.TW * GR.TW)[:, None]) & ~live if pads else np.zeros_like(live)
    src, ln = out["rad_src"].reshape(N, RS), out["rad_len"].reshape(N, RS)
    assert np.array_equal(src[live].astype(np.int64), ref["rad_src"][live]), what
    assert np.array_equal(bits(ln[live]), bits(ref["rad_len"][live])), what
    me = np.broadcast_to(np.arange(N)[:, None], (N, RS))
    assert np.array_equal(src[pad], me[pad]) and np.all(bits(ln[pad]) == 0), what + ": pad rows"
    rest = ~live & ~pad
    assert np.all(src[rest] == SENT_I) and np.all(bits(ln[rest]) == SENT_BITS), what + ": rows past the count written"
    sc = out["r_scale"].reshape(-1, N, RS)
    if not scaled:
        assert np.all(bits(sc) == SENT_BITS), what + ": r_scale written"
        return
    mine, beyond = sc[:EK.R.NPLANES], sc[EK.R.NPLANES:]
    assert np.all(bits(beyond) == SENT_BITS) and np.all(bits(mine[:, rest]) == SENT_BITS), what + ": r_scale written past the rows"
    assert np.all(bits(mine[:, pad]) == 0), what + ": pad scales"
    _check_scales(what + " r_scale", mine[:, live].astype(np.float64), ln[live])


def _check_build(what, out, ref, b, ronly, scaled):
    N, G = b["batch"].shape[0], b["num_graphs"]
    E, c = ref["num_edges"], ref["canon"][ronly]
    assert int(out["num_edges"][0]) == E and int(out["num_canon"][0]) == c["num_canon"], what
    for k in ("e_src", "e_dst", "e_type", "ref2dst", "e_loc", "e_len"):
        _live_and_rest(out[k], ref[k], SENT_I, "%s %s" % (what, k))
    for k in ("c_src", "c_dst", "c_type", "c_pos", "c_mir", "c_len"):
        _live_and_rest(out[k], c[k], SENT_I, "%s %s" % (what, k))
    for k, want in (("in_ptr", ref["in_ptr"]), ("out_ptr", ref["out_ptr"]), ("graph_edge_cnt", ref["graph_edge_cnt"]),
                    ("graph_edge_ptr", ref["graph_edge_ptr"]), ("graph_canon_cnt", c["graph_canon_cnt"]),
                    ("graph_canon_ptr", c["graph_canon_ptr"])):
        assert out[k].shape[0] == want.shape[0] and np.array_equal(out[k].astype(np.int64), want), "%s %s" % (what, k)
    _check_rows(what, out, ref, N, pads=scaled, scaled=scaled)
    assert np.all(out["canon_counter"] == SENT_I)


LDS_VARIANTS = [("plain", 0), ("ex", 0), ("ex", 1), ("scaled", 0), ("scaled", 1)]


def test_every_output_of_a_build_is_among_the_checked_buffers():
    """What a build writes, as tests/test_hip_large_molecules.py lists it for both paths (the large path fills the per-graph counts and
    pointers from its atom-order prefix sums): every one of those buffers starts as a sentinel here and is compared."""
    from test_hip_large_molecules import OUTPUTS
    assert set(OUTPUTS) <= set(INT_OUT + FLT_OUT)


# ------------------------------------------------------------------------------------------------ A: the ordinary entry points
@pytest.mark.parametrize("name", GR.BATCHES)
def test_graph_build_entry_points_bit_for_bit(name):
    """A: agdiff_graph_build, agdiff_graph_build_ex and agdiff_graph_build_scaled, each canon_radius_only 0 and 1: k_graph at 1024
    and 512 threads and 2..16 mask words, k_scan_graphs with its carry; clusters520 takes the large path by itself.  With the
    count -> fill hand-over and without it; a second build gives the same bits."""
    b, topo, _, _, _ = _setup(name)
    ref = GR.reference(name)
    for entry, ronly in LDS_VARIANTS:
        what = "%s %s(%d)" % (name, entry, ronly)
        out = _build(name, entry, ronly)
        _check_build(what, out, ref, b, ronly, entry == "scaled")
        _same(out, _build(name, entry, ronly))
        if not topo.large:
            _same(out, _build(name, entry, ronly, handover=False))


# ------------------------------------------------------------------------------------------------ B: the large path
@pytest.mark.parametrize("name", GR.BATCHES)
def test_large_build_forced_bit_for_bit(name):
    """B: agdiff_graph_build_large on every batch, with scales (p) and without, canon_radius_only 0 and 1: k_lg_thr (the 33rd
    candidate on either side of a ballot boundary), k_lg_count / k_lg_fill (self at and behind the threshold, one-way edges),
    k_lg_scan, lg_graph_of stepping over an empty molecule."""
    b = _setup(name)[0]
    ref = GR.reference(name)
    for entry in ("large", "large_scaled"):
        for ronly in (0, 1):
            out = _build(name, entry, ronly)
            _check_build("%s %s(%d)" % (name, entry, ronly), out, ref, b, ronly, entry == "large_scaled")
            _same(out, _build(name, entry, ronly))


# ------------------------------------------------------------------------------------------------ C: the front's graph phase
def _front(name, gt, parity, ws=None):
    from agdiff_amd import _lib
    b, topo, pk, pos, lib = _setup(name, gt)
    ws = _workspace(topo) if ws is None else ws
    ws.canon_counter[parity] = 0                 # (the live word: molecules add to it; the other one the kernel zeroes itself)
    sa = _lib.StepArgs()
    sa.pos_in = _lib.ptr(pos)
    rc = lib.agdiff_sampler_front(ctypes.byref(pk.struct), ctypes.byref(topo.struct), ctypes.byref(ws.struct), ctypes.byref(sa),
                                  2 | 4 | (16 if parity else 0), ctypes.c_float(b["cutoff"]), _lib.stream_ptr())
    assert rc == 0, (name, gt, parity, rc)
    return _snap(ws)


@pytest.mark.parametrize("gt", [4, 1])
@pytest.mark.parametrize("name", SMALL)
def test_sampler_front_graph_phase_bit_for_bit(name, gt):
    """C: agdiff_sampler_front(2 | 4 [| 16]) on a topology of quads (pad rows off) and one of single targets (pad rows on): radius
    rows and r_scale as the builds'; the canonical radius list per molecule -- molecules claim their range by an atomic, so their
    order is free; inside a range the order is fixed -- with c_pos / c_mir as radius rows; canon_counter[parity] the count, the
    other word zeroed; nothing of the full edge list touched."""
    b, topo, _, _, _ = _setup(name, gt)
    ref = GR.reference(name)
    N = b["batch"].shape[0]
    c = ref["canon"][1]
    C = c["num_canon"]
    for parity in (0, 1):
        what = "%s front gt%d parity %d" % (name, gt, parity)
        out = _front(name, gt, parity)
        _check_rows(what, out, ref, N, pads=gt != 4, scaled=True)
        assert out["canon_counter"].tolist() == ([C, 0] if parity == 0 else [0, C]), what
        src, dst, pos_, mir = (out[k][:C].astype(np.int64) for k in ("c_src", "c_dst", "c_pos", "c_mir"))
        mol = b["batch"][dst]
        order = np.lexsort((pos_, mol))
        assert np.array_equal(src[order], c["c_src"]) and np.array_equal(dst[order], c["c_dst"]), what
        assert np.array_equal(pos_[order], c["row_pos"]) and np.array_equal(mir[order], c["row_mir"]), what
        assert np.array_equal(bits(out["c_len"][:C][order]), bits(c["c_len"])), what
        # a molecule's entries are one contiguous range in the reference's order
        runs = 1 + int((np.diff(mol) != 0).sum()) if C else 0
        assert runs == np.unique(mol).size and np.all(np.diff(pos_)[np.diff(mol) == 0] > 0), what
        for k in ("c_src", "c_dst", "c_pos", "c_mir"):
            assert np.all(out[k][C:] == SENT_I), what
        assert np.all(bits(out["c_len"][C:]) == SENT_BITS), what
        for k in ("num_edges", "num_canon", "in_ptr", "out_ptr", "e_src", "e_dst", "e_type", "ref2dst", "e_loc", "c_type",
                  "graph_edge_cnt", "graph_edge_ptr", "graph_canon_cnt", "graph_canon_ptr"):
            assert np.all(out[k] == SENT_I), (what, k)
        assert np.all(bits(out["e_len"]) == SENT_BITS), what
        # a second launch: the same bits everywhere but in the list, whose molecules may come in another order
        _same(out, _front(name, gt, parity), [k for k in INT_OUT + FLT_OUT if k not in ("c_src", "c_dst", "c_pos", "c_mir", "c_len")])


# ------------------------------------------------------------------------------------------------ D: one length everywhere
def _check_local_lengths(what, out, ref, topo):
    """l_len by local edge, lc_len by canonical local edge, l_len_p by padded slot, lt_len by quad-tile row: the reference's length of
    the edge, bit for bit, and nothing else written"""
    Lc = topo.Lc
    want = ref["l_len"]
    _live_and_rest(out["l_len"], want, None, what + " l_len")
    canon_len = np.zeros(Lc, dtype=np.float32)
    canon_len[ref["loc_row"]] = want              # (mirrors carry the same bits: asserted through l_len above)
    _live_and_rest(out["lc_len"], canon_len, None, what + " lc_len")
    g = lambda x: x.cpu().numpy().astype(np.int64)
    for buf, cpos, cmir in (("l_len_p", g(topo.lc_ppos), g(topo.lc_pmir)), ("lt_len", g(topo.lc_tpos), g(topo.lc_tmir))):
        exp = np.full(out[buf].shape[0], SENT_F, dtype=np.float32)
        exp[cpos] = canon_len
        exp[cmir[cmir >= 0]] = canon_len[cmir >= 0]
        assert np.array_equal(bits(out[buf]), bits(exp)), "%s %s" % (what, buf)


@pytest.mark.parametrize("name", GR.BATCHES)
def test_one_length_in_every_copy(name):
    """D: for every local edge the bits of e_len (the build), of l_len / lc_len / l_len_p / lt_len (agdiff_local_lengths, and the
    front's local phase) and of graph_ref's definition are the same; for every radius edge those of e_len, rad_len of the build and
    rad_len of the front."""
    from agdiff_amd import _lib
    b, topo, pk, pos, lib = _setup(name)
    ref = GR.reference(name)
    ws = _workspace(topo)
    out = _build(name, "ex", 0, ws=ws)
    assert lib.agdiff_local_lengths(ctypes.byref(topo.struct), ctypes.byref(ws.struct), _lib.ptr(pos), _lib.stream_ptr()) == 0
    out = _snap(ws)
    E = ref["num_edges"]
    _check_local_lengths(name + " local_lengths", out, ref, topo)
    loc = out["e_loc"][:E]
    assert np.array_equal(loc >= 0, ref["e_type"] > 0)
    assert np.array_equal(bits(out["e_len"][:E][loc >= 0]), bits(out["lc_len"][loc[loc >= 0]]))
    live = np.arange(GR.RS)[None, :] < out["rad_cnt"][:, None]
    assert np.array_equal(bits(out["rad_len"].reshape(-1, GR.RS)[live]), bits(out["e_len"][:E][loc < 0]))
    assert np.array_equal(bits(out["e_len"][:E]), bits(ref["e_len"]))
    if not topo.large:
        front = _front(name, 4, 0)
        _check_local_lengths(name + " front", front, ref, topo)
        _same(front, out, ("rad_cnt", "l_len", "lc_len", "l_len_p", "lt_len"))
        assert np.array_equal(bits(front["rad_len"].reshape(-1, GR.RS)[live]), bits(out["e_len"][:E][loc < 0]))
