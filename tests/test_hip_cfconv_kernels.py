"""GPU (MI355X): k_cfconv_quad and k_cfconv_node (csrc/nodeconv.hip) through their C-ABI entry agdiff_cfconv_node, on a topology and
a workspace the library sized, against the float64 restatement of tests/cfconv_ref.py (anchored on the CPU by
tests/test_cfconv_ref_cpu.py).

Everything the kernels read is DATA here.  The coefficient sets are drawn (cfconv_ref.coefficient_sets: every k-tile carries
weight, the one-pass terms of plans 1..3 exactly the weight their bound allows), packed as PackedParams._pack_filter_sets packs a
fit, and hung into a byte copy of the model's agdiff_params_t together with poly_kt, poly_plan, the slot table and 2^-S -- so no
case pays for a 64-, 96- or 128-term fit, and no k-tile multiplies coefficients that are zero to rounding.  The row tables
(cfconv_ref.tables) go into ws.rad_cnt / rad_src / rad_len / r_scale (12 planes, each its own draw), ws.lt_len / lt_scale and
ws.xs; they keep the host's invariants (valid sources everywhere, scale 0 in a target's pad rows), so a wrong read shows as a
wrong number: NaN scales beyond what a launch may use, decoy lengths where k_cfconv_quad must select 0.  The aggregate goes to a
test-owned buffer with eight rows more than the batch, NaN (or a sentinel) before the launch.  ws.variant_log is zeroed before
and asserted after every launch against cfconv_ref.launch.  Every comparison: helpers.check_close at the mode's gates, scale = 1.

Expectation, before any run: about 2^-20 per product in f16x3 and up to ~50 rows x 128 terms per sum -- well inside the gates; the
measured figures are in DESIGN.md §2."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cfconv_ref as CR
import node_ref as NR
from helpers import check_close, t

pytestmark = pytest.mark.gpu
PRECISIONS = ["f32", "bf16x3", "f16x3"]
SENTINEL = -777.25
NAN = float("nan")
BLOCKS = (0, 2, 5)
EXTRA = 8                                          # rows of the aggregate buffer past N
NODE = {"cfconv_quad_tiles": -1}
TWELVE = {"cfconv_four_min_quads": -1}
SIXTEEN = {"cfconv_four_min_quads": 1}


# ------------------------------------------------------------------------------------------------- model, batch, sets
@functools.lru_cache(maxsize=None)
def _model(precision):
    """One model per precision on node_ref.state_dict, 32-term radius fit ("auto"; poly_passes "full": no typed fits for a plan the
    copies overwrite anyway).  It exists to provide a valid agdiff_params_t."""
    from agdiff_amd import _lib, drugs_model_config, get_model
    cfg = drugs_model_config()
    m = get_model(cfg)
    m.precision, m.precision_local, m.radius_poly, m.poly_passes = precision, precision, "auto", "full"
    m.load_state_dict({k: v.clone() for k, v in NR.state_dict(cfg).items()}, strict=True)
    m = m.to("cuda:0").eval()
    pk = m.packed()
    assert m.effective_precision == precision and pk.poly_kt == 1 and pk.struct.num_convs == CR.NCONV
    return m, cfg, _lib.load()


def _slot_table(name, tv):
    types = [int(ty) for ty in np.unique(tv["lt_type"]) if name != "types" or ty in CR.SLOTTED]
    table = np.full(100, -1, dtype=np.int64)
    table[types] = np.arange(len(types))
    return table, len(types)


@functools.lru_cache(maxsize=None)
def _host(name, gt):
    """(view, tables, slot table, number of slots) of a batch at `gt` targets per group, from a host-side topology."""
    tv = CR.view(CR.topology(name, gt))
    tb = CR.tables(tv, name, 10.0, slotted=CR.SLOTTED if name == "types" else None)
    return (tv, tb) + _slot_table(name, tv)


@functools.lru_cache(maxsize=256)
def _reference(name, gt, kt, plan, mode, k):
    """float64 aggregate of block k, once for every mode that shares the sets (plan 0: all three)."""
    tv, tb, table, ns = _host(name, gt)
    rad, typed, _ = CR.coefficient_sets(name, kt, plan, mode if plan else 0, ns, k)
    ref = CR.cfconv(rad, typed, table, (tv, tb), tb["xs"], 10.0, k)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=8)
def _device_sets(name, kt, plan, mode, ns):
    """Blocks 0, 2, 5: (radius set, typed sets, S) packed and on the device."""
    out = {}
    for k in BLOCKS:
        rad, typed, S = CR.coefficient_sets(name, kt, plan, mode if plan else 0, ns, k)
        dev = lambda a: t(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        out[k] = (dev(CR.pack_filter_sets(rad, kt, plan, mode, S)),
                  dev(np.concatenate([CR.pack_filter_sets(c, kt, plan, mode, S) for c in typed])) if ns else None, S)
    return out


class Bench:
    """One batch on the device in one mode: topology (model.group_targets -> prepare_topology), workspace, the injected tables."""

    def __init__(self, precision, name, gt=4):
        from agdiff_amd import _lib
        from agdiff_amd.topology import Workspace
        self.m, self.cfg, self.lib = _model(precision)
        self.precision, self.mode, self.name, self.gt = precision, CR.MODES[precision], name, gt
        b = CR.make_batch(name)
        self.m.group_targets = gt
        try:
            self.topo = self.m.prepare_topology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], b["num_graphs"],
                                                b["extend_order"], device="cuda:0")
        finally:
            self.m.group_targets = None
        self.ws = Workspace(self.topo)
        self.tv, self.tb, self.table, self.ns = _host(name, gt)
        tv, tb, ws = self.tv, self.tb, self.ws
        N, T = tv["N"], tv["T"]
        self.N = N
        assert self.topo.group_targets == gt and np.array_equal(CR.view(self.topo)["quad_tgt"], tv["quad_tgt"])
        assert np.array_equal(CR.view(self.topo)["lt_src"], tv["lt_src"]) and self.topo.T == T
        i32 = lambda a: t(np.ascontiguousarray(a).astype(np.int32)).cuda().view(-1)
        f32 = lambda a: t(np.ascontiguousarray(a, dtype=np.float32)).cuda().view(-1)
        ws.rad_cnt.copy_(i32(tb["rad_cnt"]))
        ws.rad_src.copy_(i32(tb["rad_src"]))
        ws.rad_len.copy_(f32(tb["rad_len"]))
        ws.r_scale.fill_(NAN)
        ws.r_scale[: 2 * CR.NCONV * N * CR.RS].copy_(f32(tb["r_scale"]))
        if T:
            ws.lt_len.copy_(f32(tb["lt_len"]))
            ws.lt_scale.fill_(NAN)
            ws.lt_scale.view(2 * CR.MAX_CONVS, -1)[: 2 * CR.NCONV].copy_(f32(tb["lt_scale"]).view(2 * CR.NCONV, -1))
        ws.xs.copy_(f32(tb["xs"]))
        self.agg = torch.empty((N + EXTRA) * 192, dtype=torch.float32, device="cuda:0")
        self.W = type(ws.struct).from_buffer_copy(ws.struct)
        self.W.agg = _lib.ptr(self.agg)
        self.slot_dev = i32(self.table)
        self.inputs = [ws.rad_cnt, ws.rad_src, ws.rad_len, ws.r_scale, ws.lt_len, ws.lt_scale, ws.xs, self.topo.quad_tgt,
                       self.topo.lt_ptr, self.topo.lt_src, self.topo.lt_type]
        self.before = [x.clone() for x in self.inputs]
        self.zero_rows = np.nonzero((tb["rad_cnt"] == 0) & (np.bincount(tb["lt_tgt"][tb["lt_live"]], minlength=N) == 0))[0]

    def params(self, kt, plan, k, tuning):
        """A byte copy of the model's agdiff_params_t (tune_* through set_tuning) with the drawn sets of block k hung in."""
        from agdiff_amd import _lib
        self.m.tuning = dict(tuning or {})
        s = self.m.packed().struct
        self.m.tuning = {}
        p = type(s).from_buffer_copy(s)
        self.m.packed()                           # (the model's own struct back at tuning = {})
        rad, typed, S = _device_sets(self.name, kt, plan, self.mode, self.ns)[k]
        p.conv[k].filt_poly_pk = _lib.ptr(rad)
        p.conv[k].filt_poly_typed_pk = _lib.ptr(typed)
        p.conv[k].filt_poly_unscale = 2.0 ** -S
        p.poly_kt, p.poly_plan = kt, plan
        p.poly_type_slot, p.poly_num_slots = _lib.ptr(self.slot_dev), self.ns
        sm = [0, 0]
        for ty in np.nonzero(self.table >= 0)[0]:
            sm[int(ty) >> 6] |= 1 << (int(ty) & 63)
        for w in (0, 1):
            p.poly_slot_mask[w] = sm[w]
        self._keep = (rad, typed)
        return p

    def run(self, kt, plan, k, tuning=None, fill=NAN, ranges=True):
        """One launch: the aggregate [N, 192] (float32 array).  Asserts the status, the variant word, finite rows < N, untouched
        rows past N, untouched inputs.  ranges=False: through a copy of agdiff_topo_t without quad_wg_ptr."""
        from agdiff_amd import _lib
        p = self.params(kt, plan, k, tuning)
        T = self.topo.struct
        if not ranges:
            T = type(T).from_buffer_copy(T)
            T.quad_wg_ptr = None
        want = CR.launch(self.tv["Q"], kt, tuning, group_targets=self.gt, num_slots=self.ns if self.tv["T"] else 0,
                         have_ranges=ranges and self.topo.quad_wg_ptr is not None)
        lp = self.lib.agdiff_local_poly_enabled(ctypes.byref(p), ctypes.byref(self.topo.struct), ctypes.byref(self.W))
        assert lp == (0 if not self.tv["T"] else 2 if self.name == "types" else 1)
        self.agg.fill_(fill)
        self.ws.variant_log.zero_()
        rc = self.lib.agdiff_cfconv_node(ctypes.byref(p), ctypes.byref(T), ctypes.byref(self.W), k, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        assert int(self.ws.variant_log.item()) == want["bits"], (hex(int(self.ws.variant_log.item())), hex(want["bits"]))
        out = self.agg.view(-1, 192).cpu().numpy()
        tail = out[self.N:]
        assert np.isfinite(out[: self.N]).all() and (np.isnan(tail).all() if fill != fill else np.all(tail == fill))
        for a, b in zip(self.inputs, self.before):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        self.shape = want
        return out[: self.N].copy()

    def check(self, what, got, kt, plan, k):
        ref = _reference(self.name, self.gt, kt, plan, self.mode, k)
        assert np.all(got[self.zero_rows] == 0.0)
        return check_close("cfconv %s %s gt%d kt%d plan%d k%d" % (what, self.name, self.gt, kt, plan, k), got, ref, self.precision)


@functools.lru_cache(maxsize=4)
def _bench(precision, name, gt=4):
    return Bench(precision, name, gt)


def _plans(precision):
    return [kp for kp in CR.KT_PLANS if precision != "f32" or kp[1] == 0]


def _variants(kt):
    """(label, tuning): both kernels; at one k-tile both wave shapes."""
    shapes = [("12w", TWELVE), ("16w", SIXTEEN)] if kt == 1 else [("", {})]
    return [("quad" + s, dict(tn)) for s, tn in shapes] + [("node" + s, dict(tn, **NODE)) for s, tn in shapes]


# ------------------------------------------------------------------------------------------------- 1. every instantiation
@pytest.mark.parametrize("precision,name,kt,plan", [(pr, n, kt, pl) for pr in PRECISIONS for n in ("rows", "hub", "types") for kt, pl in _plans(pr)])
def test_every_instantiation(precision, name, kt, plan):
    """1.  k_cfconv_quad and k_cfconv_node<MODE, NKT, WAVES, PLAN> for every (kt, plan) the launcher knows (f32: plan 0), blocks 0, 2
    and 5 (the 2 k / 2 k + 1 scale planes), at kt 1 in the 12- and the 16-wave shape; k_cfconv_node also on groups of two and of
    one target.  rows: molecules of 1 .. 64 atoms, every radius count of CNT_CHOICES, quad tails with one to three missing
    targets, quads without tiles, the arranged quads, one pre-filled launch per kernel (zero rows are WRITTEN as zeros).
    hub: several tiles of one type in a quad.  types: seven slotted types -- 5 / 2 / 1 / 0 sets in LDS at kt 1 / 2 / 3 / 4, the rest
    from L2, and every typed set from L2 at poly_lds_sets = 1 -- and one type without a slot, whose NaN scales are ignored."""
    b = _bench(precision, name)
    for k in BLOCKS:
        for label, tn in _variants(kt):
            fill = SENTINEL if k == 2 else NAN
            b.check(label, b.run(kt, plan, k, tn, fill=fill), kt, plan, k)
            assert b.shape["kernel"] == label[:4] and b.shape["four"] == label.endswith("16w")
            if name == "types":
                assert b.shape["lds_slots"] == {1: 5, 2: 2, 3: 1, 4: 0}[kt]
        if name == "types":
            for tn in ({"poly_lds_sets": 1}, dict(NODE, poly_lds_sets=1)):
                b.check("L2 sets", b.run(kt, plan, k, tn), kt, plan, k)
                assert b.shape["lds_slots"] == 0
    for gt in (2, 1):
        g = _bench(precision, name, gt)
        for k in BLOCKS:
            g.check("node", g.run(kt, plan, k, {}), kt, plan, k)
            assert g.shape["kernel"] == "node"


# ------------------------------------------------------------------------------------------------- 2. bits
@pytest.mark.parametrize("kernel", ["quad", "node"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_wave_shapes_agree_and_launches_repeat_bit_for_bit(precision, kernel):
    """2.  The 12- and the 16-wave shape of a kernel give the same bits (a quad's result does not depend on the wave that computes
    it), and so does a repeated launch."""
    b = _bench(precision, "rows")
    extra = NODE if kernel == "node" else {}
    for kt, plan in [(1, 0)] + ([(1, 1)] if precision != "f32" else []):
        a12 = b.run(kt, plan, 2, dict(TWELVE, **extra)).view(np.int32)
        a16 = b.run(kt, plan, 2, dict(SIXTEEN, **extra)).view(np.int32)
        again = b.run(kt, plan, 2, dict(TWELVE, **extra)).view(np.int32)
        assert np.array_equal(a12, again) and np.array_equal(a12, a16)
    for kt, plan in ((2, 0), (4, 0)):
        assert np.array_equal(b.run(kt, plan, 5, extra).view(np.int32), b.run(kt, plan, 5, extra).view(np.int32))


# ------------------------------------------------------------------------------------------------- 3. workgroup walk
# (Q, tuning) -> (grid, quads per workgroup, quads of the last one, XCD remap).  Below 256 workgroups the last workgroup is never
# empty (tests/test_cfconv_ref_cpu.py: test_launch_lds_sets_and_variant_words); test 4 has empty ranges.
WALKS = [(84, TWELVE, (7, 12, 12, False)), (96, TWELVE, (8, 12, 12, True)), (97, TWELVE, (9, 11, 9, False)), (192, TWELVE, (16, 12, 12, True)),
         (97, SIXTEEN, (7, 14, 13, False)), (1, TWELVE, (1, 1, 1, False))]


@pytest.mark.parametrize("Q,tuning,shape", WALKS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_workgroup_walk_without_ranges(precision, Q, tuning, shape):
    """3.  Q molecules of four atoms = Q quads (every fifth without any tile): grids of 7, 8, 9 and 16 workgroups, 8 and 16 through
    the XCD remap; a last workgroup with 9 quads for 12 waves and with 13 for 16; one quad in one workgroup with eleven idle
    waves."""
    b = _bench(precision, "q%d" % Q)
    assert b.tv["Q"] == Q
    for kernel in ({}, NODE):
        got = b.run(1, 0, 0, dict(tuning, **kernel))
        assert (b.shape["grid"], b.shape["per_wg"], b.shape["last"], b.shape["remap"]) == shape and not b.shape["ranges"]
        b.check("walk", got, 1, 0, 0)


# ------------------------------------------------------------------------------------------------- 4. ranges
def _written_ranges(Q, waves):
    """quad_wg_ptr as data: two empty ranges, three quads, a range of 5 waves + 1 quads that starts and ends with a quad without
    tiles, one quad, three empty ranges, equal shares, six empty ranges at the end."""
    w = [0, 0, 0, 3, 3 + 5 * waves + 1]
    w.append(w[-1] + 1)
    w += [w[-1]] * 3
    rest = 251 - len(w)
    w += list(np.linspace(w[-1], Q, rest + 1).astype(np.int64)[1:])
    w += [Q] * (257 - len(w))
    w = np.asarray(w, dtype=np.int64)
    assert w.shape[0] == 257 and w[0] == 0 and w[-1] == Q and np.all(np.diff(w) >= 0)
    return w


@pytest.mark.parametrize("Q,kt,tuning", [(4081, 1, SIXTEEN), (3061, 1, TWELVE), (2041, 4, {})])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ranges_on_a_grid_of_256(precision, Q, kt, tuning):
    """4.  The smallest batches with 256 workgroups (16, 12 and 8 waves): k_cfconv_quad with the host's quad_wg_ptr and with ranges
    written as data -- empty ranges at the start, in the middle and at the end, a one-quad range, a range of 5 waves + 1 quads dealt
    over several rounds whose first and last quad have no tile (have_pf, ntiles == 0) --, and k_cfconv_node, which walks equal
    shares (a wave takes two quads, the last workgroup one).  One float64 reference per batch."""
    b = _bench(precision, "q%d" % Q)
    waves = CR.launch(Q, kt, tuning)["waves"]
    host = b.tv["wg_ptr"]
    assert host is not None and host.shape[0] == 257 and host[-1] == Q
    got = b.run(kt, 0, 0, tuning)
    assert b.shape["ranges"] and (b.shape["grid"], b.shape["waves"], b.shape["last"]) == (256, waves, 1)
    b.check("host ranges", got, kt, 0, 0)
    w = _written_ranges(Q, waves)
    ntiles = np.diff(b.tv["lt_ptr"]) + b.tb["nR"]
    assert ntiles[3] == 0 and ntiles[3 + 5 * waves] == 0 and ntiles[4] > 0 and (ntiles[3:3 + 5 * waves] == 0).sum() >= waves
    keep = b.topo.quad_wg_ptr.clone()
    try:
        b.topo.quad_wg_ptr.copy_(t(w.astype(np.int32)).cuda())
        got2 = b.run(kt, 0, 0, tuning)
    finally:
        b.topo.quad_wg_ptr.copy_(keep)
    b.check("written ranges", got2, kt, 0, 0)
    assert np.array_equal(got.view(np.int32), got2.view(np.int32))          # (a quad's result does not depend on its workgroup)
    b.check("equal shares", b.run(kt, 0, 0, dict(tuning, **NODE)), kt, 0, 0)
    assert not b.shape["ranges"]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_equal_shares_on_256_workgroups_leave_some_empty(precision):
    """4, without ranges.  3,073 quads in 12-wave workgroups: 13 quads each, workgroup 236 takes five and the last nineteen none
    (their first quad lies past the end) -- k_cfconv_node, which never takes ranges, and k_cfconv_quad on a topology without
    quad_wg_ptr, which deals 13 quads to 12 waves."""
    b = _bench(precision, "q3073")
    for tn, ranges in ((dict(TWELVE, **NODE), True), (TWELVE, False)):
        got = b.run(1, 0, 0, tn, ranges=ranges)
        assert (b.shape["grid"], b.shape["per_wg"], b.shape["last"], b.shape["ranges"]) == (256, 13, -242, False)
        b.check("equal shares", got, 1, 0, 0)


# ------------------------------------------------------------------------------------------------- 5. independence
@pytest.mark.parametrize("kernel", ["quad", "node"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rows_of_a_target_depend_on_its_own_molecule_only(precision, kernel):
    """5.  xs, the lengths and the scales of ONE molecule changed (a 34-atom one, whose quads sit between other molecules'): its own
    rows change, every other molecule's rows keep their bits."""
    b = _bench(precision, "rows")
    tn = NODE if kernel == "node" else {}
    base = b.run(2, 0, 2, tn).view(np.int32)
    gp = b.tv["graph_ptr"]
    g = int(np.nonzero(np.diff(gp) == 34)[0][0])
    lo, hi = int(gp[g]), int(gp[g + 1])
    ws, N = b.ws, b.N
    lrows = torch.from_numpy(np.nonzero((b.tv["mol"][b.tv["lt_src"]] == g))[0]).cuda()
    saved = [x.clone() for x in (ws.xs, ws.rad_len, ws.r_scale, ws.lt_len, ws.lt_scale)]
    try:
        ws.xs.view(N, 192)[lo:hi] *= -1.5
        ws.rad_len.view(N, CR.RS)[lo:hi] *= 0.75
        ws.r_scale.view(2 * CR.MAX_CONVS, N, CR.RS)[:, lo:hi] *= 0.5
        ws.lt_len[lrows] *= 0.75
        ws.lt_scale.view(2 * CR.MAX_CONVS, -1)[:, lrows] *= 0.5
        b.before = [x.clone() for x in b.inputs]
        got = b.run(2, 0, 2, tn).view(np.int32)
    finally:
        for x, s in zip((ws.xs, ws.rad_len, ws.r_scale, ws.lt_len, ws.lt_scale), saved):
            x.copy_(s)
        b.before = [x.clone() for x in b.inputs]
    other = np.ones(N, dtype=bool)
    other[lo:hi] = False
    assert np.array_equal(base[other], got[other])
    changed = (base[lo:hi] != got[lo:hi]).any(axis=1)
    live = (b.tb["rad_cnt"][lo:hi] > 0) | (np.bincount(b.tb["lt_tgt"][b.tb["lt_live"]], minlength=N)[lo:hi] > 0)
    assert np.array_equal(changed, live)
    assert np.array_equal(b.run(2, 0, 2, tn).view(np.int32), base)
