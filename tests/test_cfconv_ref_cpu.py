"""CPU: tests/cfconv_ref.py (the float64 restatement tests/test_hip_cfconv_kernels.py compares k_cfconv_quad and k_cfconv_node with)
anchored against the network itself in float64; its features against packing.poly_features; its drawn inputs shown to be well
conditioned (plain float32 in the kernels' row order stays within a quarter of the "f32" gates) and its comparison shown to be
sensitive (every wrong kernel listed below moves the aggregate past ten times the loosest gate); the one-pass weights of the
plan 1..3 coefficient sets; the launch shapes against a table of hand-worked cases."""
import functools
import math

import numpy as np
import pytest
import torch

import cfconv_ref as CR
import node_ref as NR
from helpers import TOL_ELEM, TOL_NORM, elem_err, rel_err
from test_hip_kernels import _agg_ref

TEN_GATES = 10 * max(TOL_NORM.values())          # 3e-4
CUTOFF = 10.0


@functools.lru_cache(maxsize=None)
def _rows(name, gt=4):
    tv = CR.view(CR.topology(name, gt))
    return tv, CR.tables(tv, name, CUTOFF, slotted=CR.SLOTTED if name == "types" else None)


def _slots(name):
    tv, _ = _rows(name)
    types = [ty for ty in np.unique(tv["lt_type"]) if name != "types" or ty in CR.SLOTTED]
    table = np.full(100, -1, dtype=np.int64)
    table[types] = np.arange(len(types))
    return table, len(types)


@functools.lru_cache(maxsize=64)
def _reference(name, kt, plan, mode, k):
    table, ns = _slots(name)
    rad, typed, S = CR.coefficient_sets(name, kt, plan, mode, ns, k)
    return CR.cfconv(rad, typed, table, _rows(name), _rows(name)[1]["xs"], CUTOFF, k)


def _sets(name, kt, plan, mode, k):
    table, ns = _slots(name)
    return CR.coefficient_sets(name, kt, plan, mode, ns, k) + (table, ns)


# ------------------------------------------------------------------------------------------------- the network
def test_reference_equals_the_network_in_float64():
    """The fitted 32-term coefficients (packing.fit_type on node_ref.state_dict: radius set and one set per local type) through
    cfconv_ref.cfconv against the network itself -- MLPEdgeEncoder, nn.0, ssp, nn.2, times lw C: test_hip_kernels._agg_ref -- in
    float64 on the hub batch with positions: radius rows = the pairs of a molecule inside the cutoff that are no local edge (at
    most 33 per target, sources ascending), lengths from the positions, lw C from the same float64 evaluation."""
    from agdiff_amd import drugs_model_config, packing
    cfg = drugs_model_config()
    sd = NR.state_dict(cfg)
    sd64 = NR.to64(sd)
    topo = CR.topology("hub")
    tv = CR.view(topo)
    N = tv["N"]
    rng = np.random.default_rng(5)
    pos = rng.standard_normal((N, 3)) * 3.0
    src_l, dst_l, typ_l = (x.numpy().astype(np.int64) for x in (topo.loc_src, topo.loc_dst, topo.loc_type))
    is_local = np.zeros((N, N), dtype=bool)
    is_local[src_l, dst_l] = True
    dist = np.sqrt(((pos[:, None] - pos[None]) ** 2).sum(-1))
    cnt = np.zeros(N, dtype=np.int64)
    rsrc = np.tile(np.arange(N)[:, None], (1, CR.RS))
    rlen = np.ones((N, CR.RS))
    es, ed = [], []
    for i in range(N):
        js = [j for j in range(tv["graph_ptr"][tv["mol"][i]], tv["graph_ptr"][tv["mol"][i] + 1])
              if j != i and dist[j, i] < cfg.cutoff and not is_local[j, i]][:CR.CAP]
        cnt[i] = len(js)
        rsrc[i, :len(js)] = js
        rlen[i, :len(js)] = dist[js, i]
        es += js
        ed += [i] * len(js)
    assert cnt.max() >= 17 and cnt.min() == 0
    src = np.concatenate([src_l, np.asarray(es, dtype=np.int64)])
    dst = np.concatenate([dst_l, np.asarray(ed, dtype=np.int64)])
    typ = np.concatenate([typ_l, np.zeros(len(es), dtype=np.int64)])
    d = dist[src, dst]
    attr = np.zeros((src.shape[0], 128))
    for ty in np.unique(typ):
        attr[typ == ty] = packing._edge_attr_fn(sd, "edge_encoder_global", int(ty))(d[typ == ty]).numpy()
    g = dict(edge_index=np.stack([src, dst]), edge_length=d, edge_attr=attr)

    def lw_c(k, c, dd):                          # schnet.py:140-146 in float64
        p = "encoder_global.interactions.%d.conv%d.distance_weighting" % (k, c)
        x = torch.from_numpy(np.ascontiguousarray(dd, dtype=np.float64)).view(-1, 1)
        lw = torch.sigmoid(torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(x, sd64[p + ".layer1.weight"], sd64[p + ".layer1.bias"])),
                                                      sd64[p + ".layer2.weight"], sd64[p + ".layer2.bias"])).view(-1).numpy()
        assert cfg.smooth_conv
        dd = np.asarray(dd, dtype=np.float64)
        return lw.reshape(dd.shape) * 0.5 * (np.cos(dd * math.pi / cfg.cutoff) + 1.0) * (dd <= cfg.cutoff)
    eid = topo.lt_eid
    real = tv["lt_real"]
    llen = np.where(real, dist[src_l[np.maximum(eid, 0)], dst_l[np.maximum(eid, 0)]], 1.0)
    RT = 16 // tv["GT"]
    trow = np.arange(16 * tv["T"])
    lt_tgt = tv["quad_tgt"][np.repeat(np.arange(tv["Q"]), np.diff(tv["lt_ptr"]))[trow // 16], (trow % 16) // RT]
    assert np.array_equal(lt_tgt[real], dst_l[eid[real]]) and np.array_equal(tv["lt_src"][real], src_l[eid[real]])
    types = [int(x) for x in np.unique(typ_l)]
    table = np.full(100, -1, dtype=np.int64)
    table[types] = np.arange(len(types))
    order = packing.poly_feature_order(1)
    h = torch.from_numpy(NR.draw("h:net", (N, 128))).double()
    for k in (0, 3):
        tb = dict(rad_cnt=cnt, rad_src=rsrc, rad_len=rlen, lt_len=llen, lt_tgt=lt_tgt, lt_live=real,
                  r_raw=np.stack([lw_c(kk // 2, 1 + kk % 2, rlen) for kk in range(2 * cfg.num_convs)]),
                  l_raw=np.stack([lw_c(kk // 2, 1 + kk % 2, llen) for kk in range(2 * cfg.num_convs)]))

        def term_order(mats):
            C = np.empty((192, 32))
            C[:, order] = mats["conv%d.filt_poly_pk" % k]
            return C
        mats, err = packing.fit_type(sd, cfg, 0, 1, True)
        assert err < 1e-12
        typed = np.stack([term_order(packing.fit_type(sd, cfg, ty, 1, False)[0]) for ty in types])
        xs = NR.prep(sd64, k, h)
        got = CR.cfconv(term_order(mats), typed, table, (tv, tb), xs.numpy(), cfg.cutoff, k)
        want = _agg_ref(sd64, cfg, "encoder_global.interactions.%d" % k, g, xs).numpy()
        assert rel_err(got, want) < 1e-9, k


@pytest.mark.parametrize("K", [32, 64, 96, 128])
def test_features_equal_packing_poly_features(K):
    """phi from cos(n arccos x) against the recurrences of packing.poly_features (what fit_poly fits with); the packed column
    order is packing.poly_feature_order, applied by cfconv_ref.natural_columns alone."""
    from agdiff_amd import packing
    x = np.concatenate([np.linspace(-1.0, 1.0, 2049), [-1.0, 1.0, 0.0]])
    assert np.abs(CR.phi(x, K) - packing.poly_features(x, K)).max() < 1e-13
    assert np.abs(CR.phi32(x, K) - CR.phi(x.astype(np.float32), K)).max() < 2e-4
    C = np.arange(192 * K, dtype=np.float64).reshape(192, K)
    nat = CR.natural_columns(C, K // 32)
    back = np.empty_like(C)
    back[:, packing.poly_feature_order(K // 32)] = nat
    assert np.array_equal(back, C)
    # lengths: 0 -> x = -1, rc -> 1, beyond -> clamped
    assert CR.length_x([0.0, CUTOFF, 1.5 * CUTOFF, 1e30], CUTOFF).tolist() == [-1.0, 1.0, 1.0, 1.0]


# ------------------------------------------------------------------------------------------------- the drawn inputs
def test_tables_keep_the_hosts_invariants_and_reach_the_edges():
    """What tests/test_hip_cfconv_kernels.py relies on: valid sources everywhere, scale 0 / NaN / decoys by row class, the arranged
    quads, every count of CNT_CHOICES, quad tails with one, two and three missing targets, quads without any tile."""
    for name, gt in (("rows", 4), ("rows", 2), ("rows", 1), ("hub", 4), ("types", 4), ("q97", 4)):
        tv, tb = _rows(name, gt)
        N, qt, cnt = tv["N"], tv["quad_tgt"], tb["rad_cnt"]
        tile_mol = tv["mol"][qt[np.repeat(np.arange(tv["Q"]), np.diff(tv["lt_ptr"])), 0]]
        assert np.all(tv["mol"][tb["rad_src"]] == tv["mol"][:, None]) and np.all(tv["mol"][tv["lt_src"]] == tile_mol.repeat(16))
        assert np.all(qt[:, 0] >= 0)
        r = np.arange(CR.RS)[None, :]
        live, r16 = r < cnt[:, None], ((cnt + 15) // 16 * 16)[:, None]
        s, ln = tb["r_scale"], tb["rad_len"]
        assert np.isfinite(s[:, live]).all() and np.all(s[:, (~live) & (r < r16)] == 0) and np.isnan(s[:, r >= r16]).all()
        assert np.isfinite(ln[r < np.maximum(r16, tb["walked"][:, None])]).all() and np.isnan(ln[r >= np.maximum(r16, tb["walked"][:, None])]).all()
        assert np.all(tb["lt_scale"][:, ~tv["lt_real"] & ~np.isnan(tb["lt_scale"][0])] == 0)
        assert np.array_equal(s[:, live], tb["r_raw"][:, live]) and np.array_equal(tb["lt_scale"][:, tb["lt_live"]], tb["l_raw"][:, tb["lt_live"]])
        assert len({tb["r_raw"][p].tobytes() for p in range(12)}) == 12 and len({tb["l_raw"][p].tobytes() for p in range(12)}) == 12
    tv, tb = _rows("rows")
    qt, cnt = tv["quad_tgt"], tb["rad_cnt"]
    assert set(cnt.tolist()) >= set(CR.CNT_CHOICES)
    per_quad = {tuple(np.where(q >= 0, cnt[np.maximum(q, 0)], -1).tolist()) for q in qt}
    assert set(CR.QUAD_PATTERNS) <= per_quad
    assert {int((q < 0).sum()) for q in qt} == {0, 1, 2, 3}
    ntiles = np.diff(tv["lt_ptr"]) + tb["nR"]
    assert (ntiles == 0).sum() >= 3 and ((np.diff(tv["lt_ptr"]) == 0) & (tb["nR"] > 0)).any()
    ln, live = tb["rad_len"], np.arange(CR.RS)[None, :] < cnt[:, None]
    assert (ln[live] == 0).any() and (ln[live] == np.float32(CUTOFF)).any() and (ln[live] > CUTOFF).any()
    decoys = ln[(np.arange(CR.RS)[None, :] >= ((cnt + 15) // 16 * 16)[:, None]) & np.isfinite(ln)]
    assert decoys.size and set(np.unique(decoys).tolist()) == {0.0, np.float32(3.0), 20.0, float(np.float32(1e30))}
    tv, tb = _rows("hub")
    assert np.diff(tv["lt_ptr"]).max() >= 8                       # the 52-edge centre: several tiles of one type in a quad
    tv, tb = _rows("types")
    assert len(np.unique(tv["lt_type"])) == 8 and np.isnan(tb["lt_scale"][:, tv["lt_type"] == CR.UNSLOTTED]).all()
    tv, tb = _rows("q97")
    assert tv["Q"] == 97 and np.array_equal(tv["mol"][tv["quad_tgt"][:, 0]], np.arange(97))


CASES32 = [(n, kt, plan, k) for n in ("rows", "hub", "types") for kt, plan in CR.KT_PLANS for k in ((0, 2, 5) if (kt, plan) == (4, 0) else (2,))] + \
    [("q97", 1, 0, 0), ("q2041", 4, 0, 5)]


@pytest.mark.parametrize("name,kt,plan,k", CASES32)
def test_plain_float32_stays_within_a_quarter_of_the_f32_gates(name, kt, plan, k):
    """The same sums in plain float32 (features by recurrence, rows in the kernels' order) against the float64 reference, on the
    drawn inputs: the inputs themselves support the gates."""
    for mode in ((0,) if plan == 0 else (1, 2)):
        rad, typed, S, table, ns = _sets(name, kt, plan, mode, k)
        ref = _reference(name, kt, plan, mode, k)
        got = CR.cfconv(rad, typed, table, _rows(name), _rows(name)[1]["xs"], CUTOFF, k, dtype=np.float32)
        assert np.isfinite(ref).all() and np.abs(ref).max() > 1.0
        rn, re_ = rel_err(got, ref), elem_err(got, ref)
        print("float32 %s kt %d plan %d mode %d k %d: normwise %.2e element-wise %.2e" % (name, kt, plan, mode, k, rn, re_))
        assert rn < TOL_NORM["f32"] / 4 and re_ < TOL_ELEM["f32"] / 4


# ------------------------------------------------------------------------------------------------- one-pass weights
@pytest.mark.parametrize("kt,plan", [kp for kp in CR.KT_PLANS if kp[1]])
@pytest.mark.parametrize("mode", [1, 2])
def test_one_pass_terms_weigh_a_quarter_gate_and_a_lost_k_tile_ten_gates(mode, kt, plan):
    """Plans 1..3: POLY_EPS1[mode] x packing.poly_high_weight of every set is a quarter of the mode's normwise gate (about 3.4e-3
    f16x3, 9.6e-4 bf16x3), and the aggregate with the TOP k-tile of the radius set lost still sits past ten times that gate."""
    from agdiff_amd import packing
    prec = {1: "bf16x3", 2: "f16x3"}[mode]
    rad, typed, S, table, ns = _sets("rows", kt, plan, mode, 2)
    hi = CR.one_pass_from(kt, plan)
    for C in [rad] + list(typed):
        hw = packing.poly_high_weight(CR.natural_columns(C, kt), kt, hi)
        assert abs(packing.POLY_EPS1[mode] * hw / (TOL_NORM[prec] / 4) - 1.0) < 1e-3
    assert abs(CR.high_weight(mode) - {1: 9.6e-4, 2: 3.41e-3}[mode]) < 1e-5
    if kt >= 2:
        lost = rad.copy()
        lost[:, 32 * (kt - 1):] = 0.0
        ref = _reference("rows", kt, plan, mode, 2)
        err = rel_err(CR.cfconv(lost, typed, table, _rows("rows"), _rows("rows")[1]["xs"], CUTOFF, 2), ref)
        print("top k-tile lost, kt %d plan %d %s: %.2e" % (kt, plan, prec, err))
        assert err > 10 * TOL_NORM[prec]


# ------------------------------------------------------------------------------------------------- mutations
def _mut(name, kt, plan, k, mutate=None, coefs=None):
    rad, typed, S, table, ns = _sets(name, kt, plan, 0, k)
    if coefs:
        rad, typed = coefs(rad.copy(), typed.copy())
    got = CR.cfconv(rad, typed, table, _rows(name), _rows(name)[1]["xs"], CUTOFF, k, mutate=mutate or {})
    return rel_err(got, _reference(name, kt, plan, 0, k))


def _zero_top(kt):
    def f(rad, typed):
        rad[:, 32 * (kt - 1):] = 0.0
        typed[:, :, 32 * (kt - 1):] = 0.0
        return rad, typed
    return f


def _swap_tiles(a, b):
    def f(rad, typed):
        for C in (rad, typed):
            C[..., 32 * a:32 * a + 32], C[..., 32 * b:32 * b + 32] = C[..., 32 * b:32 * b + 32].copy(), C[..., 32 * a:32 * a + 32].copy()
        return rad, typed
    return f


def _target(tb, pred):
    i = np.nonzero(pred(tb["rad_cnt"]))[0]
    assert i.size
    return int(i[0])


def _mutations():
    tv, tb = _rows("rows")
    tvt, tbt = _rows("types")
    cnt = tb["rad_cnt"]
    pad = np.nonzero(~tv["lt_real"] & (tb["lt_tgt"] >= 0))[0]
    tile = int(np.nonzero(tb["lt_live"])[0][0] // 16)
    quad4 = int(np.nonzero((tv["quad_tgt"] >= 0).all(axis=1) & (cnt[np.maximum(tv["quad_tgt"], 0)] > 0).all(axis=1))[0][0])
    wg = CR.launch(tv["Q"], 1)
    out = [("top k-tile zeroed, rung %d" % kt, "rows", kt, {}, _zero_top(kt)) for kt in (2, 3, 4)]
    out += [("k-tiles 1 and 3 swapped", "rows", 4, {}, _swap_tiles(1, 3)), ("k-tiles 0 and 1 swapped", "rows", 2, {}, _swap_tiles(0, 1)),
            ("T_8g one step short for g >= 8", "rows", 3, {"T8g_short": 8}, None),
            ("T_8g one step short for g >= 8 (rung 4)", "rows", 4, {"T8g_short": 8}, None),
            ("conv1 and conv2 scales swapped", "rows", 1, {"conv_scales_swapped": 1}, None),
            ("block k + 1's scale plane", "rows", 1, {"next_block_scale": 1}, None),
            ("last radius row dropped", "rows", 1, {"radius_last_dropped": _target(tb, lambda c: c == 17)}, None),
            ("row cnt counted", "rows", 1, {"radius_cnt_counted": _target(tb, lambda c: c == 15)}, None),
            ("the 33rd row dropped", "rows", 1, {"row33_dropped": _target(tb, lambda c: c == CR.CAP)}, None),
            ("a local tile with the neighbouring slot's set", "rows", 1, {"neighbour_slot": (tile, _slots("rows")[1])}, None),
            ("an unslotted type's rows counted", "types", 1, {"unslotted_counted": 1}, None),
            ("a pad local row counted", "rows", 1, {"pad_local_counted": int(pad[0])}, None),
            ("first quad of a workgroup range skipped", "rows", 1, {"quads_skipped": [wg["per_wg"] * 3]}, None),
            ("fourth target given the third's sums", "rows", 1, {"fourth_gets_third": quad4}, None),
            ("unscale omitted", "rows", 1, {"no_unscale": 7}, None)]
    return out


@pytest.mark.parametrize("index", range(18))
def test_every_wrong_kernel_sits_past_ten_times_the_loosest_gate(index):
    """Each entry of _mutations() is one way a kernel can be wrong; the comparison of tests/test_hip_cfconv_kernels.py must see
    it: normwise past 3e-4 on the drawn inputs (plan-0 sets, block 2)."""
    muts = _mutations()
    assert len(muts) == 18
    what, name, kt, mutate, coefs = muts[index]
    err = _mut(name, kt, 0, 2, mutate, coefs)
    print("%-48s %.2e" % (what, err))
    assert err > TEN_GATES, what


# ------------------------------------------------------------------------------------------------- launch shapes
FOUR = {"cfconv_four_min_quads": 1}
TWELVE = {"cfconv_four_min_quads": -1}
# (Q, kt, tuning) -> (waves, grid, quads per workgroup, quads of the last workgroup, XCD remap, ranges), worked by hand from
# launch_cfconv_node_s and the kernels' first lines
HAND = [(1, 1, None, (12, 1, 1, 1, False, False)), (12, 1, None, (12, 1, 12, 12, False, False)), (84, 1, None, (12, 7, 12, 12, False, False)),
        (96, 1, None, (12, 8, 12, 12, True, False)), (97, 1, None, (12, 9, 11, 9, False, False)), (192, 1, None, (12, 16, 12, 12, True, False)),
        (3060, 1, None, (12, 255, 12, 12, False, False)), (3061, 1, None, (12, 256, 12, 1, True, True)),
        (4080, 1, FOUR, (16, 255, 16, 16, False, False)), (4081, 1, FOUR, (16, 256, 16, 1, True, True)),
        (4081, 1, TWELVE, (12, 256, 16, 1, True, True)), (8192, 1, None, (16, 256, 32, 32, True, True)),
        (97, 1, FOUR, (16, 7, 14, 13, False, False)), (97, 2, FOUR, (12, 9, 11, 9, False, False)),
        (2040, 4, None, (8, 255, 8, 8, False, False)), (2041, 4, None, (8, 256, 8, 1, True, True)), (2041, 3, FOUR, (8, 256, 8, 1, True, True)),
        (3073, 1, TWELVE, (12, 256, 13, -242, True, True))]


@pytest.mark.parametrize("Q,kt,tuning,want", HAND)
def test_launch_shapes_against_hand_worked_cases(Q, kt, tuning, want):
    s = CR.launch(Q, kt, tuning)
    assert (s["waves"], s["grid"], s["per_wg"], s["last"], s["remap"], s["ranges"]) == want
    assert s["kernel"] == "quad" and s["four"] == (s["waves"] == 16)
    n = CR.launch(Q, kt, dict(tuning or {}, cfconv_quad_tiles=-1))
    assert n["kernel"] == "node" and not n["ranges"] and (n["waves"], n["grid"]) == want[:2]
    assert CR.launch(Q, kt, tuning, group_targets=2)["kernel"] == "node"


def test_launch_lds_sets_and_variant_words():
    """Typed sets in LDS next to the radius set: 5 of 24 KiB at one k-tile, 2, 1 and 0 at two, three and four; poly_lds_sets = 1
    sends every typed set to L2.  Below 256 workgroups no workgroup is ever empty: grid = ceil(Q / W) gives (grid - 1) W < Q,
    and per_wg <= W."""
    D = CR._lib.DEFINES
    assert [CR.launch(600, kt, None, num_slots=7)["lds_slots"] for kt in (1, 2, 3, 4)] == [5, 2, 1, 0]
    assert [CR.launch(600, kt, {"poly_lds_sets": 1}, num_slots=7)["lds_slots"] for kt in (1, 2, 3, 4)] == [0, 0, 0, 0]
    assert CR.launch(600, 1, None, num_slots=5)["bits"] == D["AGDIFF_VAR_CFCONV_NODE"] | D["AGDIFF_VAR_CFCONV_NODE_LOCAL"] | D["AGDIFF_VAR_CFCONV_NODE_QUAD"]
    assert CR.launch(600, 1, FOUR, num_slots=7)["bits"] & (D["AGDIFF_VAR_POLY_L2_SETS"] | D["AGDIFF_VAR_CFCONV_NODE_FOUR"]) == \
        D["AGDIFF_VAR_POLY_L2_SETS"] | D["AGDIFF_VAR_CFCONV_NODE_FOUR"]
    for Q in range(1, 4200):
        for kt, tn in ((1, None), (1, FOUR), (4, None)):
            s = CR.launch(Q, kt, tn)
            assert s["grid"] == 256 or (s["last"] >= 1 and s["per_wg"] <= s["waves"])
    assert sorted(CR.workgroup_of_block(b, 16) for b in range(16)) == list(range(16))
    assert [CR.workgroup_of_block(b, 16) for b in (0, 1, 8, 9)] == [0, 2, 1, 3] and CR.workgroup_of_block(5, 9) == 5
