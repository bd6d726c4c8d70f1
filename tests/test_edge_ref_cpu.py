"""CPU: tests/edge_ref.py (the float64 restatement tests/test_hip_edge_kernels.py compares the per-edge producers of csrc/edge.hip
with) anchored: the segment tables and the union table packing builds from the twelve written networks ARE those networks; a
plain float32 evaluation of the float32 tables stays within a quarter of the "f32" gates (the inputs are well conditioned); every
wrong kernel listed in edge_ref moves some result past ten times the loosest gate (the comparison is sensitive); float32 torch runs
of both encoders meet the gates of all three modes against float64 on every case; and the design facts the GPU tests rest on.
Prints the figures the GPU module's absolute bound cites."""
import numpy as np
import pytest
import torch

import edge_ref as R
from helpers import TOL_ELEM, TOL_NORM, elem_err, rel_err

TEN_GATES = 10 * max(TOL_NORM.values())          # 3e-4
SETS = ("wide", "narrow")


@pytest.fixture(scope="module")
def world():
    w = {}
    for which in SETS:
        nets = R.networks(which)
        t64, t32 = R.segment_tables(nets)
        w[which] = dict(nets=nets, t64=t64, t32=t32, union=R.union_table(nets), d=R.lengths(which), mid=R.mid_segment_lengths(which))
    return w


def _inside(d):
    return (d >= 0) & (d <= R.RC32)


# ------------------------------------------------------------------------------------------------- the design
def test_planes_hold_the_kink_patterns_they_are_named_for(world):
    for which in SETS:
        t32 = world[which]["t32"]
        kinks = [t32[p, :32][np.isfinite(t32[p, :32])] for p in range(R.NPLANES)]
        inside = [int(((k > 0) & (k < R.RC32)).sum()) for k in kinks]
        assert kinks[0].size == 0 and np.all(world[which]["nets"][0][0] == 0)
        assert kinks[1].size == 32 and inside[1] == 32
        assert kinks[2].size == 32 and inside[2] == 31 and (kinks[2] > R.RC32).sum() == 1
        assert kinks[3].size == 32 and np.all(kinks[3] < 0)
        assert kinks[4].size == 32 and np.all(kinks[4] > R.RC32)
        assert kinks[5].size == 32 and np.unique(kinks[5]).size == 30
        assert np.intersect1d(kinks[6], kinks[1]).size >= 2
        assert np.float32(0.0) in kinks[7] and R.RC32 in kinks[7]
        for p in (9, 10, 11):
            assert inside[p] == 32
        # every kink is the float32 value that was written: -b1 / w1 is exact
        for p in range(1, R.NPLANES):
            assert np.array_equal(np.sort(R.plane_kinks(p, which == "wide")), kinks[p])
    tab, K, S = world["wide"]["union"]
    assert K == 512 and S <= K
    tab, K, S = world["narrow"]["union"]
    assert K <= 64 and S > 32


def test_pre_activations_stay_where_the_sigmoid_has_a_slope(world):
    """every plane but the tail plane: |pre-activation| < 4 on at least half the lengths in [0, rc] (a saturated sigmoid hides a
    wrong line); the tail plane passes +30 and, on the other side, the clamp of ag_sigmoid (-87.3); slopes change by 0.5 .. 0.875 at the first kink of the zigzag planes and by 1 .. 1.75 at every later one"""
    for which in SETS:
        w = world[which]
        d = w["d"][_inside(w["d"])]
        for p in range(R.NPLANES):
            f = R.preact64(w["nets"][p], d)
            if p == R.TAIL_PLANE:
                assert f.max() > 30.0 and f.min() < -126.0 / 1.4426950408889634       # (the kernel's fminf(-x log2 e, 126) engages)
            else:
                assert (np.abs(f) < 4.0).mean() >= 0.5, (which, p)
        for p in (1, 2, 9, 10, 11):
            a = w["t64"][p, 32:65]
            assert np.abs(np.diff(a))[0] >= 0.5 and np.abs(np.diff(a))[1:].min() >= 1.0, (which, p)


def test_lengths_hold_every_kink_its_neighbours_and_the_cutoff(world):
    for which in SETS:
        d = world[which]["d"]
        assert d.dtype == np.float32 and not np.isnan(d).any()
        for k in R.all_kinks(which):
            for v in (k, np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-np.inf))):
                assert v in d
        signs = np.signbit(d[d == 0])
        assert signs.tolist() == [True, False]
        for v in (R.RC32, np.nextafter(R.RC32, np.float32(np.inf)), np.nextafter(R.RC32, np.float32(0)), np.float32(15.0), np.float32(1000.0),
                  np.float32(1e-3)):
            assert v in d
        assert world[which]["mid"].size > (100 if which == "wide" else 40)


# ------------------------------------------------------------------------------------------------- tables = networks
@pytest.mark.parametrize("smooth", [0, 1])
def test_tables_and_union_equal_the_networks_in_float64(world, smooth):
    """packing.dist_segments with s = number of kinks <= d, and packing.dist_union_table with u = number of union kinks <= d (for
    lengths in [0, rc]: beyond it the envelope is 0 and the union table promises nothing), against the network at every length"""
    for which in SETS:
        w = world[which]
        d = np.concatenate([w["d"], w["mid"]])
        ref = R.scales64(w["nets"], d, R.RC, smooth)
        got = R.table_scales(w["t64"], d, R.RC, smooth)
        assert np.abs(got - ref).max() < 1e-13
        tab, K, S = w["union"]
        un = R.union_scales(tab, K, R.NPLANES, d, R.RC, smooth)
        # (the union table holds the float32 tables' lines: compare with those, in float64)
        t32 = R.table_scales(w["t32"].astype(np.float64), d, R.RC, smooth)
        ins = _inside(d)
        assert np.abs(un[:, ins] - t32[:, ins]).max() < 1e-15
        assert np.all(un[:, ~ins] == 0.0) and np.all(ref[:, ~ins] == 0.0)


@pytest.mark.parametrize("smooth", [0, 1])
def test_plain_float32_meets_a_quarter_of_the_f32_gates(world, smooth):
    """float32 tables, float32 lengths, one rounding each for the FMA, the sigmoid, the envelope and the product: per plane within
    a quarter of helpers.check_close's "f32" gates.  |beta| stays below 20 outside the tail plane (whose table is exact), or the
    FMA would lose digits to cancellation.  Prints the worst absolute error: the GPU tests' absolute bound is
    max(1e-6, 4 x this)."""
    for which in SETS:
        w = world[which]
        assert np.abs(np.delete(w["t64"][:, 65:98], R.TAIL_PLANE, axis=0)).max() < 20.0
        assert np.array_equal(w["t64"][R.TAIL_PLANE], w["t32"][R.TAIL_PLANE].astype(np.float64))
        d = w["d"]
        ref = R.scales64(w["nets"], d, R.RC, smooth)
        got = R.table_scales(w["t32"], d, R.RC, smooth, dtype=np.float32)
        rn = max(rel_err(got[p], ref[p]) for p in range(R.NPLANES))
        re_ = max(elem_err(got[p], ref[p]) for p in range(R.NPLANES))
        print("float32 restatement %-6s smooth %d: normwise %.2e element-wise %.2e absolute %.2e" % (which, smooth, rn, re_, np.abs(got - ref).max()))
        assert rn < TOL_NORM["f32"] / 4 and re_ < TOL_ELEM["f32"] / 4
        assert np.abs(got - ref).max() < 2.5e-7


# ------------------------------------------------------------------------------------------------- mutants
SCALE_MUTANTS = ["segment_low", "segment_high", "no_fixup", "alpha_beta_swapped", "conv_planes_swapped", "envelope_lt",
                 "smooth_for_gaussian"]


@pytest.mark.parametrize("mutant", SCALE_MUTANTS)
def test_every_wrong_scale_kernel_passes_ten_gates(world, mutant):
    """Each wrong kernel moves some plane's normwise figure past ten times the loosest gate.  A segment one too low or too high
    cannot show AT a kink -- the function is continuous there: the two lines meet --, so those two are judged at the mid-segment
    lengths; the others at the test lengths themselves.  "envelope_lt" shows only where C(rc) != 0: the Gaussian envelope (the smooth one is 0 at
    rc); "smooth_for_gaussian" is a mutant of the Gaussian mode."""
    for which in SETS:
        w = world[which]
        d = w["mid"] if mutant.startswith("segment") else w["d"]
        for smooth in ([0] if mutant in ("envelope_lt", "smooth_for_gaussian") else [0, 1]):
            ref = R.scales64(w["nets"], d, R.RC, smooth)
            got = R.table_scales(w["t64"], d, R.RC, smooth, mutate=(mutant,))
            worst = max(rel_err(got[p], ref[p]) for p in range(R.NPLANES))
            print("%-22s %-6s smooth %d: %.2e" % (mutant, which, smooth, worst))
            assert worst > TEN_GATES
    if mutant == "no_fixup":        # ... and it is the planes with 32 kinks <= d that see it: 1 and 3, not 2
        w = world["wide"]
        ref = R.scales64(w["nets"], w["d"], R.RC, 0)
        got = R.table_scales(w["t64"], w["d"], R.RC, 0, mutate=(mutant,))
        assert rel_err(got[1], ref[1]) > TEN_GATES and rel_err(got[3], ref[3]) > TEN_GATES and np.abs(got[2] - ref[2]).max() < 1e-13


def test_segment_mutants_are_invisible_exactly_at_a_kink(world):
    """... which is why they are judged mid-segment: at the kinks themselves the lower segment gives the same value to rounding"""
    w = world["wide"]
    k = R.all_kinks("wide")
    k = k[(k > 0) & (k < R.RC32)]
    ref = R.scales64(w["nets"], k, R.RC, 0)
    got = R.table_scales(w["t64"], k, R.RC, 0, mutate=("segment_low",))
    own = [np.isin(k, R.plane_kinks(p)) for p in (9, 10, 11)]
    assert max(np.abs(got[p][o] - ref[p][o]).max() for p, o in zip((9, 10, 11), own)) < 1e-12


def test_lost_pad_rows_and_lost_mirrors_show():
    cnt = np.asarray(R.RAD_COUNTS)
    RS = 48
    scales = np.full((R.NPLANES, cnt.size, RS), 0.5)
    ref, written = R.rad_expected(cnt, None, scales, RS)
    assert written.sum(axis=1).tolist() == [0, 16, 16, 16, 32, 32, 48]
    assert np.all(ref[:, 1, 1:16] == 0.0) and np.isnan(ref[:, 1, 16:]).all() and np.isnan(ref[:, 0]).all()
    bad, _ = R.rad_expected(cnt, None, scales, RS, mutate=("pad_rows_not_zeroed",))
    assert R.payload_error(bad, ref) > TEN_GATES
    n = 33
    pos, mir = R.scatter_indices(n)
    vals = np.arange(1.0, n + 1.0)[:, None] * np.ones((1, 4))
    ref, written = R.scatter_expected(vals, 2 * n, pos, mir)
    assert written.sum() == n + (mir >= 0).sum() and written[0]
    bad, _ = R.scatter_expected(vals, 2 * n, pos, mir, mutate=("mirror_not_written",))
    assert R.payload_error(bad, ref) > TEN_GATES
    assert R.payload_error(ref, ref) == 0.0


@pytest.mark.parametrize("n", [17, 33])
def test_row_index_case_has_missing_rows_and_a_shared_row(n):
    pos, mir = R.scatter_indices(n)
    ri, n_rows = R.row_index_case(n)
    assert ri.shape == (2 * n,) and ri.max() < n_rows
    named = np.concatenate([pos, mir[mir >= 0]])
    assert (ri[named] < 0).any()                                        # a named position without a row
    has = mir >= 0
    shared = has & (ri[pos] == ri[np.maximum(mir, 0)]) & (ri[pos] >= 0)
    assert shared.any()                                                  # a mirror pair with ONE row
    own = has & (ri[pos] != ri[np.maximum(mir, 0)]) & (ri[pos] >= 0) & (ri[np.maximum(mir, 0)] >= 0)
    assert own.any()                                                     # ... and pairs with two
    rows = ri[ri >= 0]
    # no row is handed to two different edges
    owner = {}
    for e in range(n):
        for p in [pos[e]] + ([mir[e]] if mir[e] >= 0 else []):
            if ri[p] >= 0:
                assert owner.setdefault(int(ri[p]), e) == e
    assert np.unique(rows).size < n_rows                                 # rows nothing names exist
    unnamed = np.setdiff1d(np.arange(2 * n), named)
    assert np.all(ri[unnamed] == -1)
    vals = np.arange(1.0, n + 1.0)[:, None] * np.ones((1, 4))
    ref, written = R.scatter_expected(vals, n_rows, pos, mir, row_index=ri)
    assert written.sum() == np.unique(rows).size


# ------------------------------------------------------------------------------------------------- encoders
@pytest.fixture(scope="module")
def weights():
    from agdiff_amd import qm9_model_config
    from oracle import agdiff_oracle as O
    sd = O.synth_state_dict_for(qm9_model_config(), head_scale=1.0)
    return {"synthetic": sd, "expanded": R.scaled_feature_expansion(sd),
            "gaussian": O.synth_state_dict_for(qm9_model_config(edge_encoder="gaussian"), head_scale=1.0)}


def test_encoder_cases_cover_types_tiles_and_both_gelu_tails(weights):
    assert R.E_ROUNDS > 16 * 256 * 16 and (R.E_ROUNDS + 15) // 16 == 4097
    ty = R.edge_types(R.E_ROUNDS)
    assert ty[0] == 0 and ty[1] == 99 and ty.min() >= 0 and ty.max() < 100
    for tile in range(0, 40):
        assert np.unique(ty[16 * tile:16 * tile + 16]).size >= 4
    d = R.edge_lengths(33)
    assert np.float32(1000.0) in d[:15] and np.float32(0.0) in d[:15]
    big = R.edge_lengths(R.E_ROUNDS)
    assert big.shape == (R.E_ROUNDS,) and np.all(np.isin(R.lengths("wide"), big))
    inside = big[_inside(big)]
    x = R.first_gelu_arguments(weights["synthetic"], inside)
    assert np.abs(x).max() < 6.0                                         # the plain weights never reach a tail inside the cutoff
    x = R.first_gelu_arguments(weights["expanded"], inside)
    assert x.max() > 6.0 and x.min() < -6.0


@pytest.mark.parametrize("name", ["synthetic", "expanded"])
def test_float32_torch_mlp_encoder_meets_every_gate(weights, name):
    """O.mlp_edge_encoder in float32 against float64 on every case: rows within 1.5 rc and the rows at 100 rc judged separately
    (edge_ref.near), as the GPU tests judge them"""
    sd = weights[name]
    for n in R.E_COUNTS + (R.E_ROUNDS,):
        d, ty = R.edge_lengths(n), R.edge_types(n)
        ref = R.mlp_encoder(sd, d, ty).numpy()
        got = R.mlp_encoder(sd, d, ty, dtype=torch.float32).numpy()
        for what, part in (("near", R.near(d)), ("far", ~R.near(d))):
            if part.any():
                rn, re_ = rel_err(got[part], ref[part]), elem_err(got[part], ref[part])
                print("float32 mlp encoder %-9s E=%-6d %-4s: normwise %.2e element-wise %.2e" % (name, n, what, rn, re_))
                assert rn < min(TOL_NORM.values()) and re_ < min(TOL_ELEM.values())
    d, ty = R.edge_lengths(33), R.edge_types(33)
    bad = R.mlp_encoder(sd, d, ty, mutate=("type0_tables",)).numpy()
    ref = R.mlp_encoder(sd, d, ty).numpy()
    assert rel_err(bad[R.near(d)], ref[R.near(d)]) > TEN_GATES


def test_float32_torch_gaussian_encoder_meets_every_gate(weights):
    sd = weights["gaussian"]
    for n in R.E_COUNTS + (16 * 13 + 5,):
        d, ty = R.gaussian_lengths(n), R.edge_types(n)
        ref = R.gaussian_encoder(sd, d, ty).numpy()
        got = R.gaussian_encoder(sd, d, ty, dtype=torch.float32).numpy()
        assert ref.shape == (n, 128)
        rn, re_ = rel_err(got, ref), elem_err(got, ref)
        print("float32 gaussian encoder E=%-4d: normwise %.2e element-wise %.2e" % (n, rn, re_))
        assert rn < min(TOL_NORM.values()) and re_ < min(TOL_ELEM.values())
    d = R.gaussian_lengths(64)
    ref = R.gaussian_encoder(sd, d, R.edge_types(64)).numpy()
    far = d >= np.float32(3.0 * R.RC)
    assert far.any() and np.all(ref[far, :64] < 1e-30)                   # every Gaussian underflows float32 there
    assert ref[0, 0] == 1.0                                              # d = 0 sits on the first offset


def test_flagged_case_masks():
    c = R.flagged_case()
    assert c["masks"].tolist() == [0, 0x0001, 0, 0x8000, 0, 0, (1 << 11) - 1]
    by_type = c["etype"] == R.UNSLOTTED_TYPE
    by_length = c["length"] > 10 * R.RC
    assert np.array_equal(c["hard"], by_type | by_length) and by_type[-11:].any() and by_length[-11:].any() and not (by_type & by_length).any()
    assert np.all(c["soft_length"] <= R.RC32) and np.all(np.isin(c["soft_type"], R.SLOTTED_TYPES))
    assert np.array_equal(c["soft_length"][~c["hard"]], c["length"][~c["hard"]]) and np.array_equal(c["soft_type"][~c["hard"]], c["etype"][~c["hard"]])


@pytest.mark.parametrize("which", SETS)
def test_producer_batch_puts_radius_lengths_on_the_kinks(which):
    b = R.producer_batch(which)
    k, pos = b["kinks"], b["pos"]
    assert pos.dtype == np.float32 and k.size + 1 == b["sizes"][0] <= 512 and np.unique(k).size == k.size
    x = pos[1:1 + k.size, 0]
    assert np.array_equal(np.sqrt(x * x), k)                              # float32 throughout: the length IS the kink
    assert k.size >= (256 if which == "wide" else 40)
    d = np.linalg.norm(pos[-40:, None, :].astype(np.float64) - pos[None, -40:, :], axis=-1)
    assert ((d < R.RC).sum(axis=1) - 1).min() >= 33                       # molecule D: every target beyond the cap
