"""CPU: tests/graph_ref.py -- the NumPy restatement of the graph build and the inputs tests/test_hip_graph_kernels.py feeds the
kernels -- checked without a GPU.  This file proves the INPUTS: that the reference is the oracle's graph, that a few answers
written by hand come out, and that every wrong rule a kernel could implement instead (graph_ref.RULES) gives another edge list on
the batch that is there to catch it.  A kernel that matches graph_ref bit for bit on these batches therefore implements the rule
and none of the alternates."""
import numpy as np
import pytest
import torch

import graph_ref as GR
from helpers import load_golden, rel_err, t
from large_mols import check_graph_properties

CAP = GR.CAP


def _oracle(b):
    from oracle import agdiff_oracle as O
    pos = t(b["pos"])
    ei, et = O.extend_graph_order_radius(pos.shape[0], pos, t(b["bond_index"]), t(b["bond_type"]), t(b["batch"]),
                                         cutoff=b["cutoff"], extend_order=False)
    return ei.numpy(), et.numpy(), O.get_distance(pos, ei).numpy()


def _against_oracle(b, ref):
    ei, et, elen = _oracle(b)
    perm = ref["ref2dst"]
    assert ref["num_edges"] == ei.shape[1]
    assert np.array_equal(np.sort(perm), np.arange(ref["num_edges"]))
    assert np.array_equal(np.stack([ref["e_src"][perm], ref["e_dst"][perm]]), ei)
    assert np.array_equal(ref["e_type"][perm], et)
    # (the oracle's norm() is not the definition of a length: graph_ref's own lengths are; 1e-6 is the existing tests' figure)
    assert rel_err(ref["e_len"][perm], elen) < 1e-6


@pytest.mark.parametrize("name", GR.BATCHES)
def test_reference_is_the_oracles_graph_on_every_batch(name):
    """Edge set, (src, dst) order and types exact against O.extend_graph_order_radius, lengths within 1e-6 of O.get_distance."""
    _against_oracle(GR.make_batch(name), GR.reference(name))


@pytest.mark.parametrize("case", ["g3_forward_qm9_small", "g3_forward_drugs_capped"])
def test_reference_is_the_oracles_graph_on_golden_fixtures(case):
    g = load_golden(case)
    b = dict(atom_type=g["atom_type"], bond_index=g["bond_index"], bond_type=g["bond_type"], batch=g["batch"],
             num_graphs=int(g["batch"].max()) + 1, pos=g["pos"], cutoff=10.0, extend_order=False)
    ref = GR.build(b)
    _against_oracle(b, ref)
    # ... and the reference project's own recorded graph (its radius_graph is torch_cluster's)
    perm = ref["ref2dst"]
    assert np.array_equal(np.stack([ref["e_src"][perm], ref["e_dst"][perm]]), g["edge_index"])
    assert np.array_equal(ref["e_type"][perm], g["edge_type"])


@pytest.mark.parametrize("name", ["max65", "lattice", "clusters", "max129", "graphs1025"])
def test_reference_has_the_properties_of_every_correct_build(name):
    """large_mols.check_graph_properties (CSR invariants, ref2dst, mirrors, the canonical partition) on the reference's own lists,
    the local list against BatchTopology's, and canon_radius_only: one entry per pair of mirror radius edges.  (Not on the shell
    batches: a d2 one ulp below r2 = 100 is an edge whose correctly rounded length IS 10.0f, which that check's "shorter than the
    cutoff" rightly calls out -- test_shell_batches_hold_exact_ties_and_an_inexact_r2 asserts that such edges are there.)"""
    from agdiff_amd.topology import BatchTopology
    b, ref = GR.make_batch(name), GR.reference(name)
    topo = BatchTopology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], b["num_graphs"], device="cpu")
    ls, ld, lt = ref["loc"]
    assert np.array_equal(ls, topo.loc_src.numpy()) and np.array_equal(ld, topo.loc_dst.numpy())
    assert np.array_equal(lt, topo.loc_type.numpy()) and np.array_equal(ref["loc_row"], topo.loc_row.numpy())
    assert ref["num_edges"] <= topo.max_edges and np.array_equal(ref["graph_ptr"], topo.graph_ptr.numpy())
    E = ref["num_edges"]
    c0, c1 = ref["canon"]
    w = dict(E=E, C=c0["num_canon"], **{k: ref[k] for k in ("e_src", "e_dst", "e_type", "e_len", "in_ptr", "out_ptr", "ref2dst")},
             **{k: c0[k] for k in ("c_pos", "c_mir", "c_src", "c_dst", "c_type", "c_len")})
    check_graph_properties(w, dict(batch=b["batch"], loc_src=ls, loc_dst=ld, loc_type=lt), b["pos"], b["cutoff"])
    ty, cp, cm = ref["e_type"], c1["c_pos"], c1["c_mir"]
    cover = np.bincount(np.concatenate([cp, cm[cm >= 0]]), minlength=E)
    assert np.array_equal(cover, (ty == 0).astype(cover.dtype))
    assert np.array_equal(ref["rad_cnt"], np.bincount(ref["e_dst"][ty == 0], minlength=b["batch"].shape[0]))
    rows = np.arange(GR.RS)[None, :] < ref["rad_cnt"][:, None]
    assert np.array_equal(ref["rad_src"][rows], ref["e_src"][ty == 0])
    assert np.array_equal(ref["rad_len"][rows].view(np.int32), ref["e_len"][ty == 0].view(np.int32))
    # the front's row form of the same list
    assert np.array_equal(ref["rad_src"].reshape(-1)[c1["row_pos"]], c1["c_src"])
    m = c1["row_mir"] >= 0
    assert np.array_equal(m, cm >= 0) and np.array_equal(ref["rad_src"].reshape(-1)[c1["row_mir"][m]], c1["c_dst"][m])
    assert np.array_equal(c1["row_pos"] // GR.RS, c1["c_dst"]) and np.array_equal(c1["row_mir"][m] // GR.RS, c1["c_src"][m])


def _bondless(pos, cutoff=10.0):
    pos = np.asarray(pos, dtype=np.float32)
    n = pos.shape[0]
    return dict(atom_type=np.full(n, 6, dtype=np.int64), bond_index=np.zeros((2, 0), dtype=np.int64), bond_type=np.zeros(0, dtype=np.int64),
                batch=np.zeros(n, dtype=np.int64), num_graphs=1, pos=pos, cutoff=cutoff, extend_order=False)


def test_three_atoms_on_a_line_with_one_exact_tie():
    """Atoms at x = 0, 10, 19, no bonds, cutoff 10: d2(0, 1) = 100 is a tie and no edge, d2(1, 2) = 81 is one, d2(0, 2) = 361 is
    none.  Written by hand."""
    ref = GR.build(_bondless([[0, 0, 0], [10, 0, 0], [19, 0, 0]]))
    assert ref["num_edges"] == 2
    assert ref["e_src"].tolist() == [2, 1] and ref["e_dst"].tolist() == [1, 2] and ref["e_type"].tolist() == [0, 0]
    assert ref["e_len"].tolist() == [9.0, 9.0] and ref["e_loc"].tolist() == [-1, -1]
    assert ref["in_ptr"].tolist() == [0, 0, 1, 2] and ref["out_ptr"].tolist() == [0, 0, 1, 2] and ref["ref2dst"].tolist() == [1, 0]
    assert ref["graph_edge_cnt"].tolist() == [2] and ref["graph_edge_ptr"].tolist() == [0, 2]
    for c in ref["canon"]:       # one canonical entry: 1 -> 2 (src < dst), its mirror 2 -> 1 at position 0
        assert (c["num_canon"], c["c_src"].tolist(), c["c_dst"].tolist(), c["c_pos"].tolist(), c["c_mir"].tolist()) == (1, [1], [2], [1], [0])
    assert ref["canon"][1]["row_pos"].tolist() == [2 * GR.RS] and ref["canon"][1]["row_mir"].tolist() == [1 * GR.RS]
    assert ref["rad_cnt"].tolist() == [0, 1, 1] and ref["rad_src"][1, 0] == 2 and ref["rad_src"][2, 0] == 1
    assert ref["n_within"].tolist() == [1, 2, 2]
    le = GR.build(_bondless([[0, 0, 0], [10, 0, 0], [19, 0, 0]]), rule="le")
    assert le["num_edges"] == 4 and le["e_len"].tolist() == [10.0, 10.0, 9.0, 9.0]


def test_thirty_five_atoms_all_in_range():
    """35 atoms inside one ball, no bonds: the candidates of every target are atoms 0..34, the first 33 are 0..32.  Targets 0..32
    keep the other 32 of those (self is the one dropped), targets 33 and 34 all 33.  Written by hand."""
    pos = np.random.default_rng(1).uniform(-2, 2, size=(35, 3))
    ref = GR.build(_bondless(pos))
    first = list(range(33))
    for i in range(35):
        lo, hi = ref["in_ptr"][i], ref["in_ptr"][i + 1]
        assert ref["e_src"][lo:hi].tolist() == [j for j in first if j != i]
        assert ref["rad_cnt"][i] == (32 if i < 33 else 33)
    assert ref["num_edges"] == 33 * 32 + 2 * 33
    assert np.all(ref["n_within"] == 35) and np.all(ref["thr"] == 32) and ref["self_rank"].tolist() == list(range(35))
    # 33 -> i and 34 -> i do not exist: the 66 edges into 33 and 34 have no mirror, 32 * 33 / 2 pairs have one
    c = ref["canon"][1]
    assert c["num_canon"] == 33 * 32 // 2 + 66 and int((c["c_mir"] < 0).sum()) == 66
    assert np.all(c["c_dst"][c["c_mir"] < 0] >= 33)
    # the wrong rules on the same molecule
    assert GR.build(_bondless(pos), rule="cap32")["num_edges"] == 32 * 31 + 3 * 32
    assert GR.build(_bondless(pos), rule="cap34")["num_edges"] == 34 * 33 + 34
    assert GR.build(_bondless(pos), rule="self_excluded_first")["num_edges"] == 35 * 33


# discriminating edges found, (only under the rule, only under the alternate): see the docstring below
SHELL_FOUND = {("shell10", "reordered"): (21, 20), ("shell10", "fma"): (19, 32), ("shell10", "float64"): (38, 155),
               ("shell3.7", "reordered"): (26, 28), ("shell3.7", "fma"): (17, 35), ("shell3.7", "float64"): (26, 135)}


@pytest.mark.parametrize("rule", ["reordered", "fma", "float64"])
@pytest.mark.parametrize("name", ["shell10", "shell3.7"])
def test_shell_batches_tell_the_rule_from_other_arithmetic(name, rule):
    """On every shell batch each other way to compute or compare d2 gives another FINAL edge list (pairs that are no local edge and
    are not cut by the cap): at least 4 edges only under the rule and at least 4 only under the alternate.  Found (rule only /
    alternate only): cutoff 10: reordered sum 21 / 20, FMA chain 19 / 32, float64 38 / 155; cutoff 3.7: reordered 26 / 28, FMA
    17 / 35, float64 26 / 135 -- counting only edges whose OWN comparison flips; with those that follow from a moved 33rd place the
    lists differ by 33 / 35, 36 / 46, 132 / 178 and 38 / 45, 34 / 42, 118 / 147 of 16,129 / 16,146 edges.  The counts are pinned so
    that a change of the builders shows."""
    b, ref = GR.make_batch(name), GR.reference(name)
    N = b["batch"].shape[0]
    alt = GR.build(b, rule=rule)
    pos, li = b["pos"], np.arange(N) - ref["graph_ptr"][b["batch"]]

    def direct(keys):
        """of the edges `keys` that one list has and the other lacks, those whose own comparison d2 < r2 comes out differently
        under the two rules (the others follow from one: a candidate more or less moves the 33rd place), each between a core atom
        and a shell atom placed at the cutoff from a core atom"""
        s, d = keys // N, keys % N
        flip = GR.in_range(GR.d2_of(pos[d], pos[s]), b["cutoff"]) != GR.in_range(GR.d2_of(pos[d], pos[s], rule), b["cutoff"], rule)
        assert np.all((li[s[flip]] < GR.SHELL_CORE) != (li[d[flip]] < GR.SHELL_CORE))
        return int(flip.sum())
    mine, theirs = direct(GR.only_in(ref, alt, N)), direct(GR.only_in(alt, ref, N))
    print("%s %s: %d edges only under the rule, %d only under the alternate" % (name, rule, mine, theirs))
    assert mine >= 4 and theirs >= 4
    assert (mine, theirs) == SHELL_FOUND[name, rule]
    ls, ld, _ = ref["loc"]
    assert not np.isin(np.concatenate([GR.only_in(ref, alt, N), GR.only_in(alt, ref, N)]), ls * N + ld).any()      # no local edge among them


def test_shell_batches_hold_exact_ties_and_an_inexact_r2():
    """Cutoff 10: r2 = 100 exactly, and a good part of the shell pairs are exact ties d2 == r2 (the strict < rejects them: "le"
    differs by 435 edges there, 483 at cutoff 3.7).  Cutoff 3.7: the float32 product 3.7f * 3.7f is not the exact square."""
    assert float(GR.r2_of(10.0)) == 100.0 == float(GR.r2_of(10.0, "float64"))
    assert float(GR.r2_of(3.7)) != float(GR.r2_of(3.7, "float64"))
    for name, found in (("shell10", 435), ("shell3.7", 483)):
        b, ref = GR.make_batch(name), GR.reference(name)
        N = b["batch"].shape[0]
        le = GR.build(b, rule="le")
        assert GR.only_in(ref, le, N).size + GR.only_in(le, ref, N).size == found >= 8
        rad = ref["e_len"][ref["e_type"] == 0]
        assert rad.max() == np.float32(b["cutoff"]) and (rad == np.float32(b["cutoff"])).sum() >= 8     # d2 < r2, length == cutoff


def test_lattice_batch_tells_less_than_from_less_or_equal():
    """Integer coordinates: 78 directed pairs at d2 == 100 exactly become edges under "le" and are none under the rule (at least 8
    asked for); pairs at 99 are edges, pairs at 101 are not; coincident atoms give length 0, once as a radius pair and once as a
    bonded pair."""
    b, ref = GR.make_batch("lattice"), GR.reference("lattice")
    N = b["batch"].shape[0]
    le = GR.build(b, rule="le")
    assert GR.only_in(ref, le, N).size == 0
    extra = GR.only_in(le, ref, N)
    assert extra.size == 78 >= 8
    p = b["pos"].astype(np.float64)
    d2 = lambda keys: ((p[keys // N] - p[keys % N]) ** 2).sum(1)
    assert np.all(d2(extra) == 100.0)
    mine = d2(GR.edge_keys(ref, N)[ref["e_type"] == 0])
    assert (mine == 99.0).sum() >= 8 and mine.max() == 99.0          # nothing at 100 or beyond
    n0 = b["sizes"][0]
    inside = np.arange(1, n0)
    assert (((p[inside] - p[0]) ** 2).sum(1) == 101.0).sum() >= 6     # pairs at 101 exist, and are no edges
    zero = ref["e_len"] == 0.0
    assert sorted(set(ref["e_type"][zero].tolist())) == [0, 1]       # length 0: a radius pair and a bonded pair
    assert ref["num_edges"] == 338
    assert np.all(ref["n_within"] <= CAP)                             # the cap never cuts here: every decision shows


CLUSTER_FOUND = {("clusters", "cap32"): (619, 0), ("clusters", "cap34"): (0, 581), ("clusters", "self_excluded_first"): (0, 378),
                 ("clusters520", "cap32"): (507, 0), ("clusters520", "cap34"): (0, 507), ("clusters520", "self_excluded_first"): (0, 429)}


@pytest.mark.parametrize("rule", ["cap32", "cap34", "self_excluded_first"])
@pytest.mark.parametrize("name", ["clusters", "clusters520"])
def test_cluster_batches_tell_the_cap_rule_from_its_neighbours(name, rule):
    """A cap of 32 or 34 and "self removed before counting to 33" each give another edge list.  Found (rule only / alternate
    only): clusters: cap32 619 / 0, cap34 0 / 581, self first 0 / 378; clusters520: 507 / 0, 0 / 507, 0 / 429."""
    b, ref = GR.make_batch(name), GR.reference(name)
    N = b["batch"].shape[0]
    alt = GR.build(b, rule=rule)
    found = (GR.only_in(ref, alt, N).size, GR.only_in(alt, ref, N).size)
    print(name, rule, found)
    assert sum(found) > 0 and found == CLUSTER_FOUND[name, rule]


def test_cluster_batches_hold_every_placement():
    """From the reference's own intermediate counts: targets with exactly 32, 33, 34 and 35 candidates; self before the 33rd
    candidate, as the 33rd, as the 34th and beyond; the 33rd candidate at index 63, 64, 127 and 128; a capped target without a
    radius row (all 33 kept candidates local sources or itself); unpaired radius edges with src < dst and with src > dst; the
    520-atom molecule capped everywhere with its 33rd candidate past index 416."""
    b, ref = GR.make_batch("clusters"), GR.reference("clusters")
    gp, nw, thr, sr = ref["graph_ptr"], ref["n_within"], ref["thr"], ref["self_rank"]
    N = b["batch"].shape[0]
    m0 = slice(gp[0], gp[1])
    assert sorted(set(nw[m0].tolist())) == [32, 33, 34, 35]
    assert np.array_equal(np.bincount(nw[m0])[32:], [32, 33, 34, 35])
    big = nw[m0] == 35
    assert {int(r) for r in sr[m0][big]} == set(range(35))            # ranks 0..31 before, 32 = the 33rd, 33 = the 34th, 34 after
    assert np.all(thr[m0][nw[m0] == 32] == -1) and np.all(thr[m0][nw[m0] >= 33] >= 0)
    for g, idx in zip(range(1, 5), GR.CAP_INDICES):
        mine = np.arange(gp[g], gp[g + 1])[GR._cap_at(idx, gp[g + 1] - gp[g]) == 0]
        assert np.all(thr[mine] == idx) and np.all(nw[mine] == CAP + 3)
        # the members behind the 33rd are sources of nobody, the 33rd is a source of every other member
        src_of = lambda i: set(ref["e_src"][ref["in_ptr"][i]:ref["in_ptr"][i + 1]].tolist())
        assert gp[g] + idx in src_of(mine[0]) and gp[g] + idx + 1 not in src_of(mine[0])
    centre = gp[5]
    assert nw[centre] == 53 and thr[centre] == 32 and ref["rad_cnt"][centre] == 0
    assert ref["in_ptr"][centre + 1] - ref["in_ptr"][centre] == 52     # ... and its 52 local in-edges are all there
    c = ref["canon"][1]
    un = c["c_mir"] < 0
    assert (un & (c["c_src"] < c["c_dst"])).sum() > 0 and (un & (c["c_src"] > c["c_dst"])).sum() > 0
    w = GR.ONE_WAY
    i, j = gp[6] + w["i"], gp[6] + w["j"]
    keys = set(GR.edge_keys(ref, N).tolist())
    assert j * N + i in keys and i * N + j not in keys and nw[i] == 2 and nw[j] == w["block"] + 2
    k = np.nonzero((c["c_src"] == j) & (c["c_dst"] == i))[0]
    assert k.size == 1 and c["c_mir"][k[0]] == -1                       # canonical, unpaired, src > dst
    ls, ld, _ = ref["loc"]
    assert not np.any((ls == j) & (ld == i))                            # (and no local edge)
    big = GR.reference("clusters520")
    assert GR.make_batch("clusters520")["sizes"][0] == 520 > 512
    assert np.all(big["n_within"][:520] == 40) and np.array_equal(big["thr"][:520], 416 + np.arange(520) % 13)


def test_the_batches_reach_every_launch_shape():
    """(threads, mask words, dynamic LDS bytes, rounds of the scan over the graphs) of the LDS build, recomputed from the launcher's
    rule (csrc/graph.hip): every word count from 2 to 16 the sizes select, the first size past 48 KiB of LDS (385 atoms: the
    launcher raises the kernel's limit there), the 512-thread launch from 512 graphs on, and the carry between the 1024-blocks of
    k_scan_graphs past 1024 graphs with zero counts inside the scan."""
    shape = {n: GR.launch_shape(GR.make_batch(n)) for n in GR.BATCHES if n.startswith(("max", "graphs"))}
    want = {"max1": (1024, 2), "max2": (1024, 2), "max63": (1024, 2), "max64": (1024, 2), "max65": (1024, 4), "max128": (1024, 4),
            "max129": (1024, 6), "max384": (1024, 12), "max385": (1024, 14), "max512": (1024, 16), "graphs511": (1024, 2),
            "graphs512": (512, 2), "graphs1024": (512, 2), "graphs1025": (512, 2), "graphs2050": (512, 2)}
    assert {n: s[:2] for n, s in shape.items()} == want
    assert shape["max384"][2] <= 48 * 1024 < shape["max385"][2] and shape["max512"][2] <= 152 * 1024
    assert [shape["graphs%d" % g][3] for g in GR.SHAPE_GRAPHS] == [1, 1, 1, 2, 3]
    for n in shape:
        b = GR.make_batch(n)
        if n.startswith("max"):
            assert max(b["sizes"]) == int(n[3:]) and (int(n[3:]) <= 2 or sorted(b["sizes"])[:3] == [1, 2, 23])
        else:
            ref = GR.reference(n)
            cnt = ref["graph_edge_cnt"]
            assert set(b["sizes"]) >= {1, 2, 3} and b["num_graphs"] == int(n[6:]) and b["batch"].shape[0] <= 4000
            assert (cnt == 0).sum() > b["num_graphs"] // 4 and (cnt[1:-1] == 0).any() and (cnt > 0).sum() > b["num_graphs"] // 4
            assert (ref["e_type"] == 0).sum() >= 16                   # radius pairs inside the cutoff: the counts are not all local
            if b["num_graphs"] > 1024:                                  # a zero count on the first slot of a later scan round
                assert cnt[1024:].sum() > 0 and cnt[:1024].sum() > 0
    assert GR.launch_shape(GR.make_batch("clusters"))[:2] == (1024, 6) and max(GR.make_batch("clusters520")["sizes"]) > 512
    assert GR.reference("max1")["num_edges"] == 0                       # a batch without any edge


def test_an_empty_molecule_is_accepted():
    """BatchTopology takes a molecule without atoms (graph_ptr[g] == graph_ptr[g + 1]): graphs1025 has one in the middle, and the
    topology, the reference and the oracle agree on everything around it."""
    from agdiff_amd.topology import BatchTopology
    b = GR.make_batch("graphs%d" % GR.EMPTY_IN)
    assert b["sizes"][700] == 0 and b["sizes"].count(0) == 1 and 700 not in set(b["batch"].tolist())
    topo = BatchTopology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], b["num_graphs"], device="cpu")
    gp = topo.graph_ptr.numpy()
    assert topo.G == GR.EMPTY_IN and gp[700] == gp[701] and np.array_equal(np.diff(gp), b["sizes"])
    ref = GR.reference("graphs%d" % GR.EMPTY_IN)
    assert ref["graph_edge_cnt"][700] == 0 and ref["graph_edge_ptr"][700] == ref["graph_edge_ptr"][701]
    assert torch.equal(topo.lcm_ptr[700], topo.lcm_ptr[701])
