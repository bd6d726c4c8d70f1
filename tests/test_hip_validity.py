"""GPU (MI355X): the geometry checks (agdiff_amd.validity; csrc/eval.hip: k_pair_bounds, k_clash_scan, k_clash_finish) against the
float64 numpy restatement of their definitions (tests/validity_ref.py), and through the prune, the driver and the command lines.

Gates, none taken from what the kernels give:
  VR.GATE   4 x 2^-24 = 2.4e-7 relative, for dist, worst and min_ratio: kernel and reference both compute in fp64 from the same fp32
            coordinates, so they differ by the final fp32 store (half an ulp, 2^-24 relative) plus at most an fp64 ulp where the
            compiler contracts a multiply-add.  Counts and indices must be equal exactly.
  VR.MARGIN for exact counts and indices to be a fair demand the reference asserts on its own output, before the kernel is asked
            anything, that no distance or ratio lies within 1e-5 (relative) of the bound or threshold that decides its count and that
            the best and second-best value of a conformer are that far apart.  The seeds below were chosen on the CPU so that it holds.
  MOVE_ATOL 1e-6 on min_ratio after a rigid motion done in fp64 and rounded to fp32 again: every coordinate stays below 16 in
            magnitude (asserted), where fp32's spacing is at most 2^-20, so rounding moves a coordinate by at most 2^-21, an atom by
            at most sqrt(3) 2^-21 and a distance by at most twice that, 1.65e-6 Angstrom; the radii are >= 1, so a ratio moves by at
            most 8.3e-7, and its own fp32 store (ratio < 1: 2^-25) stays inside the rest.  That test asserts margins of 4 x MOVE_ATOL
            in the reference first, so that counts and indices cannot move."""
import functools
import glob

import numpy as np
import pytest
import torch

import validity_ref as VR

pytestmark = pytest.mark.gpu
MOVE_ATOL = 1e-6


def _gpu(pos):
    return torch.from_numpy(np.array(pos, dtype=np.float32)).cuda()        # (a copy: the cached cases are read-only)


def _item(mol, **kw):
    at, ei, et = mol
    return dict(atom_type=at, edge_index=ei, edge_type=et, **kw)


def _close(got, want):
    """every entry within VR.GATE (relative) of the reference; infinities and NaNs in the same places"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    if not (np.array_equal(fin, np.isfinite(got)) and np.array_equal(np.isnan(want), np.isnan(got))):
        return False
    if not np.array_equal(np.sign(want[~fin & ~np.isnan(want)]), np.sign(got[~fin & ~np.isnan(want)])):
        return False
    return bool((np.abs(got[fin] - want[fin]) <= VR.GATE * np.abs(want[fin])).all())


def _walk(rng, G, bonds, n, step=1.5):
    """float32 [G, n, 3]: every atom one step of `step` Angstrom in a random direction from its parent in the tree"""
    pos = np.zeros((G, n, 3))
    for parent, a, _ in bonds:
        d = rng.normal(size=(G, 3))
        pos[:, a] = pos[:, parent] + step * d / np.linalg.norm(d, axis=1, keepdims=True)
    return (pos - pos.mean(1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. bounded pairs
def _bounds_inputs(n, G, K, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.normal(size=(G, n, 3)) * 1.5).astype(np.float32)
    pairs = np.stack([rng.permutation(n)[:2] for _ in range(K)]).astype(np.int32).reshape(-1, 2) if K else np.zeros((0, 2), np.int32)
    lo = rng.uniform(0.5, 3.0, size=K).astype(np.float32)
    hi = (lo + rng.uniform(0.0, 2.0, size=K)).astype(np.float32)
    return pos, pairs, lo, hi


BOUNDS_CASES = [(2, 1, 1), (9, 3, 0), (23, 10, 12), (61, 33, 70), (200, 40, 130)]
BOUNDS_SEED_SHIFT = {(200, 40, 130): 1}      # (seed + 0 puts a distance within 1e-5 of its bound: the reference's own margin fails)


@functools.lru_cache(maxsize=None)
def _bounds_case(n, G, K):
    """(inputs, the reference's results) -- computed once, margins asserted before any kernel runs"""
    pos, pairs, lo, hi = _bounds_inputs(n, G, K, 1000 * n + K + BOUNDS_SEED_SHIFT.get((n, G, K), 0))
    want = VR.pair_bounds(pos, pairs, lo, hi)
    VR.assert_bounds_margins(want[0], want[1], lo, hi)
    for a in (pos, pairs, lo, hi) + want:
        a.setflags(write=False)
    return (pos, pairs, lo, hi), want


@pytest.mark.parametrize("n,G,K", BOUNDS_CASES)
def test_pair_bounds_match_the_float64_reference(n, G, K):
    from agdiff_amd.validity import pair_bounds
    (pos, pairs, lo, hi), (dist, viol, worst, wpair, nbad) = _bounds_case(n, G, K)
    got = pair_bounds(_gpu(pos), pairs, lo, hi, want_dist=True)
    w, wp, nb, d = (x.cpu().numpy() for x in got)
    assert w.dtype == d.dtype == np.float32 and wp.dtype == nb.dtype == np.int32
    assert w.shape == wp.shape == nb.shape == (G,) and d.shape == (G, K)
    if K:
        print("n = %d, G = %d, K = %d: largest relative difference of dist %.3e, of worst %.3e" % (
            n, G, K, (np.abs(d.astype(np.float64) - dist) / dist).max(), (np.abs(w.astype(np.float64) - worst) / np.maximum(worst, 1e-30)).max()))
    assert _close(d, dist) and _close(w, worst)
    assert np.array_equal(wp, wpair) and np.array_equal(nb, nbad)
    if K == 0:
        assert not w.any() and (wp == -1).all() and not nb.any()
    # without dist the three results are the same bits
    again = pair_bounds(_gpu(pos), pairs, lo, hi)
    assert again[3] is None and all(torch.equal(a, b) for a, b in zip(again[:3], got[:3]))


def test_equal_violations_take_the_lowest_pair():
    from agdiff_amd.validity import pair_bounds
    # small integers: squared distances, their roots (3, 4, 5) and the violations are exact on both sides
    pos = np.zeros((2, 6, 3), dtype=np.float32)
    pos[:, 1, 0], pos[:, 2, 1], pos[:, 3, :2], pos[:, 4, 2] = 3, 4, (3, 4), 7
    K = 140
    pairs = np.tile(np.array([[0, 1]], dtype=np.int32), (K, 1))        # d = 3, inside [2, 4]
    lo, hi = np.full(K, 2, np.float32), np.full(K, 4, np.float32)
    for k, pr in ((70, (0, 3)), (67, (1, 2)), (3, (2, 1)), (131, (0, 3))):      # d = 5: violation 1, in lanes 6, 3, 3, 3
        pairs[k] = pr
    want = VR.pair_bounds(pos, pairs, lo, hi)
    assert want[2].tolist() == [1.0, 1.0] and want[3].tolist() == [3, 3] and want[4].tolist() == [4, 4]
    w, wp, nb, _ = pair_bounds(_gpu(pos), pairs, lo, hi)
    assert w.tolist() == [1.0, 1.0] and wp.tolist() == [3, 3] and nb.tolist() == [4, 4]
    pairs[3] = (0, 1)
    assert pair_bounds(_gpu(pos), pairs, lo, hi)[1].tolist() == [67, 67]
    pairs[67] = (0, 1)
    assert pair_bounds(_gpu(pos), pairs, lo, hi)[1].tolist() == [70, 70]
    pairs[130] = (0, 4)                                                 # d = 7: violation 3 beats them all
    w, wp, nb, _ = pair_bounds(_gpu(pos), pairs, lo, hi)
    assert w.tolist() == [3.0, 3.0] and wp.tolist() == [130, 130] and nb.tolist() == [3, 3]


def test_a_pair_outside_the_molecule_is_an_infinite_violation_and_reads_nothing():
    from agdiff_amd.validity import pair_bounds
    (pos, pairs, lo, hi), _ = _bounds_case(23, 10, 12)
    far = pairs.copy()
    far[5] = (3, 23 + 10 ** 8)                        # (400 MB past the tensor if it were read)
    far[9] = (-1, 2)
    want = VR.pair_bounds(pos, far, lo, hi)
    w, wp, nb, d = (x.cpu().numpy() for x in pair_bounds(_gpu(pos), far, lo, hi, want_dist=True))
    assert np.isposinf(w).all() and (wp == 5).all() and np.isnan(d[:, 5]).all() and np.isnan(d[:, 9]).all()
    assert _close(d, want[0]) and np.array_equal(nb, want[4]) and np.array_equal(wp, want[3])


# ------------------------------------------------------------------------------------------------ 2. clash scan
# (kind, n, G, seed): seeds chosen on the CPU so that the reference's margins hold
CLASH_CASES = [("none", 2, 1, 0), ("full", 5, 4, 0), ("chain", 63, 3, 0), ("chain", 64, 3, 0), ("chain", 65, 33, 0), ("chain", 257, 5, 0),
               ("chain", 600, 2, 0), ("star", 41, 3, 0), ("star", 71, 3, 0), ("none", 30, 2, 0)]
THRESH = 0.6


def _clash_inputs(kind, n, G, seed):
    """(pos fp32 [G, n, 3], radius fp32 [n], ex_ptr, ex_idx): "chain" a random tree with the exclusions of its order-3 bond list;
    "full" the same with every pair excluded (n = 5: everything is within three bonds of a path... made so by a star); "star" one
    atom with n - 1 neighbours and the RAW bonds as exclusions (its row is n - 1 long, the leaves' pairs stay); "none" no exclusions"""
    from agdiff_amd.validity import exclusions
    rng = np.random.default_rng(7919 * n + 31 * G + seed)
    if kind in ("star", "full"):
        bonds = [(0, a, 1) for a in range(1, n)]
        mol = VR.graph([6] * n, bonds, order=1 if kind == "star" else 3)
    else:
        mol, bonds = VR.random_chain(rng, n)
    pos = _walk(rng, G, bonds, n)
    radius = rng.uniform(1.0, 2.0, size=n).astype(np.float32)
    if kind == "none":
        ex_ptr, ex_idx = np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)
    else:
        ex_ptr, ex_idx = exclusions(n, mol[1], mol[2])
    return pos, radius, ex_ptr, ex_idx


@functools.lru_cache(maxsize=None)
def _clash_case(kind, n, G, seed):
    pos, radius, ex_ptr, ex_idx = _clash_inputs(kind, n, G, seed)
    want = VR.clash_scan(pos, radius, VR.excluded_set(ex_ptr, ex_idx), THRESH)
    VR.assert_clash_margins(want[3], THRESH)
    for a in (pos, radius, ex_ptr, ex_idx) + want:
        a.setflags(write=False)
    return (pos, radius, ex_ptr, ex_idx), want


@pytest.mark.parametrize("kind,n,G,seed", CLASH_CASES)
def test_clash_scan_matches_the_float64_reference(kind, n, G, seed):
    from agdiff_amd.validity import clash_scan
    (pos, radius, ex_ptr, ex_idx), (ratio, pair, count, vals) = _clash_case(kind, n, G, seed)
    if kind == "star":
        assert ex_ptr[1] == n - 1
    r, p, c = (x.cpu().numpy() for x in clash_scan(_gpu(pos), radius, ex_ptr, ex_idx, THRESH))
    assert r.dtype == np.float32 and p.dtype == c.dtype == np.int32 and r.shape == c.shape == (G,) and p.shape == (G, 2)
    print("%s n = %d, G = %d: %d pairs per conformer, %s clashes, min ratios %s" % (kind, n, G, vals.shape[1], count.tolist()[:4],
                                                                                   ratio.tolist()[:4]))
    assert _close(r, ratio)
    assert np.array_equal(p, pair) and np.array_equal(c, count)
    if kind == "full":
        assert np.isposinf(r).all() and (p == -1).all() and not c.any()
    else:
        assert (0 <= p[:, 0]).all() and (p[:, 0] < p[:, 1]).all() and (p[:, 1] < n).all()


def _lattice(n):
    """float32 [n, 3]: atom a at 10 x (a % 8, (a / 8) % 8, a / 64): small integers, every pair at least 10 apart"""
    a = np.arange(n)
    return np.stack([10 * (a % 8), 10 * ((a // 8) % 8), 10 * (a // 64)], axis=1).astype(np.float32)


def test_equal_ratios_in_different_slices_take_the_lowest_pair():
    from agdiff_amd.validity import clash_scan
    n = 300
    radius = np.ones(n, dtype=np.float32)
    ex_ptr, ex_idx = np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)
    two, three = _lattice(n), _lattice(n)
    for p in (two, three):
        p[280] = p[270] + (0, 3, 0)                   # i = 270: slice 1
        p[290] = p[5] + (3, 0, 0)                     # i = 5: slice 0, j in slice 1's tile
    three[120] = three[5] + (0, 0, 3)                 # i = 5 again, a lower j in slice 0's own tile
    pos = np.stack([two, three])
    want = VR.clash_scan(pos, radius, set(), 1.75)
    assert want[0].tolist() == [1.5, 1.5] and want[1].tolist() == [[5, 290], [5, 120]] and want[2].tolist() == [2, 3]
    assert (np.sort(want[3], axis=1)[:, 3] >= 2.0).all()          # nothing else comes near
    r, p, c, scratch = clash_scan(_gpu(pos), radius, ex_ptr, ex_idx, 1.75, want_scratch=True)
    assert r.tolist() == [1.5, 1.5] and p.tolist() == [[5, 290], [5, 120]] and c.tolist() == [2, 3]
    # the partials: slice 0 holds atom 5's pairs, slice 1 the pair (270, 280) with the same bits
    s = scratch.cpu().numpy()
    assert s.shape == (2, 2, 4) and s[:, :, 0].view(np.float32).tolist() == [[1.5, 1.5], [1.5, 1.5]]
    assert s[:, :, 1:].tolist() == [[[5, 290, 1], [270, 280, 1]], [[5, 120, 2], [270, 280, 1]]]
    # the same with the roles turned: only the pair of slice 1 left, then one pair whose i is the LAST atom of slice 0
    alone = _lattice(n)
    alone[280] = alone[270] + (0, 3, 0)
    edge = _lattice(n)
    edge[256] = edge[255] + (0, 0, 3)
    assert clash_scan(_gpu(np.stack([alone, edge])), radius, ex_ptr, ex_idx, 1.75)[1].tolist() == [[270, 280], [255, 256]]


def _broken_batch():
    (pos, radius, ex_ptr, ex_idx), _ = _clash_case("chain", 65, 33, 0)
    clean = pos[:4].copy()
    broken = clean.copy()
    broken[2, 7, 1] = np.nan
    broken[2, 40, 0] = np.inf
    return clean, broken, radius, ex_ptr, ex_idx


def test_a_conformer_that_is_not_finite_is_the_worst_case_and_leaves_the_others_alone():
    from agdiff_amd.validity import clash_scan, pair_bounds
    clean, broken, radius, ex_ptr, ex_idx = _broken_batch()
    excluded = VR.excluded_set(ex_ptr, ex_idx)
    want = VR.clash_scan(broken, radius, excluded, THRESH)
    assert want[0][2] == 0.0 and want[2][2] > 60
    got = clash_scan(_gpu(broken), radius, ex_ptr, ex_idx, THRESH)
    base = clash_scan(_gpu(clean), radius, ex_ptr, ex_idx, THRESH)
    r, p, c = (x.cpu().numpy() for x in got)
    assert r[2] == 0.0 and np.array_equal(p, want[1]) and np.array_equal(c, want[2]) and _close(r, want[0])
    others = [0, 1, 3]
    assert all(torch.equal(a[others], b[others]) for a, b in zip(got, base))
    rng = np.random.default_rng(3)
    pairs = np.stack([rng.permutation(65)[:2] for _ in range(90)]).astype(np.int32)
    pairs[11], pairs[80] = (7, 3), (12, 40)
    lo, hi = np.full(90, 0.0, np.float32), np.full(90, 100.0, np.float32)
    wantb = VR.pair_bounds(broken, pairs, lo, hi)
    assert np.isposinf(wantb[2][2]) and wantb[3][2] <= 11 and wantb[4][2] >= 2 and not wantb[4][others].any()
    gotb = pair_bounds(_gpu(broken), pairs, lo, hi, want_dist=True)
    baseb = pair_bounds(_gpu(clean), pairs, lo, hi, want_dist=True)
    w, wp, nb, d = (x.cpu().numpy() for x in gotb)
    assert np.isposinf(w[2]) and np.array_equal(wp, wantb[3]) and np.array_equal(nb, wantb[4]) and _close(d, wantb[0])
    assert all(torch.equal(a[others], b[others]) for a, b in zip(gotb, baseb))


def test_check_geometry_calls_a_conformer_that_is_not_finite_invalid():
    from agdiff_amd.validity import check_geometry
    mol, pos = VR.alkane(4)
    gen = np.stack([pos] * 4).astype(np.float32)
    gen[1, 9, 2] = np.nan
    res = check_geometry(_item(mol, pos_gen=gen))
    assert res["valid"].tolist() == [True, False, True, True]
    assert res["clash"][1].item() == 0.0 and np.isposinf(res["bond_dev"][1].item()) and res["n_bad"][1].item() == 1
    assert res["n_clash"][1].item() >= 1 and res["bond_pair"][1].tolist() == [2, 9]


def test_two_calls_give_the_same_bits():
    from agdiff_amd.validity import clash_scan, pair_bounds
    (pos, radius, ex_ptr, ex_idx), _ = _clash_case("chain", 600, 2, 0)
    a = clash_scan(_gpu(pos), radius, ex_ptr, ex_idx, THRESH, want_scratch=True)
    b = clash_scan(_gpu(pos), radius, ex_ptr, ex_idx, THRESH, want_scratch=True)
    assert a[3].shape == (2, 3, 4) and all(torch.equal(x, y) for x, y in zip(a, b))
    (pos, pairs, lo, hi), _ = _bounds_case(200, 40, 130)
    a, b = (pair_bounds(_gpu(pos), pairs, lo, hi, want_dist=True) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_rigid_motion_keeps_counts_and_indices_and_moves_the_ratio_by_rounding_only():
    from agdiff_amd.validity import clash_scan
    (pos, radius, ex_ptr, ex_idx), (ratio, pair, count, vals) = _clash_case("chain", 63, 3, 0)
    low = np.sort(vals.astype(np.float64), axis=1)[:, :2]
    assert (low[:, 1] - low[:, 0] > 4 * MOVE_ATOL).all() and (np.abs(vals.astype(np.float64) - THRESH) > 4 * MOVE_ATOL).all()
    rng = np.random.default_rng(11)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    moved = (pos.astype(np.float64) @ q.T + np.array([1.5, -2.0, 0.7])).astype(np.float32)
    assert np.abs(moved).max() < 16 and np.abs(pos).max() < 16 and radius.min() >= 1.0
    r, p, c = (x.cpu().numpy() for x in clash_scan(_gpu(moved), radius, ex_ptr, ex_idx, THRESH))
    assert np.array_equal(p, pair) and np.array_equal(c, count)
    print("largest move of min_ratio under a rigid motion: %.3e" % np.abs(r.astype(np.float64) - ratio).max())
    assert np.abs(r.astype(np.float64) - ratio).max() <= MOVE_ATOL


# ------------------------------------------------------------------------------------------------ 3. molecules
def test_hand_built_alkanes_under_the_default_tables():
    from agdiff_amd.validity import check_geometry
    mol, pos = VR.alkane(4)
    stretched = pos.copy()
    stretched[5] = pos[0] + (pos[5] - pos[0]) * (1.8 / 1.09)
    _, folded = VR.folded_butane(1.9)
    res = check_geometry(_item(mol, pos_gen=np.stack([pos, stretched, folded])))
    assert res["valid"].dtype == torch.bool and res["bond_dev"].dtype == res["clash"].dtype == torch.float32
    assert all(res[k].dtype == torch.int32 for k in ("bond_pair", "n_bad", "clash_pair", "n_clash"))
    assert res["bond_pair"].shape == res["clash_pair"].shape == (3, 2)
    assert res["valid"].tolist() == [True, False, True]
    assert res["n_bad"].tolist() == [0, 1, 0] and res["n_clash"].tolist() == [0, 0, 0]
    assert res["bond_pair"][1].tolist() == [0, 5] and abs(res["bond_dev"][1].item() - (1.8 - 1.2 * 1.07)) < 1e-6
    assert res["bond_dev"][0].item() == 0.0 and res["clash"].min().item() > 0.6
    mol5, pos5 = VR.alkane(5)
    _, folded5 = VR.folded_pentane(1.9)
    res = check_geometry(_item(mol5, pos_gen=np.stack([pos5, folded5])))
    assert res["valid"].tolist() == [True, False] and res["n_bad"].tolist() == [0, 0] and res["n_clash"][1].item() >= 1
    assert res["clash_pair"][1].tolist() == [0, 4] and abs(res["clash"][1].item() - 1.9 / 3.4) < 1e-6
    # the other two kinds of bounds: the references' own spread (all three conformers are their own references: valid), and a table
    refs = check_geometry(_item(mol5, pos_gen=np.stack([pos5, folded5]), pos_ref=np.stack([pos5, folded5])), bounds="references", clash=0.5)
    assert refs["valid"].tolist() == [True, True]
    tight = check_geometry(_item(mol5, pos_gen=np.stack([pos5, folded5]), pos_ref=pos5[None]), bounds="references")
    assert tight["n_bad"][0].item() == 0 and tight["n_bad"][1].item() >= 2          # the folded chain's 1-3 distances moved
    own = check_geometry(_item(mol5, pos_gen=pos5[None]), bounds=(np.array([[0, 4]]), [1.0], [2.0]))
    assert own["n_bad"].tolist() == [1] and own["bond_pair"].tolist() == [[0, 4]]
    none = check_geometry(_item(mol5, pos_gen=pos5[None]), bounds=(np.zeros((0, 2), np.int32), [], []))
    assert none["bond_pair"].tolist() == [[-1, -1]] and none["valid"].tolist() == [True]


# ------------------------------------------------------------------------------------------------ 4. prune
BROKEN = (2, 6, 11)


@functools.lru_cache(maxsize=None)
def _twelve():
    """n-butane: anti, gauche+ and gauche- three times each with a little noise, and three conformers whose C3 - C4 bond is stretched
    by 1.5, 3 and 4.5 Angstrom (the methyl group moved as one) at BROKEN"""
    rng = np.random.default_rng(2)
    confs, mol = [], None
    good = iter([t for _ in range(3) for t in (np.pi, np.pi / 3, -np.pi / 3)])
    stretch = iter((1.5, 3.0, 4.5))
    for g in range(12):
        if g in BROKEN:
            mol, pos = VR.alkane(4)
            move = [3, 11, 12, 13]                    # C4 and its hydrogens
            pos[move] += next(stretch) * (pos[3] - pos[2]) / np.linalg.norm(pos[3] - pos[2])
        else:
            mol, pos = VR.alkane(4, torsions=[next(good)])
        confs.append(pos + 0.005 * rng.normal(size=pos.shape))
    gen = np.stack(confs).astype(np.float32)
    gen.setflags(write=False)
    return mol, gen


def test_the_prune_keeps_every_broken_conformer_unless_told_which_are_valid():
    from agdiff_amd.ensemble import prune_conformers
    from agdiff_amd.validity import check_geometry
    mol, gen = _twelve()
    item = _item(mol, pos_gen=gen)
    valid = check_geometry(item)["valid"]
    good = [g for g in range(12) if g not in BROKEN]
    assert valid.tolist() == [g not in BROKEN for g in range(12)]
    # the defect: a broken conformer is far from everything, so the leader rule keeps all three
    blind = prune_conformers(item, 0.2, align=False)
    assert set(BROKEN) <= set(blind["kept"].tolist()) and blind["kept"].tolist() == [0, 1, 2, 3, 6, 11]
    for mask in (valid, valid.cpu().numpy()):
        res = prune_conformers(item, 0.2, align=False, valid=mask)
        assert res["kept"].dtype == res["leader"].dtype == torch.int32
        assert res["kept"].tolist() == [0, 1, 3] and not set(BROKEN) & set(res["kept"].tolist())
        leader = res["leader"].cpu().numpy()
        assert np.array_equal(np.nonzero(leader == -1)[0], BROKEN)
        alone = prune_conformers(_item(mol, pos_gen=gen[good]), 0.2, align=False)
        back = np.array(good)
        assert np.array_equal(res["kept"].cpu().numpy(), back[alone["kept"].cpu().numpy()])
        assert np.array_equal(leader[good], back[alone["leader"].cpu().numpy()])
        assert torch.equal(res["count"], alone["count"]) and res["count"].tolist() == [3, 3, 3]
        assert torch.equal(res["pos"], alone["pos"]) and torch.equal(res["pos"].cpu(), torch.from_numpy(gen[[0, 1, 3]]))
    aligned = prune_conformers(item, 0.2, align=True, valid=valid, metric="tfd")
    assert aligned["kept"].tolist() == [0, 1, 3] and torch.equal(aligned["pos"][0].cpu(), torch.from_numpy(gen[0]))
    nothing = prune_conformers(item, 0.2, valid=np.zeros(12, dtype=bool))
    assert nothing["kept"].shape == (0,) and nothing["count"].shape == (0,) and nothing["pos"].shape == (0, 14, 3)
    assert nothing["leader"].tolist() == [-1] * 12
    everything = prune_conformers(item, 0.2, align=False, valid=np.ones(12, dtype=bool))
    assert torch.equal(everything["kept"], blind["kept"]) and torch.equal(everything["leader"], blind["leader"])


# ------------------------------------------------------------------------------------------------ 5. driver and command lines
def test_run_job_saves_the_verdicts_with_the_switch_and_nothing_new_without_it(tmp_path):
    from agdiff_amd import driver, ensemble, get_model, qm9_model_config, synth, validity
    from agdiff_amd.validity import check_geometry
    m = get_model(qm9_model_config(num_diffusion_timesteps=8))
    m.load_state_dict(synth.synth_state_dict(m.state_dict()))
    m = m.to("cuda:0").eval()
    at, r, c, ty = synth.random_molecule(np.random.default_rng(5), 13)
    mols = [dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=ty, num_refs=5, name="mol0", index=0)]
    confs = lambda num_refs: num_refs
    kw = dict(n_steps=4, step_lr=1e-6, w_global=1.0, clip=1000.0)
    logs = []
    res = driver.run_job(m, mols, str(tmp_path / "checked"), confs, 10 ** 6, kw, "cuda:0", log=logs.append, check_geometry=True)
    files = glob.glob(str(tmp_path / "checked" / "samples_[0-9]*.npz"))
    assert len(files) == 1 and sum("conformers are invalid" in str(x) for x in logs) == 1
    item = lambda pos: dict(atom_type=at, pos_gen=pos, edge_index=mols[0]["edge_index"], edge_type=ty)
    for z in (res, np.load(files[0]), np.load(str(tmp_path / "checked" / "samples_all.npz"))):
        assert set(z.keys() if isinstance(z, dict) else z.files) == {"pos_gen_0", "name_0", "valid_0", "bond_dev_0", "clash_0"}
        assert z["valid_0"].dtype == np.int8 and z["bond_dev_0"].dtype == np.float32 and z["clash_0"].dtype == np.float32
        assert z["valid_0"].shape == z["bond_dev_0"].shape == z["clash_0"].shape == (5,) and z["pos_gen_0"].shape == (5, 13, 3)
        want = check_geometry(item(z["pos_gen_0"]))
        assert np.array_equal(z["valid_0"], want["valid"].cpu().numpy().astype(np.int8))
        assert np.array_equal(z["bond_dev_0"], want["bond_dev"].cpu().numpy()) and np.array_equal(z["clash_0"], want["clash"].cpu().numpy())
    plain = driver.run_job(m, mols, str(tmp_path / "plain"), confs, 10 ** 6, kw, "cuda:0", log=logs.append)
    assert set(plain.keys()) == {"pos_gen_0", "name_0"}
    assert set(np.load(glob.glob(str(tmp_path / "plain" / "samples_[0-9]*.npz"))[0]).files) == {"pos_gen_0", "name_0"}
    assert sum("conformers are invalid" in str(x) for x in logs) == 1
    # with a prune switch the mask goes to the walk: the invalid conformers lead nowhere
    both = driver.run_job(m, mols, str(tmp_path / "both"), confs, 10 ** 6, kw, "cuda:0", log=logs.append, check_geometry=True, prune_rms=0.5)
    assert set(both.keys()) == {"pos_gen_0", "name_0", "valid_0", "bond_dev_0", "clash_0", "kept_0", "cluster_0"}
    assert np.array_equal(both["cluster_0"] == -1, both["valid_0"] == 0) and both["valid_0"][both["kept_0"]].all()

    # the command lines on the first job's files
    driver.save_testset(str(tmp_path / "test.npz"), mols)
    samples = str(tmp_path / "checked" / "samples_all.npz")
    out = validity.main(["--samples", samples, "--testset", str(tmp_path / "test.npz"), "--out", str(tmp_path / "validity.npz")])
    z = np.load(str(tmp_path / "validity.npz"))
    assert set(z.files) == {k + "_0" for k in ("valid", "bond_dev", "bond_pair", "n_bad", "clash", "clash_pair", "n_clash", "name")}
    assert all(np.array_equal(z[k + "_0"], res[k + "_0"]) for k in ("valid", "bond_dev", "clash")) and str(z["name_0"]) == "mol0"
    assert z["valid_0"].dtype == np.int8 and z["bond_pair_0"].shape == z["clash_pair_0"].shape == (5, 2)
    assert np.array_equal(out["n_clash_0"], z["n_clash_0"]) and np.array_equal(z["valid_0"] == 1, (z["n_bad_0"] == 0) & (z["n_clash_0"] == 0))
    np.savez(str(tmp_path / "refs.npz"), pos_ref_0=res["pos_gen_0"])
    own = validity.main(["--samples", samples, "--testset", str(tmp_path / "test.npz"), "--refs", str(tmp_path / "refs.npz"), "--clash", "0",
                         "--out", str(tmp_path / "own.npz")])
    assert own["valid_0"].tolist() == [1] * 5          # every conformer is within the spread of the references it is one of
    pruned = ensemble.main(["--samples", samples, "--testset", str(tmp_path / "test.npz"), "--prune-rms", "0.5", "--drop-invalid",
                            "--out", str(tmp_path / "pruned.npz")])
    assert np.array_equal(pruned["valid_0"], res["valid_0"]) and np.array_equal(pruned["cluster_0"] == -1, res["valid_0"] == 0)
