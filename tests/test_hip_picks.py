"""GPU (MI355X): MaxMin picking (agdiff_amd.picks; csrc/eval.hip: k_maxmin_pick) against the numpy restatement of its rule
(tests/maxmin_ref.py) on the same float32 matrix -- integers equal, floats bit-equal, NaN at the same places -- and end to end
through pick_conformers and the command line.

The walk computes nothing: every float it writes is a copy of a matrix entry, so every comparison with the restatement is exact.
The one tolerance is ALIGN_ATOL, for the superposed picks against a float64 Kabsch of the same fp32 inputs: the bar that
tests/test_hip_ensemble.py carries for agdiff_align_conformers (4 x the 2.24e-7 Angstrom it measured), the same kernel under the
same bar; nothing new is measured here."""
import functools

import numpy as np
import pytest
import torch

import maxmin_ref as MR
import rings_ref as RR
import tfd_ref as TR
from test_hip_clusters import ALIGN_ATOL, GROUP4, _families, _kabsch_align, _moved, _relabel, seven_pattern_conformers

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL, FSENTINEL, TAIL = -7, -777.0, 64           # (no output is negative but the -1 of picks / owner)


def _launch(dist, G, K, first=0, stop=-1.0):
    """agdiff_maxmin_pick on a device tensor [G, G] (or a numpy matrix), its six arrays filled with a sentinel and followed by a
    canary tail: every entry must have been written, the tails must be as they were.  The result in the restatement's form."""
    from agdiff_amd import _lib
    dev = dist if torch.is_tensor(dist) else torch.from_numpy(np.array(dist, dtype=F32)).cuda()
    ints = [torch.full((m + TAIL,), SENTINEL, dtype=torch.int32, device="cuda") for m in (K, G, 1)]
    floats = [torch.full((m + TAIL,), FSENTINEL, dtype=torch.float32, device="cuda") for m in (K, G, 1)]
    _lib.call("agdiff_maxmin_pick", dev, G, K, int(first), float(stop), ints[0], floats[0], ints[1], floats[1], ints[2], floats[2])
    picks, owner, n = (a.cpu().numpy() for a in ints)
    radius, near, cover = (a.cpu().numpy() for a in floats)
    for a, m in ((picks, K), (owner, G), (n, 1)):
        assert (a[m:] == SENTINEL).all() and (a[:m] != SENTINEL).all()
    for a, m in ((radius, K), (near, G), (cover, 1)):
        assert (a[m:] == FSENTINEL).all() and not (a[:m] == FSENTINEL).any()
    assert ((picks[:K] >= -1) & (picks[:K] < G)).all() and ((owner[:G] >= -1) & (owner[:G] < K)).all() and 1 <= n[0] <= K
    return picks[:K], radius[:K], owner[:G], near[:G], int(n[0]), cover[0]


@functools.lru_cache(maxsize=None)
def _metric(G):
    """(matrix, the same on the device, its median entry) of a seeded random metric matrix -- made once, left unchanged"""
    d = MR.random_metric(G, seed=G)
    d.setflags(write=False)
    return d, torch.from_numpy(np.array(d)).cuda(), float(np.median(d))


# ------------------------------------------------------------------------------------------------ 1. the kernel against the rule
@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096])
def test_kernel_equals_the_restated_rule(G):
    """across a wave, the block (two columns per thread from 1025) and the limit (four columns per thread); K = G = 4096 is the
    longest loop there is"""
    d, dev, med = _metric(G)
    for K in sorted({1, min(7, G), G}):
        for first in sorted({0, G - 1}):
            for stop in (-1.0, med):
                want = MR.maxmin(d, K, first=first, stop=stop)
                got = _launch(dev, G, K, first=first, stop=stop)
                assert MR.same(got, want), "G = %d, K = %d, first = %d, stop = %g" % (G, K, first, stop)
                if stop < 0 and K == G:
                    assert got[4] == G and got[5] == 0 and sorted(got[0].tolist()) == list(range(G))
    MR.check_invariants(d, _launch(dev, G, min(7, G)), min(7, G), -1.0)


def test_two_launches_give_equal_tensors_through_the_wrapper():
    from agdiff_amd.picks import maxmin_pick
    for G, K in ((1000, 100), (4096, 10)):
        d, dev, _ = _metric(G)
        a, b = maxmin_pick(dev, G, K), maxmin_pick(dev, G, K)
        assert [x.dtype for x in a] == [torch.int32, torch.float32, torch.int32, torch.float32, torch.int32, torch.float32]
        assert [tuple(x.shape) for x in a] == [(K,), (K,), (G,), (G,), (1,), (1,)] and all(x.is_cuda for x in a)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
        want = MR.maxmin(d, K)
        assert MR.same(tuple(x.cpu().numpy() for x in a[:4]) + (int(a[4].item()), a[5].cpu().numpy()[0]), want)
        c = maxmin_pick(dev, G, K, stop=float(want[1][K // 2]), first=G - 1)
        assert MR.same(tuple(x.cpu().numpy() for x in c[:4]) + (int(c[4].item()), c[5].cpu().numpy()[0]),
                       MR.maxmin(d, K, first=G - 1, stop=float(want[1][K // 2])))


# ------------------------------------------------------------------------------------------------ 2. ties
@pytest.mark.parametrize("G", [65, 1025, 2500])
def test_ties_go_to_the_lowest_index_and_the_earlier_pick(G):
    d = MR.small_values(G, seed=G)                           # entries 1, 2, 3: nearly every arg-max and every min-update is a tie
    for K, first, stop in ((G, 0, -1.0), (G, G - 1, 1.0), (min(40, G), G // 2, 2.0)):
        assert MR.same(_launch(d, G, K, first=first, stop=stop), MR.maxmin(d, K, first=first, stop=stop)), (K, first, stop)
    same = np.full((G, G), 2.5, dtype=F32)                   # the all-equal matrix: the picks come out in index order
    picks, radius, owner, near, n, cover = _launch(same, G, G, first=2)
    assert picks.tolist() == [2] + [j for j in range(G) if j != 2] and (radius[1:] == 2.5).all() and n == G and cover == 0
    assert np.array_equal(owner[picks], np.arange(G)) and not near.any()
    picks, radius, owner, near, n, cover = _launch(same, G, 5)
    assert picks.tolist() == [0, 1, 2, 3, 4] and cover == 2.5 and (owner[5:] == 0).all() and (near[5:] == 2.5).all()


@pytest.mark.parametrize("G", [1, 65, 1025])
def test_the_zero_matrix(G):
    zero = np.zeros((G, G), dtype=F32)
    picks, radius, owner, near, n, cover = _launch(zero, G, G, stop=0.0)         # 0 > 0 is false: one pick
    assert n == 1 and cover == 0 and picks.tolist() == [0] + [-1] * (G - 1) and np.isnan(radius[1:]).all() and radius[0] == np.inf
    assert not owner.any() and not near.any()
    got = _launch(zero, G, G, stop=-1.0)                                         # no threshold: everybody, in index order
    assert got[0].tolist() == list(range(G)) and got[4] == G and got[5] == 0 and not got[1][1:].any()
    assert MR.same(got, MR.maxmin(zero, G))


# ------------------------------------------------------------------------------------------------ 3. eligibility
@pytest.mark.parametrize("G", [65, 1025])
def test_ineligible_conformers(G):
    d = _metric(G)[0]
    rng = np.random.default_rng(G)
    for bad in ([G // 2], [1, 62, 63, G - 1], sorted(rng.choice(np.arange(1, G), size=G // 3, replace=False).tolist())):
        m = MR.with_inf(d, bad)                              # +inf rows and columns, the diagonal 0: as agdiff_rmsd_self writes them
        for K in (7, G):
            got = _launch(m, G, K)
            assert MR.same(got, MR.maxmin(m, K))
            assert (got[2][bad] == -1).all() and np.isnan(got[3][bad]).all() and (np.delete(got[2], bad) >= 0).all()
            assert got[4] == min(K, G - len(bad)) and not set(bad) & set(got[0].tolist())
    # a first pick whose own row is all +inf: one pick, everybody else ineligible
    m = MR.with_inf(d, [5])
    picks, radius, owner, near, n, cover = _launch(m, G, G, first=5)
    assert n == 1 and cover == 0 and picks[0] == 5 and (picks[1:] == -1).all() and owner[5] == 0 and near[5] == 0
    assert (np.delete(owner, 5) == -1).all() and np.isnan(np.delete(near, 5)).all()
    # an isolated NaN in the first pick's row, a negative entry and a -inf in later picks' rows
    base = MR.maxmin(d, G)
    second, third = int(base[0][1]), int(base[0][2])
    late = [int(j) for j in base[0][G // 2:G // 2 + 3]]      # conformers that are picked late: unpicked when those rows are read
    m = d.copy()
    m[0, late[2]] = np.nan
    m[second, late[0]] = -1.0
    m[third, late[1]] = -np.inf
    m[second, 0] = np.nan                                    # (a picked column: never looked at)
    m[np.arange(G), np.arange(G)] = np.nan                   # (the diagonal is never trusted)
    got = _launch(m, G, G)
    assert MR.same(got, MR.maxmin(m, G)) and got[4] == G - 3
    assert (got[2][late] == -1).all() and (np.delete(got[2], late) >= 0).all()


@pytest.mark.parametrize("G", [65, 1025])
def test_minus_zero_entries_are_zeros(G):
    d = _metric(G)[0].copy()
    dup = np.arange(0, G, 3)                                 # conformer 3 i + 1 coincides with conformer 3 i
    dup = dup[dup + 1 < G]
    d[dup + 1] = d[dup]
    d[:, dup + 1] = d[:, dup]
    d[np.arange(G), np.arange(G)] = 0
    assert np.array_equal(d, d.T) and (d[dup, dup + 1] == 0).all()
    neg = np.where(d == 0, F32(-0.0), d)
    assert np.signbit(neg[dup, dup + 1]).all()
    for stop in (-1.0, 0.0):
        want = MR.maxmin(d, G, stop=stop)
        got = _launch(neg, G, G, stop=stop)
        assert MR.same(got, want) and MR.same(_launch(d, G, G, stop=stop), want)
        assert not np.signbit(got[1][:got[4]]).any() and not np.signbit(got[3]).any()
    assert want[4] == G - dup.size                           # at stop = 0 a duplicate of a pick is never taken


# ------------------------------------------------------------------------------------------------ 4. alignment, 5. nothing to do
@pytest.mark.parametrize("G", [63, 1023, 1025])
def test_matrix_one_float_into_its_allocation(G):
    """dist needs 4-byte alignment only; with G odd no row of it is 8-byte aligned"""
    d, _, med = _metric(G)
    buf = torch.full((G * G + 2,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    off = buf[1:1 + G * G].view(G, G)
    off.copy_(torch.from_numpy(np.array(d)))
    assert off.data_ptr() % 8 == 4 and off.is_contiguous()
    for K, first, stop in ((G, 0, -1.0), (7, G - 1, -1.0), (G, G - 1, med)):
        assert MR.same(_launch(off, G, K, first=first, stop=stop), MR.maxmin(d, K, first=first, stop=stop))


def test_no_conformers_is_no_launch():
    from agdiff_amd import _lib
    n = torch.full((1 + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    cover = torch.full((1 + TAIL,), FSENTINEL, dtype=torch.float32, device="cuda")
    ints = torch.full((TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    floats = torch.full((TAIL,), FSENTINEL, dtype=torch.float32, device="cuda")
    dist = torch.zeros(1, dtype=torch.float32, device="cuda")
    _lib.call("agdiff_maxmin_pick", dist, 0, 1, 0, -1.0, ints, floats, ints, floats, n, cover)
    assert n.cpu().tolist() == [0] + [SENTINEL] * TAIL and cover.cpu().tolist() == [0.0] + [FSENTINEL] * TAIL
    assert (ints == SENTINEL).all() and (floats == FSENTINEL).all()


def test_more_conformers_than_the_limit_are_refused_before_any_launch():
    from agdiff_amd import _lib
    from agdiff_amd.picks import maxmin_pick, pick_conformers
    G = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1
    assert G == 4097
    with pytest.raises(_lib.AgdiffLimitError):
        maxmin_pick(torch.zeros((G, G), dtype=torch.float32, device="cuda"), G, 10)
    with pytest.raises(_lib.AgdiffLimitError):
        pick_conformers({"atom_type": np.array([6, 6]), "pos_gen": np.zeros((G, 2, 3), np.float32)}, k=10)
    with pytest.raises(ValueError):
        maxmin_pick(torch.zeros((4, 5), dtype=torch.float32, device="cuda"), 4, 2)
    with pytest.raises(ValueError):
        maxmin_pick(torch.zeros((4, 4), dtype=torch.float64, device="cuda"), 4, 2)
    with pytest.raises(_lib.AgdiffHipError):
        maxmin_pick(torch.zeros((4, 4), dtype=torch.float32, device="cuda"), 4, 5)       # K > G


# ------------------------------------------------------------------------------------------------ 6. end to end
def _check_result(res, want, G, n_atoms, sel=None):
    """a pick_conformers result against the restatement run on the matrix of the usable conformers (`sel`: their indices in the item)"""
    picks, radius, owner, near, n, cover = want
    sel = np.arange(G) if sel is None else np.asarray(sel)
    for key, dtype, shape in (("picks", torch.int32, (n,)), ("radius", torch.float32, (n,)), ("owner", torch.int32, (G,)),
                              ("near", torch.float32, (G,)), ("count", torch.int32, (n,)), ("pos", torch.float32, (n, n_atoms, 3))):
        assert res[key].dtype == dtype and tuple(res[key].shape) == shape and res[key].is_cuda, key
    assert isinstance(res["cover"], float) and F32(res["cover"]) == cover
    assert res["picks"].cpu().tolist() == sel[picks[:n]].tolist()
    assert MR.same((res["radius"].cpu().numpy(),), (radius[:n],))
    full_owner, full_near = np.full(G, -1, dtype=np.int32), np.full(G, np.nan, dtype=F32)
    full_owner[sel], full_near[sel] = owner, near
    assert MR.same((res["owner"].cpu().numpy(), res["near"].cpu().numpy()), (full_owner, full_near))
    assert res["count"].cpu().tolist() == np.bincount(owner[owner >= 0], minlength=n).tolist()
    assert int(res["count"].sum()) == int((owner >= 0).sum())


@pytest.mark.parametrize("n,K,G", [(20, 4, 37), (45, 7, 150)])
def test_rmsd_picks_equal_the_restatement_on_the_devices_matrix(n, K, G):
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.picks import pick_conformers
    item, label, gen, heavy = _families(n, K, G)
    matrix = self_rmsd_matrix(item).cpu().numpy()
    for k, radius, first in ((K, None, None), (G + 10, None, 3), (None, 0.5, None), (3, 0.5, G - 1), (G, 5.0, 1)):
        want = MR.maxmin(matrix, G if k is None else min(k, G), first=first or 0, stop=-1.0 if radius is None else radius)
        res = pick_conformers(item, k=k, radius=radius, first=first, align=False)
        _check_result(res, want, G, n)
        assert torch.equal(res["pos"].cpu(), torch.from_numpy(gen[want[0][:want[4]]]))
    # the families are tight (0.03 Angstrom of noise) and far apart: K picks are one per family, and a radius of 0.5 asks for as many
    res = pick_conformers(item, k=K, align=True)
    picks = res["picks"].cpu().numpy()
    assert sorted(label[picks].tolist()) == list(range(K)) and res["cover"] < 0.5 < float(res["radius"].min())
    assert np.array_equal(label[picks][res["owner"].cpu().numpy()], label)
    assert res["count"].cpu().tolist() == [int((label == label[p]).sum()) for p in picks]
    assert pick_conformers(item, radius=0.5, align=False)["picks"].cpu().tolist() == picks.tolist()
    # align: pick 0 bit for bit, the others on it within the bar of agdiff_align_conformers
    assert torch.equal(res["pos"][0].cpu(), torch.from_numpy(gen[picks[0]]))
    want = np.stack([_kabsch_align(gen[p], gen[picks[0]], heavy) for p in picks])
    dev = np.abs(res["pos"].cpu().numpy() - want).max()
    print("aligned picks n=%d: max |aligned - float64 Kabsch| = %.3e Angstrom" % (n, dev))
    assert dev <= ALIGN_ATOL


def test_valid_mask_and_broken_coordinates_keep_the_items_own_indices():
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.picks import pick_conformers
    n, K, G = 20, 4, 37
    item, label, gen, heavy = _families(n, K, G)
    valid = np.ones(G, dtype=bool)
    valid[label == 2] = False                                # one whole family ...
    valid[[0, 5]] = False                                    # ... and the conformer that would have been pick 0
    sel = np.nonzero(valid)[0]
    matrix = self_rmsd_matrix(dict(item, pos_gen=gen[sel])).cpu().numpy()
    for mask in (valid, torch.from_numpy(valid).cuda()):
        for k, first in ((3, None), (G, None), (5, int(sel[-1])), (2, int(sel[4]))):
            want = MR.maxmin(matrix, min(k, sel.size), first=0 if first is None else int(np.searchsorted(sel, first)))
            res = pick_conformers(item, k=k, first=first, valid=mask, align=False)
            _check_result(res, want, G, n, sel=sel)
            assert np.array_equal(res["owner"].cpu().numpy() == -1, ~valid) and res["picks"][0] == (sel[0] if first is None else first)
    res = pick_conformers(item, k=3, valid=valid)
    assert sorted(label[res["picks"].cpu().numpy()].tolist()) == [0, 1, 3]
    with pytest.raises(ValueError):
        pick_conformers(item, k=3, first=0, valid=valid)
    # a conformer with a coordinate that is not finite is masked before the matrix is made: the same result as with the mask
    broken = gen.copy()
    broken[0, 3, 1], broken[5, 0, 0] = np.nan, np.inf
    for c in np.nonzero(label == 2)[0]:
        broken[c, -1, 2] = -np.inf
    got = pick_conformers(dict(item, pos_gen=broken), k=G, align=False)
    _check_result(got, MR.maxmin(matrix, sel.size), G, n, sel=sel)
    assert torch.equal(got["pos"].cpu(), torch.from_numpy(gen[got["picks"].cpu().numpy()]))
    with pytest.raises(ValueError):
        pick_conformers(dict(item, pos_gen=broken), k=3, first=5)
    none = pick_conformers(item, k=3, valid=np.zeros(G, dtype=bool))
    assert all(tuple(none[k].shape) == (0,) for k in ("picks", "radius", "count")) and tuple(none["pos"].shape) == (0, n, 3)
    assert (none["owner"] == -1).all() and bool(torch.isnan(none["near"]).all()) and none["cover"] == 0.0
    assert none["owner"].shape == (G,) and none["near"].shape == (G,)
    assert none["picks"].dtype == torch.int32 and none["radius"].dtype == torch.float32 and none["count"].dtype == torch.int32


def test_tfd_picks_equal_the_restatement_on_the_devices_matrix():
    """pentane rotamers (the construction of tests/test_hip_clusters.py) by TFD, and a six-ring's chairs, boats and twist-boats by
    the TFD with ring terms (tests/test_hip_rings.py)"""
    from agdiff_amd.picks import pick_conformers
    from agdiff_amd.torsions import tfd_self
    rng = np.random.default_rng(17)
    g = np.pi / 3
    rotamers, sizes = [(np.pi, np.pi), (np.pi, g), (g, g), (-g, -g)], [9, 6, 4, 2]
    label = rng.permutation(np.repeat(np.arange(4), sizes))
    gen = np.stack([_moved(rng, TR.chain_positions(np.array(rotamers[c]) + 0.03 * rng.normal(size=2))) for c in label]).astype(F32)
    at, bi, bt = TR.alkane(5)
    item = dict(atom_type=at, bond_index=bi, bond_type=bt, pos_gen=gen)
    G = label.shape[0]
    matrix = tfd_self(item)[0].cpu().numpy()
    for k, radius, first in ((4, None, None), (G, None, 7), (None, 0.1, None), (G, 0.02, G - 1)):
        want = MR.maxmin(matrix, G if k is None else k, first=first or 0, stop=-1.0 if radius is None else radius)
        _check_result(pick_conformers(item, k=k, radius=radius, metric="tfd", first=first, align=False), want, G, 5)
    res = pick_conformers(item, k=4, metric="tfd", align=True)
    picks = res["picks"].cpu().numpy()
    assert sorted(label[picks].tolist()) == [0, 1, 2, 3] and res["cover"] < 0.1
    assert torch.equal(res["pos"][0].cpu(), torch.from_numpy(gen[picks[0]]))
    want = np.stack([_kabsch_align(gen[p], gen[picks[0]], np.arange(5)) for p in picks])
    assert np.abs(res["pos"].cpu().numpy() - want).max() <= ALIGN_ATOL
    # the ring as a term: without it a six-ring has no torsion at all and every TFD is 0 -- one pick covers everything
    pos = np.stack([RR.chair()] * 5 + [RR.boat()] * 5 + [RR.twist_boat()] * 5)
    ring = (pos + 0.01 * np.random.default_rng(6).normal(size=pos.shape)).astype(F32)
    at, bi, bt = TR.cyclohexane()
    item = dict(atom_type=at, bond_index=bi, bond_type=bt, pos_gen=ring)
    matrix = tfd_self(item, rings=True)[0].cpu().numpy()
    for k, radius in ((3, None), (15, None), (None, 0.2)):
        want = MR.maxmin(matrix, 15 if k is None else k, stop=-1.0 if radius is None else radius)
        _check_result(pick_conformers(item, k=k, radius=radius, metric="tfd", tfd_rings=True, align=False), want, 15, 6)
    two = pick_conformers(item, radius=0.2, metric="tfd", tfd_rings=True, align=False)
    assert two["picks"].shape[0] >= 2 and two["picks"][0] == 0 and int(two["picks"][1]) >= 5 and two["cover"] <= 0.2   # a chair, then a boat
    flat = pick_conformers(item, radius=0.2, metric="tfd", align=False)
    assert flat["picks"].cpu().tolist() == [0] and flat["cover"] == 0.0 and flat["count"].tolist() == [15]


def test_five_tight_groups_give_one_pick_each():
    """Five groups of conformers whose gap (the smallest distance between two groups) exceeds twice the spread (the largest distance
    within one).  Then the rule alone gives: while a group has no pick, its members are farther from every pick than any member
    of a group that has one, so the first five picks are one per group; every conformer is owned by its group's pick, nearer
    than the gap against farther than it; and the cover is a distance within a group.  No tolerance is involved."""
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.picks import pick_conformers
    n, sizes = 20, [9, 7, 6, 5, 4]
    rng = np.random.default_rng(55)
    at = np.where(rng.random(n) < 0.5, 1, rng.choice([6, 7, 8], size=n))
    at[:4] = 6
    heavy = np.nonzero(at != 1)[0]
    perms = GROUP4(heavy.size)
    centres = [rng.normal(size=(n, 3)) * 1.5 for _ in sizes]
    label = rng.permutation(np.repeat(np.arange(5), sizes))
    G = label.shape[0]
    gen = np.stack([_moved(rng, _relabel(centres[c] + 0.03 * rng.normal(size=(n, 3)), heavy, perms[rng.integers(4)]))
                    for c in label]).astype(F32)
    item = {"atom_type": at, "pos_gen": gen, "perms": perms}
    matrix = self_rmsd_matrix(item).cpu().numpy()
    same = label[:, None] == label[None, :]
    spread, gap = float(matrix[same].max()), float(matrix[~same].min())
    print("five groups: spread %.4f, gap %.4f Angstrom" % (spread, gap))
    assert gap > 2 * spread                                  # the premise, on the matrix the device produced
    for first in (0, G - 1, int(np.nonzero(label == 4)[0][0])):
        want = MR.maxmin(matrix, 5, first=first)             # on the CPU first ...
        res = pick_conformers(item, k=5, first=first, align=False)
        _check_result(res, want, G, n)                       # ... and the device gives the same
        for picks, owner, cover in ((want[0], want[2], float(want[5])),
                                    (res["picks"].cpu().numpy(), res["owner"].cpu().numpy(), res["cover"])):
            assert sorted(label[picks].tolist()) == [0, 1, 2, 3, 4]
            assert np.array_equal(label[picks][owner], label)
            assert cover <= spread < gap


# ------------------------------------------------------------------------------------------------ 7. the command line
def test_command_line_writes_every_key(tmp_path, capsys):
    from agdiff_amd import driver, picks, synth
    rng = np.random.default_rng(9)
    at, bonds, gen7, thr = seven_pattern_conformers(rng)
    _, bi, bt = TR.graph(at, bonds)
    mols, gens = [dict(atom_type=at, edge_index=bi, edge_type=bt, num_refs=4, name="seven")], [gen7]
    for i, (n, G) in enumerate(((15, 7), (12, 5))):
        a, r, c, ty = synth.random_molecule(rng, n)
        mols.append(dict(atom_type=a, edge_index=np.stack([r, c]), edge_type=ty, num_refs=3, name="m%d" % (i + 1)))
        base = rng.normal(size=(2, n, 3)) * 1.5
        gens.append(np.stack([_moved(rng, base[k % 2] + 0.02 * rng.normal(size=(n, 3))) for k in range(G)]).astype(F32))
    driver.save_testset(str(tmp_path / "test.npz"), mols)
    np.savez(str(tmp_path / "samples_all.npz"), **{"pos_gen_%d" % i: g for i, g in enumerate(gens)})
    base = ["--samples", str(tmp_path / "samples_all.npz"), "--testset", str(tmp_path / "test.npz")]
    out = picks.main(base + ["--count", "3", "--align", "--out", str(tmp_path / "picks.npz")])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and "picked 9 of 19 conformers" in line[0] and "RMSD" in line[0]
    z = np.load(str(tmp_path / "picks.npz"))
    keys = ("pick", "radius", "owner", "near", "count", "cover", "pos", "name")
    assert set(z.files) == {"%s_%d" % (k, i) for k in keys for i in range(3)} == set(out)
    for i, g in enumerate(gens):
        G, n = g.shape[0], g.shape[1]
        for k, dtype, shape in (("pick", np.int32, (3,)), ("radius", np.float32, (3,)), ("owner", np.int32, (G,)),
                                ("near", np.float32, (G,)), ("count", np.int32, (3,)), ("cover", np.float32, ()),
                                ("pos", np.float32, (3, n, 3))):
            assert z["%s_%d" % (k, i)].dtype == dtype and z["%s_%d" % (k, i)].shape == shape, (k, i)
            assert np.array_equal(z["%s_%d" % (k, i)], out["%s_%d" % (k, i)], equal_nan=True)
        assert str(z["name_%d" % i]) == mols[i]["name"]
        assert z["pick_%d" % i][0] == 0 and z["radius_%d" % i][0] == np.inf and np.array_equal(z["pos_%d" % i][0], g[0])
        assert np.array_equal(z["owner_%d" % i][z["pick_%d" % i]], np.arange(3)) and z["count_%d" % i].sum() == G
        assert (z["near_%d" % i] <= z["cover_%d" % i]).all() and z["cover_%d" % i] <= z["radius_%d" % i][-1]
    # molecules 1 and 2 are two tight families each, the even and the odd conformers: the second pick is of the other family, and
    # after it nothing is far
    assert z["pick_1"][1] % 2 == 1 and z["pick_2"][1] % 2 == 1 and z["radius_1"][2] < 0.2 < z["radius_1"][1]
    # --radius: two picks cover those; --first moves pick 0
    moved = picks.main(base + ["--radius", "0.2", "--first", "1", "--out", str(tmp_path / "moved.npz")])
    assert "until within 0.200" in capsys.readouterr().out
    for i in (1, 2):
        assert moved["pick_%d" % i].shape == (2,) and moved["pick_%d" % i][0] == 1 and moved["pick_%d" % i][1] % 2 == 0
        assert moved["cover_%d" % i] <= 0.2 < moved["radius_%d" % i][1]
    # --drop-invalid writes valid_<i> next to the rest
    more = picks.main(base + ["--radius", "0.2", "--drop-invalid", "--out", str(tmp_path / "checked.npz")])
    capsys.readouterr()
    assert all("valid_%d" % i in more and more["valid_%d" % i].dtype == np.int8 for i in range(3))
    for i in range(3):
        assert np.array_equal(more["owner_%d" % i] == -1, more["valid_%d" % i] == 0)
        assert more["cover_%d" % i] <= 0.2
    tfd = picks.main(base + ["--count", "2", "--tfd", "--out", str(tmp_path / "tfd.npz")])
    assert tfd["pick_0"].shape == (2,) and tfd["pick_0"].dtype == np.int32 and "TFD" in capsys.readouterr().out
