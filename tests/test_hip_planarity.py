"""GPU (MI355X): the planarity check (agdiff_amd.planarity; csrc/eval.hip: k_planar_groups) against the float64 numpy restatement of
its definition (tests/planarity_ref.py, numpy.linalg.eigh), and through the prune, the driver and the command lines.

Gates, none taken from what the kernel gives:
  PR.GATE_REL, PR.GATE_ABS   4 x 2^-24 relative + 1e-9 Angstrom absolute on dev and worst.  Kernel and reference both compute in fp64
            from the same fp32 coordinates; they differ by the final fp32 store (half an ulp, 2^-24 relative) and by the eigen solver
            (cyclic Jacobi against LAPACK).  With |x| < 16 (asserted) the covariance A has entries of a few Angstrom^2, and both
            solvers return the eigenvectors of a matrix within ~2^-52 |A| of it; at a gap g = lambda_mid - lambda_min >= 1e-3
            Angstrom^2 that turns the normal by ~|A| 2^-52 / g ~ 1e-12 rad, which moves the distance of a member a few Angstrom from
            the centroid by ~1e-11 Angstrom: a hundredth of the absolute term.  (A CPU trial of the Jacobi sweeps against LAPACK over
            20,000 groups of 4 .. 8 atoms gave 6.9e-15 Angstrom at worst, while sqrt(lambda_min) differed by 3.8e-8 Angstrom on exactly
            planar groups: that is why dev is defined through the projections and not through the eigenvalue.)
  PR.MIN_GAP  entries whose gap is below 1e-3 Angstrom^2 (three atoms nearly on a line, say) have no normal worth comparing: their values are
            left out, at most 1 % of a case's entries and none in the hand-built inputs, and worst / worst_group / n_bent are
            compared on the conformers without such an entry.  There they must be equal exactly.
  PR.MARGIN for exact counts and indices to be a fair demand the reference asserts on its own output, before the kernel is asked
            anything, that no dev lies within 1e-5 (relative) of the threshold and that a conformer's best and second-best dev are
            that far apart.  The seeds (PR.case) were chosen on the CPU so that it holds.
  move      after a rigid motion done in fp64 and rounded to fp32 again: every coordinate stays below 16 in magnitude (asserted), where
            fp32's spacing is at most 2^-20, so rounding moves a coordinate by at most 2^-21 and an atom by at most d = sqrt(3) 2^-21 =
            8.3e-7 Angstrom; a centred member y_k moves by e_k, |e_k| <= d' = 2 d (the atom and the centroid).  A = (1/m) sum y y^T then
            moves by E, |E| <= 2 r d' + d'^2 with r = max |y_k|; the normal turns by an angle with sin <= 2 |E| / g (Davis-Kahan in Yu,
            Wang and Samworth's form), so |n' - n| <= 2 sin, and a projection n . y_k moves by at most |e_k| + r |n' - n|:
                move(r, g) = d' + 4 r (2 r d' + d'^2) / g          per entry, from the reference's own r (+ d') and g
            That test asserts margins of 4 x move to the threshold and between a conformer's two largest in the reference first, so
            that counts and indices cannot move."""
import glob

import numpy as np
import pytest
import torch

import planarity_ref as PR
from agdiff_amd import _lib

pytestmark = pytest.mark.gpu
THRESH = PR.THRESH


def _gpu(pos):
    return torch.from_numpy(np.array(pos, dtype=np.float32)).cuda()        # (a copy: the cached cases are read-only)


def _item(mol, **kw):
    at, ei, et = mol
    return dict(atom_type=at, edge_index=ei, edge_type=et, **kw)


def _run(pos, ptr, idx, thresh=THRESH, want_dev=True):
    from agdiff_amd.planarity import planar_deviation
    return planar_deviation(_gpu(pos), ptr, idx, thresh, want_dev=want_dev)


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("n,G,P", PR.CASES)
def test_kernel_matches_the_float64_reference(n, G, P):
    (pos, ptr, idx, shape), ref = PR.case(n, G, P)
    got = _run(pos, ptr, idx)
    w, wg, nb, d = (x.cpu().numpy() for x in got)
    assert w.dtype == d.dtype == np.float32 and wg.dtype == nb.dtype == np.int32
    assert w.shape == wg.shape == nb.shape == (G,) and d.shape == (G, P)
    out = PR.left_out(ref)
    steady = ~out.any(1)
    assert out.sum() <= 0.01 * G * P and steady.any()
    if P:
        err = np.abs(d.astype(np.float64) - ref["dev"])
        print("n = %d, G = %d, P = %d: %d of %d entries left out; largest difference of dev %.3e A (relative %.3e), of worst %.3e A" % (
            n, G, P, out.sum(), out.size, err[~out].max(), (err / np.maximum(ref["dev"], 1e-30))[~out & (ref["dev"] > 1e-3)].max(initial=0.0),
            np.abs(w.astype(np.float64) - ref["worst"])[steady].max()))
    assert PR.close(np.where(out, 0.0, d), np.where(out, 0.0, ref["dev"]))
    assert PR.close(w[steady], ref["worst"][steady])
    assert np.array_equal(wg[steady], ref["worst_group"][steady]) and np.array_equal(nb[steady], ref["n_bent"][steady])
    # worst is the maximum of the fp32 values as stored
    assert P == 0 or np.array_equal(w, d.max(1))
    if P == 0:
        assert not w.any() and (wg == -1).all() and not nb.any()
    # without dev the three results are the same bits; so are a second call's
    bare = _run(pos, ptr, idx, want_dev=False)
    assert bare[3] is None and all(torch.equal(a, b) for a, b in zip(bare[:3], got[:3]))
    again = _run(pos, ptr, idx)
    assert all(torch.equal(a, b) for a, b in zip(again, got))


def _squares():
    """float32 [2, 12, 3]: three exact squares, 0.25 (atoms 0 .. 3), 0.5 (4 .. 7) and 0.75 (8 .. 11) from their best planes"""
    pos = np.concatenate([PR.square(0.25), PR.square(0.5, (4, 0, 0)), PR.square(0.75, (0, 4, 2))])
    return np.stack([pos, pos]).astype(np.float32)


def test_equal_deviations_take_the_lowest_group():
    pos, P = _squares(), 140
    low, mid, high = np.arange(4), np.arange(4, 8), np.arange(8, 12)
    groups = [low] * P
    for k in (70, 67, 3, 131):                                           # 0.5: in lanes 6, 3, 3, 3
        groups[k] = mid
    ptr = np.arange(P + 1, dtype=np.int32) * 4
    table = lambda: np.concatenate(groups).astype(np.int32)
    ref = PR.planar(pos, ptr, table(), 0.375)
    PR.assert_margins(ref, pos, 0.375, ties=True)
    assert not PR.left_out(ref).any()
    assert ref["worst"].tolist() == [0.5, 0.5] and ref["worst_group"].tolist() == [3, 3] and ref["n_bent"].tolist() == [4, 4]
    w, wg, nb, d = _run(pos, ptr, table(), 0.375)
    assert np.array_equal(d.cpu().numpy(), ref["dev"])                   # (exact on both sides: small binary fractions)
    assert w.tolist() == [0.5, 0.5] and wg.tolist() == [3, 3] and nb.tolist() == [4, 4]
    groups[3] = low
    assert _run(pos, ptr, table(), 0.375)[1].tolist() == [67, 67]
    groups[67] = low
    assert _run(pos, ptr, table(), 0.375)[1].tolist() == [70, 70]
    groups[130] = high                                                   # 0.75 beats them all
    w, wg, nb, _ = _run(pos, ptr, table(), 0.375)
    assert w.tolist() == [0.75, 0.75] and wg.tolist() == [130, 130] and nb.tolist() == [3, 3]
    # the comparison is dev > thresh on the fp32 values: a group exactly at the threshold is not bent
    assert _run(pos, ptr, table(), 0.5)[2].tolist() == [1, 1] and _run(pos, ptr, table(), 0.0)[2].tolist() == [P, P]


def test_a_coordinate_that_is_not_finite_is_an_infinite_deviation_and_leaves_the_others_alone():
    from agdiff_amd.planarity import check_planarity
    (pos, ptr, idx, shape), ref = PR.case(61, 10, 65)
    broken = np.array(pos[:4])
    a, b = int(idx[ptr[9]]), int(idx[ptr[64] + 2])                       # a member of group 9 and one of group 64
    broken[2, a, 1] = np.nan
    broken[2, b, 0] = np.inf
    want = PR.planar(broken, ptr, idx, THRESH)
    hit = np.isposinf(want["dev"][2])
    assert hit[9] and hit[64] and not hit.all() and np.isposinf(want["worst"][2]) and want["worst_group"][2] == np.nonzero(hit)[0][0]
    got = _run(broken, ptr, idx)
    base = _run(pos[:4], ptr, idx)
    w, wg, nb, d = (x.cpu().numpy() for x in got)
    assert np.array_equal(np.isposinf(d[2]), hit) and np.isposinf(w[2]) and wg[2] == want["worst_group"][2] and nb[2] == want["n_bent"][2]
    assert nb[2] >= hit.sum()
    others = [0, 1, 3]
    assert all(torch.equal(x[others], y[others]) for x, y in zip(got, base))
    keep = ~hit
    assert torch.equal(got[3][2][torch.from_numpy(keep)], base[3][2][torch.from_numpy(keep)])
    res = check_planarity(dict(atom_type=np.full(61, 6), pos_gen=broken, bond_index=np.zeros((2, 0), np.int64), bond_type=np.zeros(0, np.int64)),
                          groups=(ptr, idx))
    assert res["flat"][2].item() is False and np.isposinf(res["flat_dev"][2].item()) and (res["groups"][2] == -1).all()


def test_a_group_the_host_would_refuse_is_nan_takes_no_part_and_reads_nothing():
    """the wrappers refuse such tables (check_groups); the entry point itself answers NaN for them"""
    pos = _squares()
    G, n = pos.shape[0], pos.shape[1]
    sets = [[4, 5, 6, 7], [0, 1], [0, 1, 2, 12 + 10 ** 8], list(range(9)), [0, 1, 2, 3], [-1, 1, 2, 3]]      # (400 MB past the tensor if read)
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    idx = np.concatenate(sets).astype(np.int32)
    want = PR.planar(pos, ptr, idx, 0.3)
    assert np.isnan(want["dev"][0]).tolist() == [False, True, True, True, False, True] and want["worst_group"].tolist() == [0, 0]

    def call(ptr, idx, P):
        t = _gpu(pos)
        dev = torch.empty((G, P), dtype=torch.float32, device="cuda")
        worst = torch.empty(G, dtype=torch.float32, device="cuda")
        group, bent = (torch.empty(G, dtype=torch.int32, device="cuda") for _ in range(2))
        _lib.call("agdiff_planar_groups", t, torch.from_numpy(ptr).cuda(), torch.from_numpy(idx).cuda(), G, n, P, 0.3, dev, worst, group, bent)
        return dev.cpu().numpy(), worst.tolist(), group.tolist(), bent.tolist()
    d, w, g, b = call(ptr, idx, 6)
    assert np.array_equal(d, want["dev"], equal_nan=True) and d[0].tolist()[0::4] == [0.5, 0.25]
    assert (w, g, b) == ([0.5, 0.5], [0, 0], [1, 1])
    # every group NaN: (0, -1, 0)
    d, w, g, b = call(ptr[1:4] - ptr[1], idx[ptr[1]:ptr[3]], 2)
    assert np.isnan(d).all() and (w, g, b) == ([0.0, 0.0], [-1, -1], [0, 0])


def test_no_groups_is_flat():
    from agdiff_amd.planarity import check_planarity, planar_deviation
    w, wg, nb, d = planar_deviation(_gpu(np.zeros((3, 5, 3))), np.zeros(1, np.int32), np.zeros(0, np.int32), want_dev=True)
    assert (w.tolist(), wg.tolist(), nb.tolist()) == ([0.0] * 3, [-1] * 3, [0] * 3) and d.shape == (3, 0)
    chain = PR.graph([6] * 4, [(0, 1, 1), (1, 2, 1), (2, 3, 1)])
    res = check_planarity(_item(chain, pos_gen=np.random.default_rng(0).normal(size=(2, 4, 3))), want_dev=True)
    assert res["flat"].tolist() == [True, True] and res["flat"].dtype == torch.bool and res["flat_group"].tolist() == [-1, -1]
    assert res["flat_dev"].tolist() == [0.0, 0.0] and res["dev"].shape == (2, 0) and res["groups"][0].tolist() == [0]
    none = planar_deviation(torch.zeros((0, 5, 3), device="cuda"), [0, 3], [0, 1, 2])
    assert none[0].shape == none[1].shape == none[2].shape == (0,)


def test_a_rigid_motion_keeps_counts_and_indices_and_moves_dev_by_rounding_only():
    (pos, ptr, idx, shape), ref = PR.case(23, 33, 5)
    assert not PR.left_out(ref).any()
    d1 = 2 * np.sqrt(3.0) * 2.0 ** -21
    r = ref["radius"] + d1
    move = d1 + 4 * r * (2 * r * d1 + d1 * d1) / ref["gap"]
    dev = ref["dev"].astype(np.float64)
    assert (np.abs(dev - np.float32(THRESH)) > 4 * move).all()
    order = np.argsort(dev, axis=1)[:, -2:]
    top, top_move = np.take_along_axis(dev, order, 1), np.take_along_axis(move, order, 1)
    assert (top[:, 1] - top[:, 0] > 4 * top_move.sum(1)).all()
    rng = np.random.default_rng(11)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    moved = (pos.astype(np.float64) @ q.T + np.array([1.5, -2.0, 0.7])).astype(np.float32)
    assert np.abs(moved).max() < 16 and np.abs(pos).max() < 16
    w, wg, nb, d = (x.cpu().numpy() for x in _run(moved, ptr, idx))
    assert np.array_equal(wg, ref["worst_group"]) and np.array_equal(nb, ref["n_bent"])
    diff = np.abs(d.astype(np.float64) - dev)
    print("largest move of dev under a rigid motion: %.3e A (bound %.3e there; largest bound %.3e)" % (
        diff.max(), move.reshape(-1)[diff.argmax()], move.max()))
    assert (diff <= move + PR.GATE_REL * dev + PR.GATE_ABS).all()


# ------------------------------------------------------------------------------------------------ 2. a molecule
def test_styrene_bent_ring_and_twisted_double_bond_pass_the_distance_checks_and_fail_this_one():
    from agdiff_amd.ensemble import prune_conformers
    from agdiff_amd.planarity import check_planarity
    from agdiff_amd.validity import check_geometry
    mol, gen = PR.styrene_conformers()
    item = _item(mol, pos_gen=gen)
    res = check_planarity(item, want_dev=True)
    ptr, idx, kind = res["groups"]
    assert PR.groups_of(ptr, idx, kind) == [(0, [0, 1, 2, 3, 4, 5]), (1, [0, 6, 7, 13, 14, 15])]
    ref = PR.planar(gen, ptr, idx, 0.25)
    assert res["flat"].dtype == torch.bool and res["flat_dev"].dtype == torch.float32
    assert res["flat_group"].dtype == res["n_bent"].dtype == torch.int32
    assert res["flat"].tolist() == [True, False, False, True] and res["n_bent"].tolist() == [0, 1, 1, 0]
    assert res["flat_group"][1:3].tolist() == [0, 1] and kind[res["flat_group"][1:3].cpu().numpy()].tolist() == [0, 1]
    assert PR.close(res["dev"].cpu().numpy(), ref["dev"]) and PR.close(res["flat_dev"].cpu().numpy(), ref["worst"])
    print("styrene: dev per (conformer, group) %s" % np.round(res["dev"].cpu().numpy(), 4).tolist())
    # the point of the feature: the distance checks call all four valid
    geo = check_geometry(item)
    assert geo["valid"].tolist() == [True] * 4 and geo["n_bad"].tolist() == [0] * 4 and geo["n_clash"].tolist() == [0] * 4
    # a looser threshold, and a caller's own groups (the ring alone, no kinds)
    assert check_planarity(item, thresh=0.35)["flat"].tolist() == [True, True, False, True]
    own = check_planarity(item, groups=(ptr[:2], idx[:6]))
    assert own["flat"].tolist() == [True, False, True, True] and own["groups"][2].tolist() == [-1]
    # the prune: the bent ring is far from everything kept and becomes a cluster; with the mask both leave the walk
    blind = prune_conformers(item, 0.1, align=False)
    assert 1 in blind["kept"].tolist() and (blind["leader"] >= 0).all()
    for mask in (res["flat"], res["flat"].cpu().numpy()):
        kept = prune_conformers(item, 0.1, align=False, valid=mask)
        assert kept["kept"].tolist() == [0] and kept["leader"].tolist() == [0, -1, -1, 0]


def test_command_lines_write_the_arrays(tmp_path, capsys):
    from agdiff_amd import driver, ensemble, planarity
    mol, gen = PR.styrene_conformers()
    chain = PR.graph([6] * 4, [(0, 1, 1), (1, 2, 1), (2, 3, 1)])
    mols = [dict(atom_type=mol[0], edge_index=mol[1], edge_type=mol[2], num_refs=2, name="styrene", index=0),
            dict(atom_type=chain[0], edge_index=chain[1], edge_type=chain[2], num_refs=1, name="butane", index=1)]
    test, samples = str(tmp_path / "test.npz"), str(tmp_path / "samples.npz")
    driver.save_testset(test, mols)
    butane = np.random.default_rng(3).normal(size=(2, 4, 3)).astype(np.float32)
    np.savez(samples, pos_gen_0=gen, name_0=np.str_("styrene"), pos_gen_1=butane, name_1=np.str_("butane"))
    out = planarity.main(["--samples", samples, "--testset", test, "--out", str(tmp_path / "flat.npz")])
    assert "2 molecules, 6 conformers, 2 bent (1 with an aromatic ring out of plane, 1 with a double bond out of plane)" in capsys.readouterr().out
    z = np.load(str(tmp_path / "flat.npz"))
    assert set(z.files) == {"%s_%d" % (k, i) for k in ("flat", "flat_dev", "flat_group", "n_bent", "name") for i in (0, 1)}
    assert z["flat_0"].dtype == np.int8 and z["flat_dev_0"].dtype == np.float32 and z["flat_group_0"].dtype == z["n_bent_0"].dtype == np.int32
    assert z["flat_0"].tolist() == [1, 0, 0, 1] and z["n_bent_0"].tolist() == [0, 1, 1, 0] and z["flat_group_0"][1:3].tolist() == [0, 1]
    assert z["flat_1"].tolist() == [1, 1] and z["flat_group_1"].tolist() == [-1, -1] and str(z["name_0"]) == "styrene"
    assert all(np.array_equal(out[k], z[k]) for k in z.files)
    planarity.main(["--samples", samples, "--testset", test, "--out", str(tmp_path / "groups.npz"), "--per-group", "--thresh", "0.35"])
    assert "1 bent (0 with an aromatic ring out of plane, 1 with" in capsys.readouterr().out
    g = np.load(str(tmp_path / "groups.npz"))
    assert set(g.files) == set(z.files) | {"%s_%d" % (k, i) for k in ("planar_dev", "planar_ptr", "planar_idx", "planar_kind") for i in (0, 1)}
    assert g["planar_dev_0"].shape == (4, 2) and g["planar_dev_1"].shape == (2, 0) and g["planar_kind_0"].tolist() == [0, 1]
    assert g["planar_ptr_0"].tolist() == [0, 6, 12] and g["planar_idx_0"].tolist() == [0, 1, 2, 3, 4, 5, 0, 6, 7, 13, 14, 15]
    assert np.array_equal(g["planar_dev_0"].max(1), z["flat_dev_0"]) and g["flat_0"].tolist() == [1, 1, 0, 1]
    # the prune of a finished job
    pruned = ensemble.main(["--samples", samples, "--testset", test, "--prune-rms", "0.1", "--drop-bent", "--out", str(tmp_path / "pruned.npz")])
    assert np.array_equal(pruned["flat_0"], z["flat_0"]) and pruned["flat_0"].dtype == np.int8 and "valid_0" not in pruned
    assert pruned["cluster_0"].tolist() == [0, -1, -1, 0] and pruned["kept_0"].tolist() == [0]
    both = ensemble.main(["--samples", samples, "--testset", test, "--prune-rms", "0.1", "--drop-bent", "--drop-invalid",
                          "--out", str(tmp_path / "both.npz")])
    assert np.array_equal(both["cluster_0"] == -1, (both["flat_0"] == 0) | (both["valid_0"] == 0))
    plain = ensemble.main(["--samples", samples, "--testset", test, "--prune-rms", "0.1", "--out", str(tmp_path / "plain.npz")])
    assert "flat_0" not in plain and (plain["cluster_0"] >= 0).all()


def test_run_job_saves_the_verdicts_with_the_switch_and_nothing_new_without_it(tmp_path):
    from agdiff_amd import driver, get_model, qm9_model_config, synth
    from agdiff_amd.planarity import check_planarity, planar_groups
    m = get_model(qm9_model_config(num_diffusion_timesteps=8))
    m.load_state_dict(synth.synth_state_dict(m.state_dict()))
    m = m.to("cuda:0").eval()
    at, r, c, ty = synth.random_molecule(np.random.default_rng(9), 13)       # (seed 9: a molecule with two double-bond groups)
    mols = [dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=ty, num_refs=5, name="mol0", index=0)]
    confs = lambda num_refs: num_refs
    kw = dict(n_steps=4, step_lr=1e-6, w_global=1.0, clip=1000.0)
    logs = []
    job = lambda name, **sw: driver.run_job(m, mols, str(tmp_path / name), confs, 10 ** 6, kw, "cuda:0", log=logs.append, noise="counter",
                                            seed=7, **sw)
    item = lambda pos: dict(atom_type=at, pos_gen=pos, edge_index=mols[0]["edge_index"], edge_type=ty)
    assert planar_groups(item(None))[2].tolist() == [1, 1]
    res = job("checked", check_planarity=True)
    files = glob.glob(str(tmp_path / "checked" / "samples_[0-9]*.npz"))
    assert len(files) == 1 and sum("conformers are bent" in str(x) for x in logs) == 1
    for z in (res, np.load(files[0]), np.load(str(tmp_path / "checked" / "samples_all.npz"))):
        assert set(z.keys() if isinstance(z, dict) else z.files) == {"pos_gen_0", "name_0", "flat_0", "flat_dev_0"}
        assert z["flat_0"].dtype == np.int8 and z["flat_dev_0"].dtype == np.float32 and z["flat_0"].shape == z["flat_dev_0"].shape == (5,)
        want = check_planarity(item(z["pos_gen_0"]))
        assert np.array_equal(z["flat_0"], want["flat"].cpu().numpy().astype(np.int8))
        assert np.array_equal(z["flat_dev_0"], want["flat_dev"].cpu().numpy())
    print("run_job: flat %s, flat_dev %s" % (res["flat_0"].tolist(), np.round(res["flat_dev_0"], 3).tolist()))
    # without the switch: the keys and the bytes a job had before there was one (the same draws: --noise counter)
    plain = job("plain")
    assert set(plain.keys()) == {"pos_gen_0", "name_0"} and sum("conformers are bent" in str(x) for x in logs) == 1
    assert set(np.load(glob.glob(str(tmp_path / "plain" / "samples_[0-9]*.npz"))[0]).files) == {"pos_gen_0", "name_0"}
    assert plain["pos_gen_0"].tobytes() == res["pos_gen_0"].tobytes()
    # valid_<i> keeps its meaning bit for bit whatever the new switch says; with a prune the mask is flat & valid
    geo = job("geo", check_geometry=True, prune_rms=0.5)
    both = job("both", check_geometry=True, check_planarity=True, prune_rms=0.5)
    assert set(both.keys()) == set(geo.keys()) | {"flat_0", "flat_dev_0"}
    assert all(geo[k].tobytes() == both[k].tobytes() for k in ("pos_gen_0", "valid_0", "bond_dev_0", "clash_0"))
    assert np.array_equal(both["flat_0"], res["flat_0"]) and np.array_equal(both["flat_dev_0"], res["flat_dev_0"])
    assert np.array_equal(both["cluster_0"] == -1, (both["valid_0"] == 0) | (both["flat_0"] == 0))
    alone = job("alone", check_planarity=True, prune_rms=0.5)
    assert np.array_equal(alone["cluster_0"] == -1, alone["flat_0"] == 0) and "valid_0" not in alone
