"""GPU (MI355X): the flattening repair (agdiff_amd.planarity.relax_planar; csrc/eval.hip: k_relax_planar) against the float64 numpy
restatement of its rule (tests/flatten_ref.py), by properties that need no reference, and through repair_planarity, the driver and
the command line.

Gates, those of tests/test_hip_relax.py and none taken from what the kernel gives:
  status, iters   equal exactly.  The reference asserts on its own output, before the kernel is asked anything, that no quantity the
            stop rule compares (|s|, c, and now e) comes within 1e-6 (relative) of its threshold at any iteration, that no distance,
            ratio or dev lies within VR.MARGIN of the bound that decides status 0, and that every group's eigenvalue gap stays
            above 1e-3 A^2 at every iteration, so that both eigen solvers give one normal (flatten_ref.Margin otherwise).
  pos_out   4 x 2^-24 x (the largest |coordinate| of that conformer) per coordinate: the final fp32 store plus the fp64 rounding
            accumulated over the updates, which the reference measures on itself by summing every atom's terms in the opposite order
            and taking the normals from an SVD instead of eigh; that self-difference is asserted below a quarter of the gate.  The
            inputs are centred; every coordinate is asserted below 16.
  resid, moved    VR.GATE (4 x 2^-24) relative.
  status 1  pair_bounds + clash_scan call the output valid AND planar_deviation calls it flat at thresh: at exit every member is
            within flat_to + pad / 2 = 0.11 A of its plane against a threshold of 0.25, so this is an exact demand.
Properties on every case: status 0 and 3 come back bit for bit, two calls give the same bits, each conformer alone and the batch
in another order give the same bits.
The shapes: 16, 10 and 18 atoms (16 lanes per atom; one group of 4 atoms; two groups that share atoms), 144 atoms (one lane per
atom, the large instantiation, 18 groups), 320 atoms (atoms strided over the threads, 40 groups), 320 atoms with exactly
AGDIFF_FLATTEN_MAX_GROUPS groups, one group more, P = 0 and G = 0."""
import functools
import glob

import numpy as np
import pytest
import torch

import flatten_ref as FR
import relax_ref as RR
import validity_ref as VR

pytestmark = pytest.mark.gpu
POS_GATE = 4.0 * 2.0 ** -24


def _gpu(pos):
    return torch.from_numpy(np.array(pos, dtype=np.float32)).cuda()        # (a copy: the cached cases are read-only)


def _run(inputs, **kw):
    from agdiff_amd.planarity import relax_planar
    out = relax_planar(_gpu(inputs[0]), *inputs[1:], **kw)
    assert out[0].dtype == out[3].dtype == out[4].dtype == torch.float32 and out[1].dtype == out[2].dtype == torch.int32
    assert out[0].shape == inputs[0].shape and all(o.shape == (inputs[0].shape[0],) for o in out[1:])
    return out


def _judged(pos_gpu, inputs):
    """(valid bool [G], flat bool [G]): the three check kernels on pos_gpu, at the true bounds and at thresh"""
    from agdiff_amd.planarity import planar_deviation
    from agdiff_amd.validity import clash_scan, pair_bounds
    _, grp_ptr, grp_idx, pairs, lo, hi, radius, ex_ptr, ex_idx = inputs
    n_bad = pair_bounds(pos_gpu, pairs, lo, hi)[2]
    n_clash = clash_scan(pos_gpu, radius, ex_ptr, ex_idx, RR.CLASH)[2]
    n_bent = planar_deviation(pos_gpu, grp_ptr, grp_idx, FR.THRESH)[2]
    return ((n_bad == 0) & (n_clash == 0)).cpu().numpy(), (n_bent == 0).cpu().numpy()


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _against(what, inputs, got, fwd, rev, **kw):
    """the comparison with the reference and the properties every result must have"""
    pos = inputs[0]
    G = pos.shape[0]
    out, status, iters, resid, moved = (x.cpu().numpy() for x in got)
    size = lambda p: np.where(np.isfinite(p), np.abs(p), 0.0).max((1, 2))
    big = np.maximum(size(fwd["pos64"]), size(pos))
    assert big.max() < 16
    gate = POS_GATE * big[:, None, None]
    fin = np.isfinite(fwd["pos64"])
    err = np.seterr(invalid="ignore")                  # (a conformer that is not finite: masked below)
    self_diff = np.where(fin, np.abs(fwd["pos64"] - rev["pos64"]), 0.0)
    assert np.array_equal(fwd["status"], rev["status"]) and np.array_equal(fwd["iters"], rev["iters"])
    assert (self_diff < 0.25 * gate).all()
    diff = np.where(fin, np.abs(out.astype(np.float64) - fwd["pos64"]), 0.0)
    rel = lambda a, b: np.abs(a.astype(np.float64) - b)[np.isfinite(b) & (b != 0)] / np.abs(b[np.isfinite(b) & (b != 0)])
    print("%s: status %s, iters %s; largest differences: pos %.3e (%.2f of its gate; the reference's two routes %.3e), resid %.3e, "
          "moved %.3e relative" % (what, status.tolist(), iters.tolist(), diff.max(), (diff / gate).max(), self_diff.max(),
                                   rel(resid, fwd["resid"]).max(initial=0.0), rel(moved, fwd["moved"]).max(initial=0.0)))
    assert np.array_equal(status, fwd["status"]) and np.array_equal(iters, fwd["iters"])
    assert (diff <= gate).all()
    for a, b in ((resid, fwd["resid"]), (moved, fwd["moved"])):
        assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.array_equal(a[~np.isfinite(b)], b[~np.isfinite(b)].astype(np.float32))
        assert (np.abs(a.astype(np.float64) - b)[np.isfinite(b)] <= VR.GATE * np.abs(b[np.isfinite(b)])).all()
    np.seterr(**err)
    # the properties
    same = np.array([np.array_equal(out[g].view(np.int32), pos[g].view(np.int32)) for g in range(G)])
    assert same[(status == 0) | (status == 3)].all() and not same[(status == 1) | (status == 2)].any()
    assert not resid[status == 0].any() and not moved[status == 0].any() and np.isposinf(resid[status == 3]).all()
    assert not iters[(status == 0) | (status == 3)].any()
    ok = np.isin(status, (0, 1))
    if ok.any():
        valid, flat = _judged(got[0][torch.from_numpy(ok).cuda()].contiguous(), inputs)
        assert valid.all() and flat.all()
    assert _same_bits(_run(inputs, **kw), got)                                  # two calls
    if G > 1:                                                                   # each conformer alone, the batch in another order
        for g in range(G):
            assert _same_bits(_run((pos[g:g + 1],) + inputs[1:], **kw), [x[g:g + 1] for x in got])
        order = list(range(G))[::-1]
        assert _same_bits(_run((pos[order],) + inputs[1:], **kw), [x[order] for x in got])
    return out, status, iters


# (case, max_iter) -> the statuses the restatement gives (tests/test_flatten_cpu.py pins the update counts)
CASES = {("styrene4", 200): [0, 1, 1, 0], ("acetone", 200): [1], ("naphthalene", 200): [1], ("boat", 200): [1], ("boat_stretched", 200): [1],
         ("vinyl85", 200): [1], ("vinyl90", 200): [1], ("mixed", 200): [0, 1, 1, 1, 3, 1], ("mixed", 5): [0, 2, 1, 2, 3, 2],
         ("styrene_x9", 200): [1, 1], ("styrene_x20", 200): [1, 1], ("styrene_x20_full", 200): [1]}


@pytest.mark.parametrize("key,max_iter", sorted(CASES))
def test_relax_planar_matches_the_float64_reference(key, max_iter):
    from agdiff_amd import _lib
    inputs, fwd, rev = FR.solved(key, max_iter=max_iter)
    assert fwd["status"].tolist() == CASES[(key, max_iter)]
    got = _run(inputs, max_iter=max_iter)
    out, status, iters = _against("%s, at most %d updates" % (key, max_iter), inputs, got, fwd, rev, max_iter=max_iter)
    assert (iters[status == 2] == max_iter).all() and (iters <= max_iter).all()
    n, P = inputs[0].shape[1], inputs[1].shape[0] - 1
    if key == "mixed":
        assert np.isnan(out[4, 9, 1])
    if key == "styrene_x9":
        assert (n, P) == (144, 18)                                              # one lane per atom, the large instantiation
    if key == "styrene_x20":
        assert (n, P) == (320, 40)                                              # atoms strided over the threads
    if key == "styrene_x20_full":
        assert (n, P) == (320, _lib.DEFINES["AGDIFF_FLATTEN_MAX_GROUPS"]) and set(np.diff(inputs[1]).tolist()) == set(range(3, 9))


def test_the_distance_repair_alone_leaves_the_bent_styrene_bent():
    """the "before": every styrene conformer is valid, so agdiff_relax_bounds returns all four as they came -- bent ones included"""
    from agdiff_amd.planarity import planar_deviation
    from agdiff_amd.validity import relax_bounds
    inputs, fwd, _ = FR.solved("styrene4")
    pos = _gpu(inputs[0])
    out, status, _, _, _ = relax_bounds(pos, *inputs[3:])
    assert status.tolist() == [0, 0, 0, 0] and torch.equal(out, pos)
    assert planar_deviation(out, inputs[1], inputs[2], FR.THRESH)[2].tolist() == [0, 1, 1, 0]
    after = planar_deviation(_run(inputs)[0], inputs[1], inputs[2], FR.THRESH)
    assert after[2].tolist() == [0, 0, 0, 0] and (after[0] <= FR.FLAT_TO + RR.PAD / 2 + 1e-6).all()


def test_without_groups_it_is_the_distance_repair():
    from agdiff_amd.planarity import relax_planar
    from agdiff_amd.validity import relax_bounds
    inputs, fwd, rev = RR.solved("tree61")
    none = (np.zeros(1, np.int32), np.zeros(0, np.int32))
    assert fwd["status"].tolist() == [1, 1, 2]
    got = relax_planar(_gpu(inputs[0]), *none, *inputs[1:])
    _against("tree61 without groups", (inputs[0],) + none + inputs[1:], got, fwd, rev)
    assert _same_bits(relax_bounds(_gpu(inputs[0]), *inputs[1:]), got)


def _raw(inputs, **over):
    """agdiff_relax_planar itself, past the host checks of relax_planar"""
    from agdiff_amd import _lib
    from agdiff_amd.planarity import membership_csr
    from agdiff_amd.validity import relax_tables
    pos = _gpu(inputs[0])
    G, n = pos.shape[:2]
    bd_ptr, bd_idx, bd_lo, bd_hi, rad, ptr, idx, K = relax_tables(n, *inputs[3:])
    mb_ptr, mb_grp = membership_csr(n, inputs[1], inputs[2])
    dev = [torch.from_numpy(np.array(x)).cuda() for x in (bd_ptr, bd_idx, bd_lo, bd_hi, rad, ptr, idx, inputs[1], inputs[2], mb_ptr, mb_grp)]
    a = dict(dict(G=G, n=n, K=K, P=inputs[1].shape[0] - 1, clash=0.6, pad=0.02, omega=1.0, max_iter=200, thresh=0.25, flat_to=0.10), **over)
    res = [torch.empty_like(pos)] + [torch.empty(G, dtype=t, device="cuda") for t in (torch.int32, torch.int32, torch.float32, torch.float32)]
    _lib.call("agdiff_relax_planar", pos, *dev, *[a[k] for k in ("G", "n", "K", "P", "clash", "pad", "omega", "max_iter", "thresh", "flat_to")],
              *res)
    return res


def test_limits_and_bad_parameters_come_back_as_errors():
    from agdiff_amd import _lib
    from agdiff_amd.planarity import relax_planar
    cap = _lib.DEFINES["AGDIFF_FLATTEN_MAX_GROUPS"]
    inputs, fwd, _ = FR.solved("styrene_x20_full")
    assert inputs[1].shape[0] - 1 == cap
    over = FR.with_groups(inputs[1:], [np.array([0, 1, 2])])
    assert over[0].shape[0] - 1 == cap + 1
    with pytest.raises(_lib.AgdiffLimitError):
        relax_planar(_gpu(inputs[0]), *over)
    small, _, _ = FR.solved("styrene4")
    assert _same_bits(_raw(small), _run(small))
    for bad in (dict(flat_to=0.24), dict(thresh=float("nan")), dict(thresh=float("inf")), dict(flat_to=float("nan")), dict(flat_to=-0.1),
                dict(P=-1)):
        with pytest.raises(_lib.AgdiffHipError) as e:
            _raw(small, **bad)
        assert not isinstance(e.value, _lib.AgdiffLimitError), bad
    with pytest.raises(ValueError, match="flat_to"):
        _run(small, flat_to=0.24)
    empty = relax_planar(torch.zeros((0, 16, 3), device="cuda"), *small[1:])
    assert empty[0].shape == (0, 16, 3) and all(x.shape == (0,) for x in empty[1:])


# ------------------------------------------------------------------------------------------------ through the layers
BENT = (1, 2, 5, 6, 9, 10)


@functools.lru_cache(maxsize=None)
def _dozen():
    """styrene, twelve conformers with 0.005 A of noise: flat, and at BENT planarity_ref's bent and twisted conformers in turn"""
    import planarity_ref as PR
    mol, four = PR.styrene_conformers()
    rng = np.random.default_rng(12)
    gen = RR.centred(np.stack([four[1 + BENT.index(g) % 2 if g in BENT else 0] for g in range(12)]) + 0.005 * rng.normal(size=(12, 16, 3)))
    gen.setflags(write=False)
    return mol, gen


def test_repair_planarity_flattens_the_bent_half_and_returns_the_rest_bit_for_bit():
    from agdiff_amd.planarity import check_planarity, repair_planarity
    from agdiff_amd.validity import check_geometry, repair_geometry
    mol, gen = _dozen()
    item = lambda pos: FR.item_of(mol, pos_gen=pos)
    assert check_planarity(item(gen))["flat"].tolist() == [g not in BENT for g in range(12)]
    assert check_geometry(item(gen))["valid"].all()
    assert not repair_geometry(item(gen))["status"].any()                       # the distance repair sees nothing to do
    res = repair_planarity(item(gen))
    assert set(res) == {"pos", "status", "iters", "resid", "moved"} and res["pos"].shape == (12, 16, 3)
    assert res["status"].tolist() == [int(g in BENT) for g in range(12)]
    good = [g for g in range(12) if g not in BENT]
    assert torch.equal(res["pos"][good].cpu(), torch.from_numpy(gen[good])) and not res["iters"][good].any()
    assert (res["iters"][list(BENT)] > 0).all() and (res["moved"][list(BENT)] > 0).all() and (res["resid"] <= 0.01).all()
    after = check_planarity(item(res["pos"]))
    assert after["flat"].all() and (after["flat_dev"] <= 0.11 + 1e-6).all() and check_geometry(item(res["pos"]))["valid"].all()
    # the caller's own groups (the ring alone: the twisted conformers are then flat as they came), a flat_to and a pad of the caller's
    ring = (np.array([0, 6], np.int32), np.arange(6, dtype=np.int32))
    own = repair_planarity(item(gen), groups=ring, flat_to=0.05, pad=0.01, max_iter=500)
    assert own["status"].tolist() == [int(g in BENT and BENT.index(g) % 2 == 0) for g in range(12)]
    assert (check_planarity(item(own["pos"]), groups=ring)["flat_dev"][own["status"] == 1] <= 0.055 + 1e-6).all()


def test_run_job_flattens_with_the_switch_and_saves_nothing_new_without_it(tmp_path):
    from agdiff_amd import driver, get_model, planarity, qm9_model_config, synth
    from agdiff_amd.planarity import check_planarity, planar_groups
    from agdiff_amd.validity import check_geometry
    m = get_model(qm9_model_config(num_diffusion_timesteps=8))
    m.load_state_dict(synth.synth_state_dict(m.state_dict()))
    m = m.to("cuda:0").eval()
    # the 13-atom molecule of tests/test_hip_relax.py with the chain 0-1-4-5-8-10 closed into an aromatic ring
    at, src, dst, typ = synth.random_molecule(np.random.default_rng(5), 13, raw_bonds=True)
    ring = [0, 1, 4, 5, 8, 10]
    on_ring = {(ring[k], ring[(k + 1) % 6]) for k in range(6)} | {(ring[(k + 1) % 6], ring[k]) for k in range(6)}
    typ = np.where([(int(a), int(b)) in on_ring for a, b in zip(src, dst)], 12, typ)
    src, dst, typ = np.append(src, [10, 0]), np.append(dst, [0, 10]), np.append(typ, [12, 12])
    r, c, ty = synth.extend_graph_order_np(13, src, dst, typ, order=3)
    mols = [dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=ty, num_refs=6, name="mol0", index=0)]
    item = lambda pos: dict(atom_type=at, pos_gen=pos, edge_index=mols[0]["edge_index"], edge_type=ty)
    ptr, idx, _ = planar_groups(item(None))
    assert ring in [idx[ptr[k]:ptr[k + 1]].tolist() for k in range(len(ptr) - 1)]
    confs = lambda num_refs: num_refs
    kw = dict(n_steps=4, step_lr=1e-6, w_global=1.0, clip=1000.0)
    logs = []
    job = lambda name, **sw: driver.run_job(m, mols, str(tmp_path / name), confs, 10 ** 6, kw, "cuda:0", log=logs.append, noise="counter",
                                            seed=7, **sw)
    plain = job("plain")
    assert set(plain.keys()) == {"pos_gen_0", "name_0"} and not any("repaired" in str(x) for x in logs)
    plain_file = glob.glob(str(tmp_path / "plain" / "samples_[0-9]*.npz"))[0]
    assert set(np.load(plain_file).files) == {"pos_gen_0", "name_0"}
    res = job("flattened", repair_planarity=True, check_geometry=True, check_planarity=True)
    assert sum("were repaired (flattened" in str(x) for x in logs) == 1
    keys = {"pos_gen_0", "name_0", "repair_status_0", "repair_moved_0", "valid_0", "bond_dev_0", "clash_0", "flat_0", "flat_dev_0"}
    for z in (res, np.load(glob.glob(str(tmp_path / "flattened" / "samples_[0-9]*.npz"))[0]),
              np.load(str(tmp_path / "flattened" / "samples_all.npz"))):
        assert set(z.keys() if isinstance(z, dict) else z.files) == keys
        status = z["repair_status_0"]
        assert status.dtype == np.int8 and z["repair_moved_0"].dtype == np.float32 and status.shape == z["repair_moved_0"].shape == (6,)
        assert z["pos_gen_0"].shape == (6, 13, 3) and z["pos_gen_0"].dtype == np.float32 and np.isin(status, (0, 1, 2)).all()
        assert np.array_equal(z["pos_gen_0"][status == 0], plain["pos_gen_0"][status == 0])
        assert (z["repair_moved_0"][status == 0] == 0).all() and (z["repair_moved_0"][status != 0] > 0).all()
        assert (z["valid_0"][status <= 1] == 1).all() and (z["flat_0"][status <= 1] == 1).all()
        assert np.array_equal(z["valid_0"], check_geometry(item(z["pos_gen_0"]))["valid"].cpu().numpy().astype(np.int8))
        want = check_planarity(item(z["pos_gen_0"]))
        assert np.array_equal(z["flat_0"], want["flat"].cpu().numpy().astype(np.int8))
        assert np.array_equal(z["flat_dev_0"], want["flat_dev"].cpu().numpy())
    # what the switch did is what repair_planarity does to the plain job's conformers; the plain job's files are as they were
    direct = planarity.repair_planarity(item(plain["pos_gen_0"]))
    assert np.array_equal(direct["pos"].cpu().numpy(), res["pos_gen_0"])
    assert np.array_equal(direct["status"].cpu().numpy().astype(np.int8), res["repair_status_0"])
    assert np.array_equal(direct["moved"].cpu().numpy(), res["repair_moved_0"])
    assert set(np.load(plain_file).files) == {"pos_gen_0", "name_0"}
    assert np.array_equal(np.load(plain_file)["pos_gen_0"], plain["pos_gen_0"])
    print("run_job: repair_status %s, moved %s" % (res["repair_status_0"].tolist(), np.round(res["repair_moved_0"], 3).tolist()))
    # both repair switches equal the new one alone
    both = job("both", repair_planarity=True, repair_geometry=True)
    assert set(both.keys()) == {"pos_gen_0", "name_0", "repair_status_0", "repair_moved_0"}
    assert all(np.array_equal(both[k], res[k]) for k in ("pos_gen_0", "repair_status_0", "repair_moved_0"))

    # the command line on the plain job's files: the same repair, the verdicts on the repaired conformers
    driver.save_testset(str(tmp_path / "test.npz"), mols)
    samples = str(tmp_path / "plain" / "samples_all.npz")
    out = planarity.main(["--samples", samples, "--testset", str(tmp_path / "test.npz"), "--out", str(tmp_path / "planarity.npz"),
                          "--repair", str(tmp_path / "flat.npz")])
    z, v = np.load(str(tmp_path / "flat.npz")), np.load(str(tmp_path / "planarity.npz"))
    assert set(z.files) == {"pos_gen_0", "name_0", "repair_status_0", "repair_moved_0"} and str(z["name_0"]) == "mol0"
    assert z["repair_status_0"].dtype == np.int8 and z["repair_moved_0"].dtype == np.float32
    assert all(np.array_equal(z[k], res[k]) for k in ("pos_gen_0", "repair_status_0", "repair_moved_0"))
    assert all(np.array_equal(v[k + "_0"], res[k + "_0"]) for k in ("flat", "flat_dev")) and np.array_equal(out["flat_0"], v["flat_0"])
    assert set(np.load(samples).files) == {"pos_gen_0", "name_0"}                  # the samples file itself is left alone
    few = planarity.main(["--samples", samples, "--testset", str(tmp_path / "test.npz"), "--out", str(tmp_path / "p2.npz"),
                          "--repair", str(tmp_path / "few.npz"), "--max-iter", "1", "--omega", "0.5", "--pad", "0.03", "--flat-to", "0.2"])
    z = np.load(str(tmp_path / "few.npz"))
    assert np.array_equal(z["repair_status_0"] == 0, res["repair_status_0"] == 0) and few["flat_0"].shape == (6,)
