"""GPU (MI355X): the geometry repair (agdiff_amd.validity.relax_bounds; csrc/eval.hip: k_relax_bounds) against the float64 numpy
restatement of its rule (tests/relax_ref.py), by properties that need no reference, and through repair_geometry, the driver and the
command line.

Gates, none taken from what the kernel gives:
  status, iters   equal exactly.  That is a fair demand because the reference asserts on its own output, before the kernel is asked
            anything, that no quantity the stop rule compares comes within 1e-6 (relative) of its threshold at any iteration, and
            that no distance or ratio lies within VR.MARGIN of the bound that decides status 0 (relax_ref.Margin otherwise).
  pos_out   4 x 2^-24 x (the largest |coordinate| of that conformer) per coordinate: kernel and reference both compute in fp64 from
            the same fp32 input, so they differ by the final fp32 store -- half an ulp of a value at most that large, 2^-24 relative
            -- plus the fp64 rounding accumulated over the updates.  The reference measures that rounding on itself by summing every
            atom's terms in the opposite order: the test asserts that this self-difference is below a quarter of the gate, which is
            why the store error gets the factor 4 VR.GATE gives it.  The inputs are centred; every coordinate is asserted below 16.
  resid, moved    VR.GATE (4 x 2^-24) relative: fp64 values stored once as fp32.
  status 1  the project's own check kernels call the output valid: at exit every distance is inside its true limit by at least
            p_k / 2 (0.01 Angstrom for the table bounds, 0.0025 in the narrow-bounds test) and fp32 rounding of coordinates below 16
            moves a distance by under 2e-6 Angstrom, so this is an exact demand.
The shapes: n = 2 (one bond), 17 and 20 atoms (4 and 8 lanes per atom), 41 (one row of 40 bounds), 61, 128 and 130 (either side of
the kernel's small-LDS instantiation and of one lane per atom), 300 (more atoms than threads), K = 0 with clashes only."""
import functools
import glob

import numpy as np
import pytest
import torch

import relax_ref as RR
import validity_ref as VR

pytestmark = pytest.mark.gpu
POS_GATE = 4.0 * 2.0 ** -24


def _gpu(pos):
    return torch.from_numpy(np.array(pos, dtype=np.float32)).cuda()        # (a copy: the cached cases are read-only)


def _item(mol, **kw):
    at, ei, et = mol
    return dict(atom_type=at, edge_index=ei, edge_type=et, **kw)


def _run(inputs, **kw):
    from agdiff_amd.validity import relax_bounds
    pos, pairs, lo, hi, radius, ex_ptr, ex_idx = inputs
    out = relax_bounds(_gpu(pos), pairs, lo, hi, radius, ex_ptr, ex_idx, **kw)
    assert out[0].dtype == out[3].dtype == out[4].dtype == torch.float32 and out[1].dtype == out[2].dtype == torch.int32
    assert out[0].shape == pos.shape and all(o.shape == (pos.shape[0],) for o in out[1:])
    return out


def _judged_valid(pos_gpu, inputs, lo=None, hi=None):
    """bool [G]: the two check kernels on pos_gpu, at the true bounds"""
    from agdiff_amd.validity import clash_scan, pair_bounds
    _, pairs, lo0, hi0, radius, ex_ptr, ex_idx = inputs
    n_bad = pair_bounds(pos_gpu, pairs, lo0 if lo is None else lo, hi0 if hi is None else hi)[2]
    n_clash = clash_scan(pos_gpu, radius, ex_ptr, ex_idx, RR.CLASH)[2]
    return ((n_bad == 0) & (n_clash == 0)).cpu().numpy()


def _against(what, inputs, got, fwd, rev):
    """the comparison with the reference and the properties every result must have"""
    pos = inputs[0]
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
    print("%s: status %s, iters %s; largest differences: pos %.3e (%.2f of its gate; the reference's two orders %.3e), resid %.3e, "
          "moved %.3e relative" % (what, status.tolist(), iters.tolist(), diff.max(), (diff / gate).max(), self_diff.max(),
                                   rel(resid, fwd["resid"]).max(initial=0.0), rel(moved, fwd["moved"]).max(initial=0.0)))
    assert np.array_equal(status, fwd["status"]) and np.array_equal(iters, fwd["iters"])
    assert (diff <= gate).all()
    for a, b in ((resid, fwd["resid"]), (moved, fwd["moved"])):
        assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.array_equal(a[~np.isfinite(b)], b[~np.isfinite(b)].astype(np.float32))
        assert (np.abs(a.astype(np.float64) - b)[np.isfinite(b)] <= VR.GATE * np.abs(b[np.isfinite(b)])).all()
    np.seterr(**err)
    # the properties
    same = np.array([np.array_equal(out[g].view(np.int32), pos[g].view(np.int32)) for g in range(pos.shape[0])])
    assert same[(status == 0) | (status == 3)].all() and not same[(status == 1) | (status == 2)].any()
    assert not resid[status == 0].any() and not moved[status == 0].any() and np.isposinf(resid[status == 3]).all()
    assert not iters[(status == 0) | (status == 3)].any()
    ok = np.isin(status, (0, 1))
    if ok.any():
        assert _judged_valid(got[0][torch.from_numpy(ok).cuda()].contiguous(), inputs).all()
    return out, status, iters


# (case, omega, max_iter)
CASES = [("bond2", 1.0, 200), ("pentane_folded_1.9", 1.0, 200), ("pentane_folded_1.2", 1.0, 200), ("hexane_shifted", 1.0, 200),
         ("hexane_short_ch", 1.0, 200), ("hexane", 1.0, 200), ("butane_folded", 1.0, 200), ("star40", 1.0, 200), ("tree23", 1.0, 200),
         ("tree61", 1.0, 200), ("cloud128", 1.0, 200), ("tree130", 1.0, 200), ("tree130", 1.5, 200), ("tree300", 1.5, 200),
         ("pentane_refs", 1.0, 200), ("tree23", 1.0, 30)]


@pytest.mark.parametrize("key,omega,max_iter", CASES)
def test_relax_bounds_matches_the_float64_reference(key, omega, max_iter):
    inputs, fwd, rev = RR.solved(key, omega=omega, max_iter=max_iter)
    got = _run(inputs, omega=omega, max_iter=max_iter)
    _, status, iters = _against("%s omega %g" % (key, omega), inputs, got, fwd, rev)
    assert (iters[status == 2] == max_iter).all() and (iters <= max_iter).all()
    if key == "star40":
        assert inputs[1].shape[0] == 40 and (inputs[1][:, 0] == 0).all()         # one row of 40 bounds
    if key == "cloud128":
        assert inputs[1].shape[0] == 0 and (status == 1).all()                   # K = 0: clashes only
    if (key, max_iter) == ("tree23", 30):
        assert sorted(status.tolist()) == [1, 2, 2, 2]                           # the iteration limit cuts three of the four short


def test_bounds_narrower_than_two_pads_are_met_at_their_middle():
    from agdiff_amd.validity import relax_bounds
    inputs, _, _ = RR.solved("pentane_folded_1.9")
    pos, pairs, lo, hi, radius, ex_ptr, ex_idx = inputs
    mid = ((lo.astype(np.float64) + hi) / 2).astype(np.float32)
    lo_n, hi_n = mid - np.float32(0.005), mid + np.float32(0.005)
    narrow = (pos, pairs, lo_n, hi_n, radius, ex_ptr, ex_idx)
    fwd = RR.relax(*narrow)
    rev = RR.relax(*narrow, reverse=True, margins=False)
    assert fwd["status"].tolist() == [1]
    got = relax_bounds(_gpu(pos), pairs, lo_n, hi_n, radius, ex_ptr, ex_idx)
    _against("narrow bounds", narrow, got, fwd, rev)
    assert _judged_valid(got[0], narrow).all() and got[3].item() <= 0.0026


@functools.lru_cache(maxsize=None)
def _mixed():
    """tree61: a valid conformer (the reference's own repaired output of conformer 0), a broken one, one with a NaN and an Inf, and one
    that 200 updates do not repair"""
    inputs, fwd, _ = RR.solved("tree61")
    assert fwd["status"].tolist() == [1, 1, 2]
    pos = np.stack([fwd["pos"][0], inputs[0][1], inputs[0][0], inputs[0][2]])
    pos[2, 7, 1], pos[2, 40, 0] = np.nan, np.inf
    batch = (pos,) + inputs[1:]
    f, r = RR.relax(*batch), RR.relax(*batch, reverse=True, margins=False)
    pos.setflags(write=False)
    return batch, f, r


def test_conformers_of_one_batch_do_not_touch_each_other():
    batch, fwd, rev = _mixed()
    assert fwd["status"].tolist() == [0, 1, 3, 2]
    got = _run(batch)
    out, status, iters = _against("mixed batch", batch, got, fwd, rev)
    assert status.tolist() == [0, 1, 3, 2] and iters[3] == 200 and np.isnan(out[2, 7, 1]) and np.isposinf(out[2, 40, 0])
    # each conformer alone, and the batch in another order: the same bits
    for g in range(4):
        alone = _run((batch[0][g:g + 1],) + batch[1:])
        assert all(torch.equal(a.view(torch.int32), b[g:g + 1].view(torch.int32)) for a, b in zip(alone, got))
    order = [3, 2, 1, 0]
    turned = _run((batch[0][order],) + batch[1:])
    assert all(torch.equal(a.view(torch.int32), b[order].view(torch.int32)) for a, b in zip(turned, got))


def test_coincident_atoms_part_along_x_with_the_lower_index_towards_plus_x():
    from agdiff_amd.validity import relax_bounds
    # small integers and halvings: every number is exact on both sides (tests/test_relax_cpu.py has the arithmetic)
    pos = np.full((1, 2, 3), 2.0, dtype=np.float32)
    ptr, idx = np.array([0, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    for pairs in ([[0, 1]], [[1, 0]]):
        want = RR.relax(pos, pairs, [1.0], [3.0], [1.0, 1.0], ptr, idx, pad=0.5)
        out, status, iters, resid, moved = relax_bounds(_gpu(pos), pairs, [1.0], [3.0], [1.0, 1.0], ptr, idx, pad=0.5)
        assert out.tolist() == want["pos"].tolist() == [[[2.65625, 2.0, 2.0], [1.34375, 2.0, 2.0]]]
        assert (status.tolist(), iters.tolist(), resid.tolist(), moved.tolist()) == ([1], [3], [0.1875], [0.65625])
    # unbonded and not excluded: the clash term parts them the same way
    none = np.zeros(3, dtype=np.int32)
    want = RR.relax(pos, np.zeros((0, 2)), [], [], [1.0, 1.0], none, none[:0], pad=0.5)
    out, status, _, _, _ = relax_bounds(_gpu(pos), np.zeros((0, 2), np.int32), [], [], [1.0, 1.0], none, none[:0], pad=0.5)
    assert status.tolist() == [1] and out.tolist() == want["pos"].tolist() and out[0, 0, 0] > 2.0 > out[0, 1, 0]
    assert out[0, :, 1:].tolist() == [[2.0, 2.0], [2.0, 2.0]]


def test_two_calls_give_the_same_bits():
    inputs, _, _ = RR.solved("tree130")
    a, b = _run(inputs), _run(inputs)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    inputs, _, _ = RR.solved("star40")
    a, b = _run(inputs), _run(inputs)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_limits_come_back_as_errors():
    from agdiff_amd import _lib
    from agdiff_amd.validity import relax_bounds
    n = _lib.DEFINES["AGDIFF_RELAX_MAX_ATOMS"] + 1
    none = (np.zeros((0, 2), np.int32), [], [])
    big = (np.ones(n, np.float32), np.zeros(n + 1, np.int32), np.zeros(0, np.int32))
    with pytest.raises(_lib.AgdiffLimitError):
        relax_bounds(torch.zeros((1, n, 3), device="cuda"), *none, *big)
    small = (np.ones(3, np.float32), np.zeros(4, np.int32), np.zeros(0, np.int32))
    pos = torch.zeros((1, 3, 3), device="cuda")
    for bad in (0, _lib.DEFINES["AGDIFF_RELAX_MAX_ITERS"] + 1):
        with pytest.raises(_lib.AgdiffHipError) as e:
            relax_bounds(pos, *none, *small, max_iter=bad)
        assert not isinstance(e.value, _lib.AgdiffLimitError)
    # the largest molecule and the longest run the limits admit go through: atoms on a lattice 10 apart are valid as they are
    a = np.arange(n - 1)
    lattice = np.stack([10 * (a % 16) - 75, 10 * ((a // 16) % 8) - 35, 10 * (a // 128) - 35], axis=1).astype(np.float32)
    out, status, _, _, _ = relax_bounds(_gpu(lattice[None]), *none, np.ones(n - 1, np.float32), np.zeros(n, np.int32), np.zeros(0, np.int32),
                                        max_iter=_lib.DEFINES["AGDIFF_RELAX_MAX_ITERS"])
    assert status.tolist() == [0] and torch.equal(out.cpu(), torch.from_numpy(lattice[None]))
    empty = relax_bounds(torch.zeros((0, 3, 3), device="cuda"), *none, *small)
    assert empty[0].shape == (0, 3, 3) and all(x.shape == (0,) for x in empty[1:])


# ------------------------------------------------------------------------------------------------ through the layers
BROKEN = (1, 3, 4, 7, 8, 10)


@functools.lru_cache(maxsize=None)
def _dozen():
    """n-butane, twelve conformers: anti and the two gauche forms with a little noise, and at BROKEN six broken ones -- the C3 - C4
    bond stretched by 1.5 Angstrom (the methyl group moved as one), a C - H shortened to 0.4 of its length, the methyl carbon pushed
    onto the chain, twice each"""
    rng = np.random.default_rng(12)
    confs, mol = [], None
    tors = iter([np.pi, np.pi / 3, -np.pi / 3] * 4)
    for g in range(12):
        mol, pos = VR.alkane(4, torsions=[next(tors)])
        if g in BROKEN:
            kind = BROKEN.index(g) % 3
            if kind == 0:
                pos[[3, 11, 12, 13]] += 1.5 * (pos[3] - pos[2]) / np.linalg.norm(pos[3] - pos[2])
            elif kind == 1:
                pos[5] = pos[0] + 0.4 * (pos[5] - pos[0])
            else:
                pos[3] = pos[2] + 0.5 * (pos[3] - pos[2])
        confs.append(pos + 0.005 * rng.normal(size=pos.shape))
    gen = RR.centred(np.stack(confs))
    gen.setflags(write=False)
    return mol, gen


def test_repair_geometry_mends_the_broken_half_and_returns_the_rest_bit_for_bit():
    from agdiff_amd.validity import check_geometry, repair_geometry
    mol, gen = _dozen()
    before = check_geometry(_item(mol, pos_gen=gen))["valid"].tolist()
    assert before == [g not in BROKEN for g in range(12)]
    res = repair_geometry(_item(mol, pos_gen=gen))
    assert set(res) == {"pos", "status", "iters", "resid", "moved"} and res["pos"].shape == (12, 14, 3)
    assert res["status"].tolist() == [int(g in BROKEN) for g in range(12)]
    good = [g for g in range(12) if g not in BROKEN]
    assert torch.equal(res["pos"][good].cpu(), torch.from_numpy(gen[good])) and not res["iters"][good].any()
    assert (res["iters"][list(BROKEN)] > 0).all() and (res["moved"][list(BROKEN)] > 0).all() and (res["resid"] <= 0.01).all()
    after = check_geometry(_item(mol, pos_gen=res["pos"]))
    assert after["valid"].all() and not after["n_bad"].any() and not after["n_clash"].any()
    # the reference conformers' own bounds, a clash threshold and a pad of the caller's
    refs = repair_geometry(_item(mol, pos_gen=gen, pos_ref=gen[good]), bounds="references", clash=0.5, pad=0.01, max_iter=500)
    assert not refs["status"][good].any() and torch.equal(refs["pos"][good].cpu(), torch.from_numpy(gen[good]))
    fixed = (refs["status"] == 1).cpu().numpy()
    again = check_geometry(_item(mol, pos_gen=refs["pos"], pos_ref=gen[good]), bounds="references", clash=0.5)["valid"].cpu().numpy()
    assert again[fixed].all() and fixed.sum() >= 1


def test_run_job_repairs_with_the_switch_and_saves_nothing_new_without_it(tmp_path):
    from agdiff_amd import driver, get_model, qm9_model_config, synth, validity
    from agdiff_amd.validity import check_geometry
    m = get_model(qm9_model_config(num_diffusion_timesteps=8))
    m.load_state_dict(synth.synth_state_dict(m.state_dict()))
    m = m.to("cuda:0").eval()
    at, r, c, ty = synth.random_molecule(np.random.default_rng(5), 13)
    mols = [dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=ty, num_refs=6, name="mol0", index=0)]
    confs = lambda num_refs: num_refs
    kw = dict(n_steps=4, step_lr=1e-6, w_global=1.0, clip=1000.0)
    logs = []
    job = lambda name, **sw: driver.run_job(m, mols, str(tmp_path / name), confs, 10 ** 6, kw, "cuda:0", log=logs.append, noise="counter",
                                            seed=7, **sw)
    plain = job("plain")
    assert set(plain.keys()) == {"pos_gen_0", "name_0"} and not any("repaired" in str(x) for x in logs)
    assert set(np.load(glob.glob(str(tmp_path / "plain" / "samples_[0-9]*.npz"))[0]).files) == {"pos_gen_0", "name_0"}
    res = job("repaired", repair_geometry=True, check_geometry=True)
    assert sum("were repaired" in str(x) for x in logs) == 1
    files = glob.glob(str(tmp_path / "repaired" / "samples_[0-9]*.npz"))
    assert len(files) == 1
    item = lambda pos: dict(atom_type=at, pos_gen=pos, edge_index=mols[0]["edge_index"], edge_type=ty)
    for z in (res, np.load(files[0]), np.load(str(tmp_path / "repaired" / "samples_all.npz"))):
        assert set(z.keys() if isinstance(z, dict) else z.files) == {"pos_gen_0", "name_0", "repair_status_0", "repair_moved_0", "valid_0",
                                                                     "bond_dev_0", "clash_0"}
        status = z["repair_status_0"]
        assert status.dtype == np.int8 and z["repair_moved_0"].dtype == np.float32 and status.shape == z["repair_moved_0"].shape == (6,)
        assert z["pos_gen_0"].shape == (6, 13, 3) and z["pos_gen_0"].dtype == np.float32
        assert np.isin(status, (0, 1, 2)).all()
        # the same draws in both jobs: a conformer valid as sampled is the plain job's, byte for byte; the verdicts are on the repaired
        assert np.array_equal(z["pos_gen_0"][status == 0], plain["pos_gen_0"][status == 0])
        assert (z["repair_moved_0"][status == 0] == 0).all() and (z["repair_moved_0"][status != 0] > 0).all()
        assert (z["valid_0"][status <= 1] == 1).all()
        want = check_geometry(item(z["pos_gen_0"]))
        assert np.array_equal(z["valid_0"], want["valid"].cpu().numpy().astype(np.int8))
        assert np.array_equal(z["bond_dev_0"], want["bond_dev"].cpu().numpy()) and np.array_equal(z["clash_0"], want["clash"].cpu().numpy())
    # what the switch did is what repair_geometry does to the plain job's conformers
    direct = validity.repair_geometry(item(plain["pos_gen_0"]))
    assert np.array_equal(direct["pos"].cpu().numpy(), res["pos_gen_0"])
    assert np.array_equal(direct["status"].cpu().numpy().astype(np.int8), res["repair_status_0"])
    print("run_job: repair_status %s, moved %s" % (res["repair_status_0"].tolist(), np.round(res["repair_moved_0"], 3).tolist()))
    alone = job("alone", repair_geometry=True)
    assert set(alone.keys()) == {"pos_gen_0", "name_0", "repair_status_0", "repair_moved_0"}
    assert np.array_equal(alone["pos_gen_0"], res["pos_gen_0"])

    # the command line on the plain job's files: the same repair, the verdicts on the repaired conformers
    driver.save_testset(str(tmp_path / "test.npz"), mols)
    samples = str(tmp_path / "plain" / "samples_all.npz")
    out = validity.main(["--samples", samples, "--testset", str(tmp_path / "test.npz"), "--out", str(tmp_path / "validity.npz"),
                         "--repair", str(tmp_path / "mended.npz")])
    z, v = np.load(str(tmp_path / "mended.npz")), np.load(str(tmp_path / "validity.npz"))
    assert set(z.files) == {"pos_gen_0", "name_0", "repair_status_0", "repair_moved_0"} and str(z["name_0"]) == "mol0"
    assert z["repair_status_0"].dtype == np.int8 and z["repair_moved_0"].dtype == np.float32
    assert all(np.array_equal(z[k], res[k]) for k in ("pos_gen_0", "repair_status_0", "repair_moved_0"))
    assert all(np.array_equal(v[k + "_0"], res[k + "_0"]) for k in ("valid", "bond_dev", "clash")) and np.array_equal(out["valid_0"], v["valid_0"])
    assert set(np.load(samples).files) == {"pos_gen_0", "name_0"}                  # the samples file itself is left alone
    few = validity.main(["--samples", samples, "--testset", str(tmp_path / "test.npz"), "--out", str(tmp_path / "v2.npz"),
                         "--repair", str(tmp_path / "few.npz"), "--max-iter", "1", "--omega", "0.5", "--pad", "0.03"])
    z = np.load(str(tmp_path / "few.npz"))
    assert np.array_equal(z["repair_status_0"] == 0, res["repair_status_0"] == 0) and few["valid_0"].shape == (6,)
