"""GPU (MI355X): the torsion fingerprint deviation (agdiff_amd.torsions; csrc/eval.hip: k_torsion_angles, k_tfd_matrix) against
the float64 numpy restatement of its definitions (tests/tfd_ref.py), and through prune, evaluation and the driver.

Gates, none taken from what the kernels give:
  ANGLE_ATOL 1e-6 rad  kernel and reference both compute in fp64 from the same fp32 coordinates, so the difference is the fp32 store
                       of theta: half an ulp, 2^-23 = 1.2e-7 at |theta| >= 2, with a margin of 8
  MOVE_ATOL  1e-5 rad  a conformer rotated and translated in fp64 and rounded to fp32 again: each coordinate (|x| < 8 here) moves by up
                       to 2^-22 = 2.4e-7, the atoms of a quad sit >= 1.3 Angstrom off the axes they turn about, four atoms, both
                       conformers rounded: a few 1e-6
  TFD_ATOL   2e-7      the value is a pure fp64 function of the fp32 angle table; only the final fp32 store differs, and 2 ulp at 1.0
                       is 1.2e-7
  MOL_ATOL   1e-5      rotamers constructed in fp64 and rounded to fp32 (as MOVE_ATOL), divided by pi"""
import functools
import glob

import numpy as np
import pytest
import torch

import tfd_ref as TR

pytestmark = pytest.mark.gpu
ANGLE_ATOL, MOVE_ATOL, TFD_ATOL, MOL_ATOL = 1e-6, 1e-5, 2e-7, 1e-5


def _angles(pos, quads):
    from agdiff_amd.torsions import torsion_angles
    return torsion_angles(torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).cuda(), quads)


def _random_quads(rng, n, Q):
    return np.stack([rng.permutation(n)[:4] for _ in range(Q)]).astype(np.int32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def _angle_case(n, G, Q):
    """(pos fp32 [G, n, 3], quads, reference dihedrals float64 [G, Q], the kernel's table as numpy) -- computed once"""
    rng = np.random.default_rng(100 * n + G)
    pos = (rng.normal(size=(G, n, 3)) * 1.5).astype(np.float32)
    quads = _random_quads(rng, n, Q)
    want = TR.dihedrals(pos, quads)
    got = _angles(pos, quads).cpu().numpy()
    for a in (pos, want, got):
        a.setflags(write=False)
    return pos, quads, want, got


def _item(mol, **kw):
    at, bi, bt = mol
    return dict(atom_type=at, bond_index=bi, bond_type=bt, **kw)


# ------------------------------------------------------------------------------------------------ 1. angles
def test_pinned_sign_of_the_dihedral():
    phis = [0.0, 1.0, np.pi / 2, -2.5, np.pi]
    pos = np.array([[[1, 0, 0], [0, 0, 0], [0, 0, 1], [np.cos(f), np.sin(f), 1]] for f in phis])
    got = _angles(pos, [[0, 1, 2, 3], [3, 2, 1, 0]]).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (5, 2) and (np.abs(got) <= np.float32(np.pi)).all()
    # (cos and sin rounded to fp32 move phi itself by up to 6e-8: inside the gate)
    assert TR.circular_difference(got[:, 0].astype(np.float64), np.array(phis)).max() <= ANGLE_ATOL
    assert TR.circular_difference(got[:, 1].astype(np.float64), np.array(phis)).max() <= ANGLE_ATOL      # reversal
    inv = _angles(-pos, [[0, 1, 2, 3]]).cpu().numpy()
    assert TR.circular_difference(inv[:, 0].astype(np.float64), -np.array(phis)).max() <= ANGLE_ATOL


@pytest.mark.parametrize("n,G,Q", [(9, 1, 3), (23, 10, 12), (61, 33, 70), (200, 40, 130)])
def test_angles_match_the_float64_reference(n, G, Q):
    pos, quads, want, got = _angle_case(n, G, Q)
    assert got.shape == (G, Q) and np.isfinite(got).all()
    err = TR.circular_difference(got.astype(np.float64), want).max()
    print("n = %d, G = %d, Q = %d: largest circular difference to the reference %.3e rad" % (n, G, Q, err))
    assert err <= ANGLE_ATOL
    mirrored = _angles(-pos, quads).cpu().numpy()
    assert TR.circular_difference(mirrored.astype(np.float64), -got.astype(np.float64)).max() <= ANGLE_ATOL


def test_a_rigid_motion_leaves_the_angles():
    rng = np.random.default_rng(7)
    G, k = 12, 9
    chains = np.stack([TR.chain_positions(rng.uniform(-np.pi, np.pi, size=k - 3)) for _ in range(G)])
    chains -= chains.mean(1, keepdims=True)
    quads = [[i, i + 1, i + 2, i + 3] for i in range(k - 3)] + [[i + 3, i + 2, i + 1, i] for i in range(k - 3)]
    moved = np.empty_like(chains)
    for g in range(G):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        moved[g] = chains[g] @ q.T + rng.normal(size=3)
    assert np.abs(moved).max() < 8.0
    a, b = _angles(chains, quads).cpu().numpy().astype(np.float64), _angles(moved, quads).cpu().numpy().astype(np.float64)
    err = TR.circular_difference(a, b).max()
    print("largest change of a dihedral under a rigid motion: %.3e rad" % err)
    assert err <= MOVE_ATOL


def test_broken_quads_give_nan_in_their_own_column_only():
    rng = np.random.default_rng(11)
    G, n = 3, 14
    clean = (rng.normal(size=(G, n, 3)) * 1.5).astype(np.float32)
    bad = clean.copy()
    bad[:, 8], bad[:, 9], bad[:, 10] = [0, 0, 0], [1, 0, 0], [2, 0, 0]          # a - u - v collinear
    bad[:, 12] = bad[:, 11]                                                     # two coincident atoms
    bad[1, 13, 0] = np.nan                                                      # one NaN coordinate, in conformer 1 only
    good = _random_quads(rng, 8, 70)                                            # atoms 0 .. 7 only; past the lane stride
    special = np.array([[8, 9, 10, 0], [0, 1, 11, 12], [0, 1, 2, 13], [0, 1, 2, n], [-1, 1, 2, 3]], dtype=np.int32)
    valid = np.array([[8, 9, 10, 0], [0, 1, 11, 12], [0, 1, 2, 13], [0, 1, 2, 3], [4, 1, 2, 3]], dtype=np.int32)
    where = [5, 20, 33, 64, 69]                                                 # columns the special quads are put at
    q_bad, q_clean = np.zeros((75, 4), dtype=np.int32), np.zeros((75, 4), dtype=np.int32)
    rest = [c for c in range(75) if c not in where]
    q_bad[rest], q_clean[rest] = good, good
    q_bad[where], q_clean[where] = special, valid
    a, b = _angles(clean, q_clean).cpu().numpy(), _angles(bad, q_bad).cpu().numpy()
    assert np.isfinite(a).all()
    assert np.array_equal(a[:, rest].view(np.int32), b[:, rest].view(np.int32))
    want_nan = np.ones((G, 5), dtype=bool)
    want_nan[[0, 2], 2] = False                                                 # (the NaN coordinate sits in conformer 1)
    assert np.array_equal(np.isnan(b[:, where]), want_nan)
    assert np.array_equal(np.isnan(TR.dihedrals(bad, q_bad)), np.isnan(b))


# ------------------------------------------------------------------------------------------------ 2. TFD from the kernel's table
@functools.lru_cache(maxsize=None)
def _tables(R, G, T):
    """(x [R, Q], y [G, Q]) on the GPU: the kernel's own angle tables of random conformers, Q = T + 3 columns"""
    rng = np.random.default_rng(1000 * R + 10 * G + T)
    n, Q = 20, T + 3
    quads = _random_quads(rng, n, Q)
    x = _angles(rng.normal(size=(R, n, 3)) * 1.5, quads)
    y = _angles(rng.normal(size=(G, n, 3)) * 1.5, quads)
    return x, y


@pytest.mark.parametrize("R,G", [(1, 1), (5, 10), (17, 33), (3, 40)])
def test_tfd_matches_the_float64_reference(R, G):
    from agdiff_amd.torsions import tfd_from_angles
    worst = 0.0
    for T in (0, 1, 7, 70):
        x0, y0 = _tables(R, G, T)
        Q = x0.shape[1]
        for P in (1, 4):
            for weighted in (False, True):
                for nan in (False, True):
                    rng = np.random.default_rng(T + 100 * P + 7 * weighted + 3 * nan)
                    tmap = rng.integers(0, Q, size=(P, T)).astype(np.int32)
                    w = rng.uniform(0.2, 3.0, size=T).astype(np.float32) if weighted else None
                    x, y = x0, y0
                    if nan and T:
                        y = y0.clone()
                        y[G // 2, int(tmap[P - 1, T // 2])] = float("nan")
                    out, mirror, _ = tfd_from_angles(x, y, tmap, weights=w, want_mirror=True)
                    xn, yn = x.cpu().numpy(), y.cpu().numpy()
                    for got, want in ((out, TR.tfd(xn, yn, tmap, w)), (mirror, TR.tfd(xn, yn, tmap, w, mirror=True))):
                        got = got.cpu().numpy()
                        assert got.dtype == np.float32 and got.shape == (R, G) and np.isfinite(got).all()
                        err = np.abs(got.astype(np.float64) - want).max()
                        worst = max(worst, err)
                        assert err <= TFD_ATOL, (T, P, weighted, nan, err)
                    if T == 0:
                        assert not out.any() and not mirror.any()
                    if nan and T and P == 1:                    # the broken torsion counts as the largest difference, pi
                        share = float(w[T // 2]) / float(w.astype(np.float64).sum()) if weighted else 1.0 / T
                        assert float(out[:, G // 2].min()) >= share - TFD_ATOL
    print("R = %d, G = %d: largest difference to the reference %.3e" % (R, G, worst))


@pytest.mark.parametrize("G", [1, 10, 33, 40])
def test_self_matrix_is_bitwise_symmetric_with_a_zero_diagonal(G):
    from agdiff_amd.torsions import tfd_from_angles
    for T in (1, 7, 70):
        ang = _tables(3, G, T)[1]
        rng = np.random.default_rng(G + T)
        tmap = rng.integers(0, ang.shape[1], size=(4, T)).astype(np.int32)
        tmap[0] = np.arange(T)
        w = rng.uniform(0.2, 3.0, size=T).astype(np.float32)
        for weights in (None, w):
            out, mirror, _ = tfd_from_angles(ang, ang, tmap, weights=weights, want_mirror=True)
            assert torch.equal(out, out.T) and torch.equal(mirror, mirror.T)
            assert not out.diagonal().any()


def test_one_direction_alone_is_not_the_tfd():
    from agdiff_amd.torsions import tfd_from_angles, torsion_table
    quads, tmap = torsion_table(_item(TR.biphenyl()))
    rng = np.random.default_rng(0)
    ang = _angles(rng.normal(size=(6, 12, 3)), quads)
    out = tfd_from_angles(ang, ang, tmap)[0].cpu().numpy().astype(np.float64)
    an = ang.cpu().numpy()
    one = TR.tfd(an, an, tmap, one_way=True)
    assert np.abs(out - TR.tfd(an, an, tmap)).max() <= TFD_ATOL
    assert np.abs(one - one.T).max() > 0.05 and np.abs(out - one).max() > 0.05 and (out <= one + TFD_ATOL).all()


# ------------------------------------------------------------------------------------------------ 3. bits
def _raw_tfd(x, y, tmap, thresh, want_out=True):
    """agdiff_tfd_matrix called directly with a bit buffer that is all ones before the call"""
    from agdiff_amd import _lib
    from agdiff_amd.ensemble import bits_pitch
    lib = _lib.load()
    R, G, Q = x.shape[0], y.shape[0], x.shape[1]
    tm = torch.from_numpy(np.ascontiguousarray(tmap, dtype=np.int32)).cuda()
    out = torch.full((R, G), -1.0, dtype=torch.float32, device="cuda") if want_out else None
    bits = torch.full((R, bits_pitch(G) // 8), -1, dtype=torch.int64, device="cuda")
    _lib.check(lib.agdiff_tfd_matrix(_lib.ptr(x), _lib.ptr(y), _lib.ptr(tm), _lib.ptr(None), R, G, Q, tm.shape[1], tm.shape[0], thresh,
                                     _lib.ptr(out), _lib.ptr(None), _lib.ptr(bits), _lib.stream_ptr()), "agdiff_tfd_matrix")
    return out, bits


@pytest.mark.parametrize("G", [1, 16, 17, 33, 100])
def test_bits_are_the_stored_matrix_under_the_threshold(G):
    from agdiff_amd.ensemble import bits_pitch, leader_prune, unpack_bits
    rng = np.random.default_rng(G)
    T = 3
    centres = rng.uniform(-np.pi, np.pi, size=(4, T))
    ang_np = centres[rng.integers(0, 4, size=G)] + 0.3 * rng.normal(size=(G, T))
    ang = torch.from_numpy(((ang_np + np.pi) % (2 * np.pi) - np.pi).astype(np.float32)).cuda()
    tmap = np.array([[0, 1, 2], [2, 1, 0]], dtype=np.int32)
    for thresh in (0.0, 0.15, 1.0):
        out, bits = _raw_tfd(ang, ang, tmap, thresh)
        assert bits.shape == (G, bits_pitch(G) // 8)
        adj = unpack_bits(bits, G)
        want = out <= thresh
        assert torch.equal(adj[:, :G], want) and not adj[:, G:].any()
        assert thresh < 1.0 or want.all()
        assert torch.equal(_raw_tfd(ang, ang, tmap, thresh, want_out=False)[1], bits)          # the bits do not need the matrix
        keep, leader, count, n_kept = leader_prune(bits, G)
        k0, l0, c0 = TR.leader_walk(want.cpu().numpy())
        assert np.array_equal(keep.cpu().numpy(), k0) and np.array_equal(leader.cpu().numpy(), l0)
        assert np.array_equal(count.cpu().numpy(), c0) and int(n_kept.item()) == int(k0.sum())
    # a rectangular matrix: R rows of the same layout
    R = min(5, G)
    out, bits = _raw_tfd(ang[:R].contiguous(), ang, tmap, 0.15)
    adj = unpack_bits(bits, R)
    assert bits.shape[0] == R and torch.equal(adj[:, :G], out <= 0.15) and not adj[:, G:].any()


# ------------------------------------------------------------------------------------------------ 4. by molecule
def test_butane_rotamers():
    """Three figures are pinned for butane: 1/3, then 2/3 proper and 0 mirror.  By the definition (delta / pi) they belong to the
    dihedrals 180, +120 and -120 degrees: 60 degrees apart is 1/3, 120 degrees 2/3.  With the gauche rotamers where chemistry puts
    them, at +-60 degrees, anti against gauche+ is 120 degrees apart as well and the definition gives 2/3, not 1/3.  Both sets are
    checked, each against the angles it was constructed with."""
    from agdiff_amd.torsions import tfd_matrix, tfd_self, torsion_table
    for side, to_anti in ((2 * np.pi / 3, 1 / 3), (np.pi / 3, 2 / 3)):
        want = np.array([np.pi, side, -side])
        pos = np.stack([TR.chain_positions([f]) for f in want]).astype(np.float32)
        item = _item(TR.alkane(4), pos_gen=pos, pos_ref=pos)
        assert torsion_table(item)[0].tolist() == [[0, 1, 2, 3]]
        ang = _angles(pos, [[0, 1, 2, 3]]).cpu().numpy()[:, 0].astype(np.float64)
        assert TR.circular_difference(ang, want).max() <= MOVE_ATOL
        out, bits = tfd_self(item)
        assert bits is None
        out = out.cpu().numpy()
        print("butane at 180, +-%.0f degrees: %r %r %r" % (np.degrees(side), out[0, 1], out[0, 2], out[1, 2]))
        assert abs(out[0, 1] - to_anti) <= MOL_ATOL and abs(out[0, 2] - to_anti) <= MOL_ATOL and abs(out[1, 2] - 2 / 3) <= MOL_ATOL
        proper, mirror = (m.cpu().numpy() for m in tfd_matrix(item, hands=True))
        assert np.array_equal(proper, out)
        assert abs(mirror[1, 2]) <= MOL_ATOL and abs(mirror[0, 0]) <= MOL_ATOL and abs(mirror[0, 1] - to_anti) <= MOL_ATOL
        assert abs(mirror[1, 1] - 2 / 3) <= MOL_ATOL


def _biphenyl_positions(rng, twist):
    r, d = 1.4, 1.5
    k = np.arange(6) * np.pi / 3
    ring_a = np.stack([-d / 2 - r + r * np.cos(k), r * np.sin(k), 0 * k], axis=1)
    ring_b = np.stack([d / 2 + r - r * np.cos(k), r * np.sin(k) * np.cos(twist), r * np.sin(k) * np.sin(twist)], axis=1)
    return np.concatenate([ring_a, ring_b]) + 0.05 * rng.normal(size=(12, 3))


def test_biphenyl_relabelled_by_a_ring_flip():
    from agdiff_amd.torsions import tfd_matrix
    rng = np.random.default_rng(3)
    x = np.stack([_biphenyl_positions(rng, t) for t in (0.7, -1.1, 2.0)]).astype(np.float32)
    flip = np.arange(12)
    flip[[7, 11, 8, 10]] = [11, 7, 10, 8]
    y = x[:, flip]
    with_symmetry = tfd_matrix(_item(TR.biphenyl(), pos_ref=x, pos_gen=y)).cpu().numpy()
    identity_only = tfd_matrix(_item(TR.biphenyl(), pos_ref=x, pos_gen=y, perms=np.arange(12, dtype=np.int32)[None])).cpu().numpy()
    assert (np.diag(with_symmetry) <= TFD_ATOL).all()
    assert (np.diag(identity_only) > 0.1).all()


# ------------------------------------------------------------------------------------------------ 5. through the interfaces
def _hexane_ensemble(rng, G):
    rot = np.array([np.pi, np.pi / 3, -np.pi / 3])
    tors = rot[rng.integers(0, 3, size=(G, 3))] + 0.05 * rng.normal(size=(G, 3))
    return np.stack([TR.chain_positions(t) for t in tors]).astype(np.float32)


def test_prune_by_tfd_equals_the_numpy_walk_and_the_rmsd_prune_is_what_it_was():
    from agdiff_amd.ensemble import leader_prune, prune_conformers, threshold_bits, _self_rmsd
    from agdiff_amd.torsions import tfd_self
    rng = np.random.default_rng(21)
    G = 40
    gen = _hexane_ensemble(rng, G)
    item = _item(TR.alkane(6), pos_gen=gen)
    out, bits = tfd_self(item, threshold=0.1)
    k0, l0, c0 = TR.leader_walk((out <= 0.1).cpu().numpy())
    assert 3 < k0.sum() < G                                  # (27 rotamers, 14 up to the chain's reversal: clusters form)
    for align in (False, True):
        res = prune_conformers(item, 0.1, align=align, metric="tfd")
        kept = np.nonzero(k0)[0]
        assert res["kept"].dtype == torch.int32 and np.array_equal(res["kept"].cpu().numpy(), kept)
        assert np.array_equal(res["leader"].cpu().numpy(), l0) and np.array_equal(res["count"].cpu().numpy(), c0[kept])
        assert res["pos"].shape == (kept.size, 6, 3) and np.array_equal(res["pos"][0].cpu().numpy(), gen[kept[0]])
        if not align:
            assert np.array_equal(res["pos"].cpu().numpy(), gen[kept])
    # metric="rmsd", the default: the bits of agdiff_rmsd_self and the walk over them, as before
    for kw in ({}, {"metric": "rmsd"}):
        res = prune_conformers(item, 0.5, align=False, **kw)
        _, _, _, rbits = _self_rmsd(item, "cuda", threshold=0.5, want_out=False)
        keep, leader, count, _ = leader_prune(rbits, G)
        kept = torch.nonzero(keep).reshape(-1)
        assert torch.equal(res["kept"], kept.to(torch.int32)) and torch.equal(res["leader"], leader)
        assert torch.equal(res["count"], count[kept]) and np.array_equal(res["pos"].cpu().numpy(), gen[kept.cpu().numpy()])
        rout, adj = threshold_bits(item, 0.5)
        k1, l1, _ = TR.leader_walk((rout <= 0.5).cpu().numpy())
        assert np.array_equal(keep.cpu().numpy(), k1) and np.array_equal(leader.cpu().numpy(), l1)


def test_covmat_over_tfd_equals_numpy_reductions_of_the_kernels_matrix():
    from agdiff_amd.evaluation import CovMatEvaluator, get_tfd_confusion_matrix
    rng = np.random.default_rng(33)
    items = [_item(TR.alkane(6), pos_ref=_hexane_ensemble(rng, 4), pos_gen=_hexane_ensemble(rng, 8), smiles="CCCCCC")]
    bx = np.stack([_biphenyl_positions(rng, t) for t in rng.uniform(-np.pi, np.pi, size=9)]).astype(np.float32)
    items.append(_item(TR.biphenyl(), pos_ref=bx[:3], pos_gen=bx[3:], smiles="c1ccccc1-c1ccccc1"))
    quiet = lambda *_: None
    res = CovMatEvaluator(metric="tfd", print_fn=quiet, either_hand=True)(items)
    plain = CovMatEvaluator(metric="tfd", print_fn=quiet)(items)
    thr = res.thresholds
    assert thr.shape == (60,) and abs(thr[0] - 0.01) < 1e-12 and abs(thr[-1] - 0.60) < 1e-12
    for k, item in enumerate(items):
        proper, mirror = (m.cpu().numpy().astype(np.float64) for m in get_tfd_confusion_matrix(item, hands=True))
        assert np.array_equal(proper, get_tfd_confusion_matrix(item).cpu().numpy().astype(np.float64))
        assert proper.shape == (len(item["pos_ref"]), len(item["pos_gen"])) and (proper >= 0).all() and (proper <= 1).all()
        for table, mat in ((res, proper), (plain, proper), (res.either_hand, np.minimum(proper, mirror))):
            assert np.array_equal(table.CoverageR[k], (mat.min(1)[:, None] <= thr[None, :]).mean(0))
            assert np.array_equal(table.CoverageP[k], (mat.min(0)[:, None] <= thr[None, :]).mean(0))
            assert table.MatchingR[k] == mat.min(1).mean() and table.MatchingP[k] == mat.min(0).mean()
        assert res.mirror_nearest[k] == float((mirror.min(0) < proper.min(0)).mean())
    assert 0.0 < plain.CoverageR[0].mean() < 1.0             # (the thresholds cut through the hexane rotamers)


def test_run_job_saves_kept_and_cluster_with_the_tfd_switch(tmp_path):
    from agdiff_amd import driver, get_model, qm9_model_config, synth
    from agdiff_amd.ensemble import prune_conformers
    m = get_model(qm9_model_config(num_diffusion_timesteps=8))
    m.load_state_dict(synth.synth_state_dict(m.state_dict()))
    m = m.to("cuda:0").eval()
    rng = np.random.default_rng(5)
    mols = []
    for i, n in enumerate((12, 17)):
        at, r, c, ty = synth.random_molecule(rng, n)
        mols.append(dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=ty, num_refs=6, name="mol%d" % i, index=i))
    confs = lambda num_refs: num_refs
    kw = dict(n_steps=4, step_lr=1e-6, w_global=1.0, clip=1000.0)
    quiet = lambda *_: None
    res = driver.run_job(m, mols, str(tmp_path / "tfd"), confs, 10 ** 6, kw, "cuda:0", log=quiet, prune_tfd=0.2)
    files = glob.glob(str(tmp_path / "tfd" / "samples_[0-9]*.npz"))
    assert len(files) == 1
    for z in (res, np.load(files[0]), np.load(str(tmp_path / "tfd" / "samples_all.npz"))):
        keys = set(z.keys() if isinstance(z, dict) else z.files)
        assert keys == {"%s_%d" % (k, i) for k in ("pos_gen", "name", "kept", "cluster") for i in range(2)}
        for x in mols:
            i = x["index"]
            pos = z["pos_gen_%d" % i]
            want = prune_conformers(dict(atom_type=x["atom_type"], pos_gen=pos, edge_index=x["edge_index"], edge_type=x["edge_type"]),
                                    0.2, align=False, metric="tfd")
            assert z["kept_%d" % i].dtype == np.int32 and z["cluster_%d" % i].dtype == np.int32
            assert np.array_equal(z["kept_%d" % i], want["kept"].cpu().numpy())
            assert np.array_equal(z["cluster_%d" % i], want["leader"].cpu().numpy()) and z["cluster_%d" % i].shape == (6,)


def test_command_lines_write_torsions_and_prune_by_tfd(tmp_path, capsys):
    from agdiff_amd import driver, ensemble, torsions
    rng = np.random.default_rng(9)
    at, bi, bt = TR.butane_with_hydrogens_and_hops()
    heavy = np.stack([TR.chain_positions([f]) for f in (np.pi, np.pi / 3, np.pi + 0.05, -np.pi / 3, np.pi / 3 - 0.05)])
    gen = np.concatenate([heavy, rng.normal(size=(5, 10, 3))], axis=1).astype(np.float32)
    driver.save_testset(str(tmp_path / "test.npz"), [dict(atom_type=at, edge_index=bi, edge_type=bt, num_refs=2, name="butane")])
    np.savez(str(tmp_path / "samples_all.npz"), pos_gen_0=gen)
    torsions.main(["--samples", str(tmp_path / "samples_all.npz"), "--testset", str(tmp_path / "test.npz"), "--out",
                   str(tmp_path / "torsions.npz")])
    z = np.load(str(tmp_path / "torsions.npz"))
    assert z["torsion_quads_0"].tolist() == [[0, 1, 2, 3]] and z["torsion_quads_0"].dtype == np.int32
    assert z["torsion_0"].shape == (5, 1) and z["torsion_0"].dtype == np.float32 and str(z["name_0"]) == "butane"
    want = np.array([np.pi, np.pi / 3, np.pi + 0.05, -np.pi / 3, np.pi / 3 - 0.05])
    assert TR.circular_difference(z["torsion_0"][:, 0].astype(np.float64), want).max() <= MOVE_ATOL
    out = ensemble.main(["--samples", str(tmp_path / "samples_all.npz"), "--testset", str(tmp_path / "test.npz"), "--prune-tfd", "0.1",
                         "--out", str(tmp_path / "pruned.npz")])
    assert "at TFD 0.100" in capsys.readouterr().out
    assert out["kept_0"].tolist() == [0, 1, 3] and out["cluster_0"].tolist() == [0, 1, 0, 3, 1] and out["count_0"].tolist() == [2, 2, 1]
    assert np.array_equal(out["pos_0"], gen[[0, 1, 3]])
