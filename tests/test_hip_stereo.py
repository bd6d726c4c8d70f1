"""GPU (MI355X): handedness.  agdiff_rmsd_matrix_hands (the RMSD to the mirror image out of the diagonalisation the proper RMSD
already pays for) against the oracle on point-inverted input; agdiff_chiral_verdict and agdiff_mirror_conformers against float64
numpy; fix_handedness through the evaluator, the prune and the sampling driver.

Tolerances: ATOL = 2e-5 Angstrom on RMSDs of order 1, as tests/test_hip_eval.py (positions are fp32, the kernel accumulates and
solves in fp64); 4 x 2^-24 x max |coordinate| for stored fp32 coordinates (twice the rounding of one stored value,
doubled); volumes 1e-6 of the largest |V| (fp64 arithmetic on fp32 inputs, one rounding to fp32 when stored: 6e-8)."""
import numpy as np
import pytest
import torch

from oracle import covmat_oracle as CO

pytestmark = pytest.mark.gpu
ATOL = 2e-5


def _mol(rng, n, R, G, frac_h=0.5):
    """the molecules of tests/test_hip_eval.py"""
    at = np.where(rng.random(n) < frac_h, 1, rng.choice([6, 7, 8], size=n))
    at[0] = 6
    base = rng.normal(size=(n, 3)) * 1.5
    ref = base[None] + 0.3 * rng.normal(size=(R, n, 3))
    gen = base[None] + 0.5 * rng.normal(size=(G, n, 3))
    return at, ref.astype(np.float32), gen.astype(np.float32)


def _inverted(gen, heavy):
    """every conformer negated about its heavy-atom centroid (float64)"""
    g = gen.astype(np.float64)
    return 2.0 * g[:, heavy].mean(1, keepdims=True) - g


@pytest.mark.parametrize("n,R,G,with_perms", [(23, 5, 10, False), (61, 17, 33, True), (9, 1, 1, True), (200, 3, 40, False)])
def test_two_matrices_against_the_oracle(n, R, G, with_perms):
    from agdiff_amd.evaluation import get_rmsd_confusion_matrix
    rng = np.random.default_rng(n)
    at, ref, gen = _mol(rng, n, R, G)
    heavy = np.nonzero(at != 1)[0]
    m = heavy.size
    data = {"atom_type": at, "pos_ref": ref.reshape(-1, 3), "pos_gen": gen.reshape(-1, 3)}
    perms = None
    if with_perms:
        perms = [np.arange(m)]
        for _ in range(4):
            p = np.arange(m)
            a, b = rng.choice(m, size=2, replace=False)
            p[[a, b]] = p[[b, a]]
            perms.append(p)
        data["perms"] = np.stack(perms)
        # one generated conformer is the relabelled AND inverted copy of a reference: only its mirror image, under the matching
        # mapping, gives ~0 (negation is exact in fp32)
        g0 = ref[0].copy()
        g0[heavy] = ref[0][heavy][perms[2]]
        gen[0] = -g0
        data["pos_gen"] = gen.reshape(-1, 3)
    single = get_rmsd_confusion_matrix(data)
    proper, mirror = get_rmsd_confusion_matrix(data, hands=True)
    assert proper.shape == mirror.shape == (R, G) and proper.is_cuda and mirror.is_cuda
    assert torch.equal(proper, single)
    want = CO.get_rmsd_confusion_matrix(ref, _inverted(gen, heavy), heavy, perms)
    err = np.abs(mirror.cpu().numpy() - want).max()
    print("mirror matrix: max |kernel - oracle| = %.3e Angstrom" % err)
    assert err < ATOL
    assert np.abs(proper.cpu().numpy() - CO.get_rmsd_confusion_matrix(ref, gen, heavy, perms)).max() < ATOL
    if with_perms:
        assert mirror[0, 0] < 1e-4 and proper[0, 0] > 0.1


def test_degenerate_sets():
    """(x, -x); planar and collinear pairs, which are their own mirror images; identical conformers"""
    from agdiff_amd.evaluation import get_rmsd_confusion_matrix
    rng = np.random.default_rng(3)
    n = 12
    at = np.full(n, 6)
    x = rng.normal(size=(n, 3)).astype(np.float32)
    a = 0.7
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=np.float32)
    planar = x.copy(); planar[:, 2] = 0.0
    planar2 = planar @ Rz.T + 0.1 * rng.normal(size=(n, 1)).astype(np.float32) * np.array([1.0, 1.0, 0.0], dtype=np.float32)
    line = np.zeros((n, 3), dtype=np.float32); line[:, 0] = np.arange(n)
    line2 = np.zeros((n, 3), dtype=np.float32); line2[:, 1] = 1.1 * np.arange(n)
    ref = np.stack([x, planar, line])
    gen = np.stack([x, -x, planar2, line2])
    item = {"atom_type": at, "pos_ref": ref, "pos_gen": gen}
    proper, mirror = (t.cpu().numpy() for t in get_rmsd_confusion_matrix(item, hands=True))
    assert np.isfinite(proper).all() and np.isfinite(mirror).all()
    assert torch.equal(get_rmsd_confusion_matrix(item), get_rmsd_confusion_matrix(item, hands=True)[0])
    assert mirror[0, 1] < 1e-5 and proper[0, 1] > 0.1              # (x, -x)
    assert proper[0, 0] < 1e-5 and mirror[0, 0] > 0.1              # identical
    assert abs(proper[1, 2] - mirror[1, 2]) < ATOL and proper[1, 2] > 0.01      # planar pair (not superposable: in-plane noise)
    assert abs(proper[2, 3] - mirror[2, 3]) < ATOL                 # collinear pair
    assert abs(proper[1, 3] - mirror[1, 3]) < ATOL and abs(proper[2, 2] - mirror[2, 2]) < ATOL      # planar x collinear
    want = CO.get_rmsd_confusion_matrix(ref, _inverted(gen, np.arange(n)), np.arange(n))
    assert np.abs(mirror - want).max() < ATOL


# ---- volumes and verdicts --------------------------------------------------------------------------------------------

_TETRA = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64) * (2.4 / (2.0 * np.sqrt(2.0)))
ROLES = ("plain", "inverted", "swapped", "coplanar", "nan")


def _centres_in(rng, n, C):
    """quads int32 [C, 4] (ascending atoms): n // 4 disjoint tetrahedra over randomly chosen atoms, and, past those, repeats of
    them in turn (C = 70 in 200 atoms).  Returns (quads, the atoms of the tetrahedra [n // 4, 4] in vertex order)."""
    T = n // 4
    atoms = rng.permutation(n)[:4 * T].reshape(T, 4)
    quads = np.sort(atoms[np.arange(C) % T], axis=1).astype(np.int32).reshape(C, 4)
    return quads, atoms


def _conformers(rng, n, G, atoms, roles):
    """[G, n, 3] float32: every tetrahedron a regular one of edge 2.4 A + 0.15 A normal noise, at its own place, the other atoms
    anywhere; then each conformer changed according to its role"""
    T = atoms.shape[0]
    where = rng.normal(size=(T, 3)) * 6.0
    pos = rng.normal(size=(G, n, 3)) * 3.0
    for t in range(T):
        pos[:, atoms[t]] = where[t] + _TETRA[None] + 0.15 * rng.normal(size=(G, 4, 3))
    pos = pos.astype(np.float32)
    for g, role in enumerate(roles):
        a = atoms[0]
        if role == "inverted":
            pos[g] = -pos[g]
        elif role == "swapped":
            pos[g, [a[0], a[1]]] = pos[g, [a[1], a[0]]]
        elif role == "coplanar":
            pos[g, a, 2] = pos[g, a[0], 2]                    # the same fp32 z for all four: the volume is exactly 0
        elif role == "nan":
            pos[g, a[2], 1] = np.nan
    return pos


def _target(n, atoms, quads):
    """the parity of every quad in the noise-free tetrahedra: the hand of every plain conformer"""
    from agdiff_amd.stereo import signed_volumes
    ideal = np.zeros((1, n, 3))
    for t in range(atoms.shape[0]):
        ideal[0, atoms[t]] = _TETRA
    return np.sign(signed_volumes(ideal, quads)[0]).astype(np.int8)


def _verdicts(vol, target):
    """numpy restatement: vol float64 [G, C], target [C]"""
    par = np.where(np.isfinite(vol), np.sign(vol), 0.0)
    out = np.ones(vol.shape[0], dtype=np.int32)
    chk = np.asarray(target) != 0
    for g in range(vol.shape[0]):
        p, t = par[g][chk], np.asarray(target)[chk]
        if p.size == 0:
            continue
        if (p == 0).any() or ((p == t).any() and (p == -t).any()):
            out[g] = 0
        elif (p == -t).all():
            out[g] = -1
    return out


@pytest.mark.parametrize("n", [5, 14, 200])
def test_volumes_and_verdicts(n):
    from agdiff_amd.stereo import chiral_verdict, signed_volumes
    rng = np.random.default_rng(100 + n)
    for G in (1, 17, 64, 65):
        for C in (0, 1, 2, 70):
            quads, atoms = _centres_in(rng, n, C)
            roles = [ROLES[(g + C) % len(ROLES)] for g in range(G)]
            pos = _conformers(rng, n, G, atoms, roles)
            vol64 = signed_volumes(pos, quads)
            first = np.array([set(q.tolist()) == set(atoms[0].tolist()) for q in quads], dtype=bool)      # centres on tetrahedron 0
            clean = np.ones((G, C), dtype=bool)
            for g, role in enumerate(roles):
                if role in ("coplanar", "nan"):
                    clean[g, first] = False
            # a condition on the INPUTS: no sign the test relies on is in doubt
            assert (np.abs(vol64[clean]) > 0.05).all()
            plain = [g for g, r in enumerate(roles) if r == "plain"]
            target = _target(n, atoms, quads)
            assert all((np.sign(vol64[g]) == target).all() for g in plain)
            t = torch.from_numpy(pos).cuda()
            verdict, vol = chiral_verdict(t, quads, target)
            assert verdict.dtype == torch.int32 and verdict.shape == (G,) and vol.shape == (G, C) and vol.dtype == torch.float32
            got = vol.cpu().numpy().astype(np.float64)
            if C:
                scale = np.abs(vol64[np.isfinite(vol64)]).max()
                assert np.array_equal(np.isnan(got), np.isnan(vol64))
                assert np.nanmax(np.abs(got - vol64), initial=0.0) <= 1e-6 * scale
            want = _verdicts(vol64, target)
            assert np.array_equal(verdict.cpu().numpy(), want), (G, C)
            distinct = atoms.shape[0]
            for g, role in enumerate(roles):
                if C == 0 or role == "plain":
                    assert want[g] == 1
                elif role == "inverted":
                    assert want[g] == -1
                elif role in ("coplanar", "nan"):
                    assert want[g] == 0
                elif role == "swapped" and C >= 2 and distinct >= 2:
                    assert want[g] == 0
            # nothing to check: + 1 for everyone; without the optional output
            none, no_vol = chiral_verdict(t, quads, np.zeros(C, dtype=np.int8), want_vol=False)
            assert no_vol is None and (none == 1).all()


def _bar(x):
    return 4.0 * 2.0 ** -24 * float(np.abs(x).max())


@pytest.mark.parametrize("n,G", [(5, 3), (14, 65), (200, 17)])
def test_mirror_in_place(n, G):
    from agdiff_amd.stereo import chiral_verdict, mirror_conformers
    rng = np.random.default_rng(n)
    quads, atoms = _centres_in(rng, n, min(2, n // 4))
    roles = [ROLES[g % 2] for g in range(G)]                   # plain, inverted, plain, ...
    pos = _conformers(rng, n, G, atoms, roles) + np.float32(3.0)       # (off the origin: the centroid matters)
    target = _target(n, atoms, quads)
    t = torch.from_numpy(pos).cuda()
    verdict, _ = chiral_verdict(t, quads, target)
    flags = (verdict < 0)
    assert flags.cpu().numpy().tolist() == [r == "inverted" for r in roles]
    out = mirror_conformers(t.clone(), flags)
    got = out.cpu().numpy()
    f = flags.cpu().numpy()
    p64 = pos.astype(np.float64)
    want = 2.0 * p64.mean(1, keepdims=True) - p64
    bar = _bar(pos)
    assert torch.equal(out[~flags], t[~flags])
    if f.any():
        assert np.abs(got[f] - want[f]).max() <= bar
        dist = lambda p: np.linalg.norm(p[:, :, None, :] - p[:, None, :, :], axis=-1)
        assert np.abs(dist(got[f].astype(np.float64)) - dist(p64[f])).max() <= bar
        assert np.abs(got[f].astype(np.float64).mean(1) - p64[f].mean(1)).max() <= bar       # the centring is kept
    after, _ = chiral_verdict(out, quads, target)
    assert (after >= 0).all() and (after == 1).all()
    twice = mirror_conformers(out.clone(), flags)
    assert np.abs(twice.cpu().numpy() - pos).max() <= bar
    assert torch.equal(twice[~flags], t[~flags])
    # no flag set: nothing is written
    assert torch.equal(mirror_conformers(t.clone(), torch.zeros(G, dtype=torch.int32)), t)


# ---- end to end, no model ----------------------------------------------------------------------------------------------

def _dichlorobutane():
    """C0 H3 - C1 HCl - C2 HCl - C3 H3; Cl4 on C1, Cl5 on C2; H6-8 on C0, H9 on C1, H10 on C2, H11-13 on C3: centres C1, C2"""
    bonds = [(0, 1), (1, 2), (2, 3), (1, 4), (2, 5), (0, 6), (0, 7), (0, 8), (1, 9), (2, 10), (3, 11), (3, 12), (3, 13)]
    bi = np.array(bonds + [(j, i) for i, j in bonds]).T
    return np.array([6, 6, 6, 6, 17, 17] + [1] * 8), bi, np.ones(bi.shape[1], dtype=np.int64)


def _one_handed_item(R=4, seed=17):
    """references: R = 4 unrelated geometries that share the hand (+, +) at both centres with |V| > 0.5; generated: 2 R copies with
    0.02 A noise, of references (0, 1, 1, 2, 3, 0, 2, 3): number 1 a diastereomer (Cl4 and H9 exchanged: centre C1 alone flips),
    numbers 2, 4, 5, 6 point-inverted.  The first R fixable ones, (0, 2, 3, 4), hold one copy of every reference, two of them as
    mirror images; references 0, 2 and 3 are there in both hands."""
    from agdiff_amd.stereo import signed_volumes, tetrahedral_centres
    assert R == 4
    at, bi, bt = _dichlorobutane()
    centre, quads = tetrahedral_centres(at, bi, bt)
    assert centre.tolist() == [1, 2]
    rng = np.random.default_rng(seed)
    refs = []
    while len(refs) < R:
        x = rng.normal(size=(len(at), 3)) * 1.6
        v = signed_volumes(x[None], quads)[0]
        if (v > 0.5).all():
            refs.append(x)
    ref = np.stack(refs).astype(np.float32)
    gen = np.stack([ref[k] + 0.02 * rng.normal(size=ref[0].shape) for k in (0, 1, 1, 2, 3, 0, 2, 3)]).astype(np.float32)
    hand = np.ones(2 * R, dtype=np.int32)
    for k in (2, 4, 5, 6):
        gen[k], hand[k] = -gen[k], -1
    gen[1, [4, 9]] = gen[1, [9, 4]]
    hand[1] = 0
    stereo = np.zeros(len(at), dtype=np.int8)
    stereo[centre] = 1
    item = {"atom_type": at, "bond_index": bi, "bond_type": bt, "stereo": stereo, "pos_ref": ref, "smiles": "CC(Cl)C(Cl)C"}
    return item, gen, hand


def test_fix_then_evaluate_equals_the_either_hand_table_and_the_prune_keeps_no_more():
    """ratio = 1: the evaluator scores the first R generated conformers of what it is given, here of the 2 R - 1 fixable ones --
    (0, 2, 3, 4) at R = 4: one copy of every reference, those of references 1 and 3 as mirror images, so the raw first table
    differs from the other two.  (The equality needs every reference to have its own copy among them: a reference without one
    could be nearest to the WRONG hand of an unrelated conformer, which the either-hand table admits and the fix does not.)"""
    from agdiff_amd.ensemble import prune_conformers
    from agdiff_amd.evaluation import CovMatEvaluator
    from agdiff_amd.stereo import fix_handedness, handedness
    item, gen, hand = _one_handed_item()
    verdict, vol = handedness(item, gen)
    assert verdict.cpu().numpy().tolist() == hand.tolist() and vol.shape == (gen.shape[0], 2)
    fixed = torch.from_numpy(gen).cuda()
    before = fix_handedness(item, fixed)
    assert before.cpu().numpy().tolist() == hand.tolist()
    assert handedness(item, fixed)[0].cpu().numpy().tolist() == np.abs(hand).tolist()
    fixable = np.nonzero(hand != 0)[0]
    quiet = lambda s: None
    raw = CovMatEvaluator(ratio=1, either_hand=True, print_fn=quiet)([dict(item, pos_gen=gen[fixable])])
    mended = CovMatEvaluator(ratio=1, print_fn=quiet)([dict(item, pos_gen=fixed[torch.from_numpy(fixable).cuda()])])
    assert "either_hand" not in mended and "mirror_nearest" not in mended
    assert np.array_equal(mended.CoverageR, raw.either_hand.CoverageR)
    assert abs(mended.MatchingR[0] - raw.either_hand.MatchingR[0]) < ATOL
    assert np.array_equal(mended.CoverageP, raw.either_hand.CoverageP)
    assert abs(mended.MatchingP[0] - raw.either_hand.MatchingP[0]) < ATOL
    assert raw.MatchingR[0] > raw.either_hand.MatchingR[0] + 0.1           # handedness cost the raw set something
    assert raw.mirror_nearest.tolist() == [0.5]                             # (0, 2, 3, 4): conformers 3 and 4 are mirror images
    # copies of one reference in one hand: < 0.1 A; everything else, a reference against its own mirror image included: > 0.5 A
    plain = prune_conformers(dict(item, pos_gen=gen), 0.3, align=False)
    caller = torch.from_numpy(gen).cuda()
    mirrored = prune_conformers(dict(item, pos_gen=caller), 0.3, align=False, fix_handedness=True)
    assert torch.equal(caller.cpu(), torch.from_numpy(gen))                  # the caller's tensor is not written
    assert "hand" not in plain and mirrored["hand"].cpu().numpy().tolist() == hand.tolist()
    assert mirrored["kept"].shape[0] <= plain["kept"].shape[0]
    # raw: nothing superposes; fixed: 5, 6 and 7 fall to 0, 3 and 4 -- the R references + the diastereomer are left
    assert (mirrored["kept"].cpu().numpy().tolist(), plain["kept"].shape[0]) == ([0, 1, 2, 3, 4], 8)
    with pytest.raises(ValueError, match="stereo"):
        prune_conformers({k: v for k, v in dict(item, pos_gen=gen).items() if k != "stereo"}, 0.3, fix_handedness=True)


# ---- the driver --------------------------------------------------------------------------------------------------------

def _gpu_model(cfg, head_scale=1e-3, precision="f16x3"):
    """the synthetic checkpoint of tests/test_hip_driver_dist.py"""
    from agdiff_amd import get_model
    from oracle import agdiff_oracle as O
    sd = O.synth_state_dict_for(cfg, head_scale=head_scale)
    m = get_model(cfg)
    m.precision = precision
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    return m.to("cuda:0").eval(), sd


def _two_tagged_molecules():
    from agdiff_amd import synth
    mols = []
    # C(H)(N)(O)F, and 2,3-difluorobutane: C0 - C1 F - C2 F - C3 with hydrogens
    graphs = [([6, 1, 7, 8, 9], [(0, 1), (0, 2), (0, 3), (0, 4)], [0]),
              ([6, 6, 6, 6, 9, 9] + [1] * 8,
               [(0, 1), (1, 2), (2, 3), (1, 4), (2, 5), (0, 6), (0, 7), (0, 8), (1, 9), (2, 10), (3, 11), (3, 12), (3, 13)], [1, 2])]
    for i, (atoms, bonds, centres) in enumerate(graphs):
        at = np.array(atoms, dtype=np.int64)
        src = np.array([a for a, b in bonds] + [b for a, b in bonds])
        dst = np.array([b for a, b in bonds] + [a for a, b in bonds])
        r, c, ty = synth.extend_graph_order_np(len(at), src, dst, np.ones(src.shape[0], dtype=np.int64), order=3)
        stereo = np.zeros(len(at), dtype=np.int8)
        stereo[centres] = 1
        mols.append(dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=ty, num_refs=3 + i, name="mol%d" % i, index=i, stereo=stereo))
    return mols


def test_driver_writes_hand_and_leaves_the_plain_job_alone(tmp_path):
    from agdiff_amd import driver, qm9_model_config
    from agdiff_amd.stereo import handedness
    cfg = qm9_model_config(num_diffusion_timesteps=10)
    m, _ = _gpu_model(cfg)
    mols = _two_tagged_molecules()
    confs = driver.num_confs("2x")
    kw = dict(n_steps=10, step_lr=1e-6, w_global=1.0, global_start_sigma=0.5, clip=1000.0)
    logs = []
    run = lambda name, **extra: driver.run_job(m, [dict(x) for x in mols], str(tmp_path / name), confs, 100000, kw, "cuda:0",
                                               log=logs.append, noise="counter", seed=5, **extra)
    off, off2, on = run("off"), run("off2"), run("on", fix_handedness=True)
    assert sorted(off) == sorted(off2) == ["name_0", "name_1", "pos_gen_0", "pos_gen_1"]
    assert sorted(on) == ["hand_0", "hand_1", "name_0", "name_1", "pos_gen_0", "pos_gen_1"]
    n_mirrored = 0
    for x in mols:
        i, g, n = x["index"], confs(x["num_refs"]), len(x["atom_type"])
        assert off["pos_gen_%d" % i].tobytes() == off2["pos_gen_%d" % i].tobytes()
        hand = on["hand_%d" % i]
        assert hand.dtype == np.int8 and hand.shape == (g,) and set(hand.tolist()) <= {-1, 0, 1}
        raw, fixed = off["pos_gen_%d" % i], on["pos_gen_%d" % i]
        assert fixed.shape == raw.shape == (g, n, 3) and fixed.dtype == raw.dtype == np.float32
        # the verdict that was written is the raw conformers' verdict; the others are the sampler's bytes
        assert handedness(x, raw)[0].cpu().numpy().tolist() == hand.tolist()
        assert fixed[hand >= 0].tobytes() == raw[hand >= 0].tobytes()
        after = handedness(x, fixed)[0].cpu().numpy()
        assert (after >= 0).all() and (after[hand < 0] == 1).all()
        n_mirrored += int((hand < 0).sum())
    assert [l for l in logs if "%d conformers were mirror images" % n_mirrored in l]
    assert len([l for l in logs if "mirror images" in l]) == 1              # only the run with the switch says so
    with pytest.raises(ValueError, match="stereo"):
        driver.run_job(m, [{k: v for k, v in x.items() if k != "stereo"} for x in mols], str(tmp_path / "untagged"), confs, 100000, kw,
                       "cuda:0", log=logs.append, fix_handedness=True)
