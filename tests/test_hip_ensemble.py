"""GPU (MI355X): conformer ensembles (agdiff_amd.ensemble; csrc/eval.hip: k_rmsd_self, k_leader_prune, k_align_conformers)
against the oracle (oracle/covmat_oracle.py: Kabsch by SVD in float64), a Python leader loop and a numpy Kabsch alignment.
RMSD tolerance: that of tests/test_hip_eval.py, 2e-5 absolute in Angstrom -- the pair arithmetic is the same."""
import functools
import glob

import numpy as np
import pytest
import torch

from oracle import covmat_oracle as CO

pytestmark = pytest.mark.gpu
ATOL = 2e-5
# The aligned coordinates against a float64 numpy Kabsch of the same fp32 inputs: the largest deviation measured on the MI355X
# over the shapes of test_alignment_matches_a_float64_kabsch was 2.24e-7 Angstrom (n = 61; 1.18e-7 at n = 8, 2.05e-7 at n = 23)
# -- exactly what rounding the float64 reference itself to fp32 loses, coordinates reaching 6.3 Angstrom.  The bar is 4 x the
# measured figure, far below the project's parity bar of 1e-4.
ALIGN_MEASURED = 2.24e-7
ALIGN_ATOL = 4 * ALIGN_MEASURED
assert ALIGN_ATOL <= 1e-4

SHAPES = [(9, 1, True), (20, 16, False), (20, 17, True), (20, 37, False), (45, 65, True)]
# {id, (0 1), (2 3), (0 1)(2 3)} on the heavy atoms (in heavy-atom order)
GROUP4 = lambda m: np.stack([np.r_[a, b, np.arange(4, m)] for a in ([0, 1], [1, 0]) for b in ([2, 3], [3, 2])]).astype(np.int32)


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _atom_types(rng, n, frac_h=0.5):
    at = np.where(rng.random(n) < frac_h, 1, rng.choice([6, 7, 8], size=n))
    at[:4] = 6                      # (the four atoms the group acts on)
    return at


def _relabel(x, heavy, perm):
    """the same structure with heavy atom k sitting where heavy atom perm[k] sat"""
    y = x.copy()
    y[heavy] = x[heavy][perm]
    return y


def _moved(rng, x):
    return x @ _rotation(rng).T + rng.normal(size=3)


@functools.lru_cache(maxsize=None)
def _case(n, G, with_perms):
    """(atom_type, gen fp32 [G, n, 3], heavy, perms or None, oracle matrix: upper triangle, mirrored) -- computed once"""
    rng = np.random.default_rng(1000 * n + G)
    at = _atom_types(rng, n)
    heavy = np.nonzero(at != 1)[0]
    perms = GROUP4(heavy.size) if with_perms else None
    base = rng.normal(size=(n, 3)) * 1.5
    gen = base[None] + 0.2 * rng.normal(size=(G, n, 3))
    twins = []
    for a, b in ((3, 0), (G - 1, 5), (G - 3, 2)):          # conformer a := conformer b relabelled by a group element, moved rigidly
        if b < a < G:
            g = perms[1 + len(twins) % 3] if with_perms else np.arange(heavy.size)
            gen[a] = _moved(rng, _relabel(gen[b], heavy, g))
            twins.append((b, a))
    gen = gen.astype(np.float32)
    want = np.zeros((G, G))
    for i in range(G):
        for j in range(i + 1, G):
            want[i, j] = want[j, i] = CO.best_rmsd(gen[i], gen[j], heavy, perms)
    want.setflags(write=False)
    return at, gen, heavy, perms, want, tuple(twins)


def _item(at, gen, perms=None):
    d = {"atom_type": at, "pos_gen": gen.reshape(-1, 3)}
    if perms is not None:
        d["perms"] = perms
    return d


def _leader_loop(adj):
    """the greedy leader algorithm in conformer order on a boolean adjacency matrix"""
    G = adj.shape[0]
    kept = np.zeros(G, dtype=bool)
    leader = np.zeros(G, dtype=np.int32)
    count = np.zeros(G, dtype=np.int32)
    for i in range(G):
        hits = np.nonzero(adj[i, :i] & kept[:i])[0]
        if hits.size == 0:
            kept[i], leader[i] = True, i
        else:
            leader[i] = hits[0]
        count[leader[i]] += 1
    return kept.astype(np.int32), leader, count


# ------------------------------------------------------------------------------------------------ 1. the self matrix
@pytest.mark.parametrize("n,G,with_perms", SHAPES)
def test_self_matrix_matches_oracle(n, G, with_perms):
    from agdiff_amd.ensemble import self_rmsd_matrix
    from agdiff_amd.evaluation import get_rmsd_confusion_matrix
    at, gen, heavy, perms, want, twins = _case(n, G, with_perms)
    got = self_rmsd_matrix(_item(at, gen, perms))
    assert got.shape == (G, G) and got.is_cuda and got.dtype == torch.float32
    assert torch.equal(got, got.T)
    assert bool((torch.diagonal(got) == 0).all())
    g = got.cpu().numpy()
    err = np.abs(g - want).max()
    print("self matrix n=%d G=%d perms=%s: max |got - oracle| = %.3e" % (n, G, with_perms, err))
    assert err < ATOL
    for b, a in twins:
        assert g[b, a] < 1e-4
    assert G < 4 or twins
    full = get_rmsd_confusion_matrix(dict(_item(at, gen, perms), pos_ref=gen.reshape(-1, 3))).cpu().numpy()
    assert np.abs(g - full).max() < ATOL
    # csrc/eval.hip, header: the two kernels agree bit for bit because they call one pair routine.  The self kernel computes (i, j),
    # i < j, with x = conformer i; the matrix kernel's x is the generated conformer, its column: that is entry [j][i] of the full matrix
    iu = np.triu_indices(G, 1)
    assert np.array_equal(g[iu].view(np.int32), full.T[iu].view(np.int32))


# ------------------------------------------------------------------------------------------------ 2. the threshold bits
@pytest.mark.parametrize("n,G,with_perms", SHAPES)
def test_threshold_bits_are_the_stored_matrix_under_the_threshold(n, G, with_perms):
    from agdiff_amd.ensemble import bits_pitch, threshold_bits
    at, gen, heavy, perms, want, twins = _case(n, G, with_perms)
    seen = set()
    for thr in (0.0, 0.5, 1e9):
        out, adj = threshold_bits(_item(at, gen, perms), thr)
        assert adj.shape == (G, 8 * bits_pitch(G))
        assert torch.equal(adj[:, :G], out <= thr)
        assert bool(torch.diagonal(adj[:, :G]).all())
        assert not bool(adj[:, G:].any())
        seen.add(int(adj.sum()))
    assert G == 1 or len(seen) == 3       # (the three thresholds cut differently: identity only, a mix, everything)


# ------------------------------------------------------------------------------------------------ 3. the leader kernel alone
def _pack(adj):
    from agdiff_amd.ensemble import bits_pitch
    G = adj.shape[0]
    wide = np.zeros((G, 8 * bits_pitch(G)), dtype=np.uint8)
    wide[:, :G] = adj
    return torch.from_numpy(np.packbits(wide, axis=1, bitorder="little").view(np.int64).copy()).cuda()


@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, 130, 1000, 4096])
def test_leader_prune_equals_the_python_loop(G):
    from agdiff_amd.ensemble import leader_prune
    rng = np.random.default_rng(G)
    for density in (0.0, 0.02, 0.5, 1.0):
        adj = np.triu(rng.random((G, G)) < density, 1)
        adj = adj | adj.T | np.eye(G, dtype=bool)
        keep, leader, count, n_kept = leader_prune(_pack(adj), G)
        k0, l0, c0 = _leader_loop(adj)
        assert np.array_equal(keep.cpu().numpy(), k0), density
        assert np.array_equal(leader.cpu().numpy(), l0), density
        assert np.array_equal(count.cpu().numpy(), c0), density
        assert int(n_kept.item()) == int(k0.sum())
        assert density > 0 or k0.all()
        assert density < 1 or k0.sum() == 1


def test_leader_prune_refuses_more_conformers_than_one_wave_holds():
    from agdiff_amd import _lib
    from agdiff_amd.ensemble import bits_pitch, leader_prune
    G = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"] + 1
    assert G == 4097
    bits = torch.zeros((G, bits_pitch(G) // 8), dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.AgdiffLimitError):
        leader_prune(bits, G)
    with pytest.raises(_lib.AgdiffLimitError):
        from agdiff_amd.ensemble import prune_conformers
        prune_conformers({"atom_type": np.array([6, 6]), "pos_gen": np.zeros((G, 2, 3), np.float32)}, 0.5)


# ------------------------------------------------------------------------------------------------ 4. end to end, clustered
@pytest.mark.parametrize("n,K,G", [(20, 4, 37), (45, 7, 150)])
def test_prune_recovers_planted_clusters(n, K, G):
    from agdiff_amd.ensemble import prune_conformers
    rng = np.random.default_rng(7 * n + G)
    at = _atom_types(rng, n)
    heavy = np.nonzero(at != 1)[0]
    perms = GROUP4(heavy.size)
    centres = [rng.normal(size=(n, 3)) * 1.5 for _ in range(K)]
    label = np.r_[rng.permutation(K), rng.integers(K, size=G - K)]
    rng.shuffle(label)
    gen = np.stack([_moved(rng, _relabel(centres[c] + 0.03 * rng.normal(size=(n, 3)), heavy, perms[rng.integers(4)]))
                    for c in label]).astype(np.float32)
    want = np.zeros((G, G))
    for i in range(G):
        for j in range(i + 1, G):
            want[i, j] = want[j, i] = CO.best_rmsd(gen[i], gen[j], heavy, perms)
    thr = 0.5
    off = want[np.triu_indices(G, 1)]
    same = (label[:, None] == label[None, :])[np.triu_indices(G, 1)]
    print("clusters n=%d: largest intra %.3f, smallest inter %.3f" % (n, off[same].max(), off[~same].min()))
    assert np.abs(off - thr).min() >= 0.1            # the result cannot hinge on rounding
    assert off[same].max() < thr < off[~same].min()
    res = prune_conformers({"atom_type": at, "pos_gen": gen, "perms": perms}, thr, align=True)
    first = np.array([np.nonzero(label == c)[0][0] for c in range(K)])
    kept = res["kept"].cpu().numpy()
    assert kept.dtype == np.int32 and np.array_equal(kept, np.sort(first))
    assert np.array_equal(res["leader"].cpu().numpy(), first[label])
    assert np.array_equal(res["count"].cpu().numpy(), np.array([(label == label[k]).sum() for k in kept]))
    assert res["pos"].shape == (K, n, 3)
    assert torch.equal(res["pos"][0].cpu(), torch.from_numpy(gen[kept[0]]))
    # the identity mapping alone does not see the relabelled members as duplicates
    plain = prune_conformers({"atom_type": at, "pos_gen": gen}, thr, align=False)
    assert plain["kept"].shape[0] > K


# ------------------------------------------------------------------------------------------------ 5. a chain
def test_chain_is_pruned_by_leaders_not_by_components_or_all_pairs():
    """0 - 1 - 2 - 3 - 4 - 5 with neighbours 0.29 apart and threshold 0.45: connected components would keep one conformer,
    'drop whatever is near anything earlier' would keep [0]; the leader rule keeps [0, 2, 4]."""
    from agdiff_amd.ensemble import prune_conformers, self_rmsd_matrix
    rng = np.random.default_rng(21)
    n = 14
    A = rng.normal(size=(n, 3)) * 1.5
    D = rng.normal(size=(n, 3))
    D -= D.mean(0)
    D *= 0.3 / np.sqrt((D * D).sum() / n)
    pos = np.stack([(A + t * D) @ _rotation(rng).T for t in range(6)]).astype(np.float32)
    at = np.full(n, 6)
    want = CO.get_rmsd_confusion_matrix(pos, pos, np.arange(n))
    thr = 0.45
    off = want[np.triu_indices(6, 1)]
    print("chain: neighbours %.3f, next %.3f, nearest to the threshold %.3f" % (want[0, 1], want[0, 2], np.abs(off - thr).min()))
    assert np.abs(off - thr).min() >= 0.1
    assert np.abs(self_rmsd_matrix({"atom_type": at, "pos_gen": pos}).cpu().numpy() - want).max() < ATOL
    res = prune_conformers({"atom_type": at, "pos_gen": pos}, thr)
    assert res["kept"].cpu().tolist() == [0, 2, 4]
    assert res["leader"].cpu().tolist() == [0, 0, 2, 2, 4, 4]
    assert res["count"].cpu().tolist() == [2, 2, 2]


# ------------------------------------------------------------------------------------------------ 6. symmetry from bonds
def test_bonds_make_the_prune_symmetry_aware():
    """toluene (the item of tests/test_hip_eval.py): a structure and its ring-mirror relabelling are one conformer when the
    item carries its bonds, two without them"""
    from agdiff_amd.ensemble import prune_conformers
    rng = np.random.default_rng(11)
    ring = [(i, (i + 1) % 6, 12) for i in range(6)]
    atoms = [6] * 7 + [1] * 8
    bonds = ring + [(0, 6, 1)] + [(1 + k, 7 + k, 1) for k in range(5)] + [(6, 12 + k, 1) for k in range(3)]
    sigma = np.array([0, 5, 4, 3, 2, 1, 6])
    at = np.array(atoms)
    heavy = np.nonzero(at != 1)[0]
    bi = np.array([[i, j] for i, j, _ in bonds] + [[j, i] for i, j, _ in bonds]).T
    bt = np.array([t for _, _, t in bonds] * 2)
    x = (rng.normal(size=(at.size, 3)) * 1.4).astype(np.float32)
    gen = np.stack([x, _relabel(x, heavy, sigma)])
    item = {"atom_type": at, "pos_gen": gen}
    sym = prune_conformers(dict(item, bond_index=bi, bond_type=bt), 0.5)
    assert sym["kept"].cpu().tolist() == [0] and sym["leader"].cpu().tolist() == [0, 0] and sym["count"].cpu().tolist() == [2]
    plain = prune_conformers(item, 0.5)
    assert plain["kept"].cpu().tolist() == [0, 1] and plain["leader"].cpu().tolist() == [0, 1]
    assert plain["count"].cpu().tolist() == [1, 1]


# ------------------------------------------------------------------------------------------------ 7. alignment
def _kabsch_align(x, target, sel):
    """float64 Kabsch (SVD, proper rotation) of x onto target over the atoms `sel`, applied to every atom"""
    x, target = np.asarray(x, np.float64), np.asarray(target, np.float64)
    cx, ct = x[sel].mean(0), target[sel].mean(0)
    H = (x[sel] - cx).T @ (target[sel] - ct)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    R = (U @ np.diag([1.0, 1.0, d]) @ Vt).T
    return (x - cx) @ R.T + ct


def _direct_rmsd(a, b, sel):
    d = np.asarray(a, np.float64)[sel] - np.asarray(b, np.float64)[sel]
    return float(np.sqrt((d * d).sum() / len(sel)))


def _pair_distances(x):
    x = np.asarray(x, np.float64)
    return np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))


@pytest.mark.parametrize("n", [8, 23, 61])
def test_alignment_matches_a_float64_kabsch(n):
    """Largest deviation of the aligned coordinates from the float64 reference measured on the MI355X over n = 8, 23, 61:
    2.24e-7 Angstrom (ALIGN_MEASURED; 1.18e-7, 2.05e-7, 2.24e-7 per shape); the bar is 4 x that = 8.96e-7."""
    from agdiff_amd.ensemble import align_conformers
    rng = np.random.default_rng(n)
    at = _atom_types(rng, n)
    heavy = np.nonzero(at != 1)[0]
    G = 6
    target = (rng.normal(size=(n, 3)) * 1.5).astype(np.float32)
    pos = np.stack([_moved(rng, target + 0.3 * rng.normal(size=(n, 3))) for _ in range(G)]).astype(np.float32)
    got, rmsd = align_conformers(pos, at, target)
    assert got.shape == (G, n, 3) and rmsd.shape == (G,)
    got, rmsd = got.cpu().numpy(), rmsd.cpu().numpy()
    want = np.stack([_kabsch_align(p, target, heavy) for p in pos])
    dev = np.abs(got - want).max()
    print("alignment n=%d: max |aligned - float64 Kabsch| = %.3e Angstrom" % (n, dev))
    assert dev <= ALIGN_ATOL
    for g in range(G):
        direct = _direct_rmsd(got[g], target, heavy)
        assert abs(direct - CO.kabsch_rmsd(pos[g][heavy], target[heavy])) < ATOL
        assert abs(rmsd[g] - direct) < 1e-6
        assert np.abs(_pair_distances(got[g]) - _pair_distances(pos[g])).max() < 1e-5


def test_alignment_of_degenerate_geometries():
    """identical, rigidly moved, planar and collinear inputs reach the optimal RMSD; a mirror image is not superposed"""
    from agdiff_amd.ensemble import align_conformers
    rng = np.random.default_rng(3)
    n = 12
    at = np.full(n, 6)
    sel = np.arange(n)
    x = rng.normal(size=(n, 3)).astype(np.float32)
    planar = x.copy(); planar[:, 2] = 0.0
    line = np.zeros((n, 3), dtype=np.float32); line[:, 0] = 0.5 * np.arange(n)
    line2 = np.zeros((n, 3), dtype=np.float32); line2[:, 1] = 0.55 * np.arange(n)
    for name, target, others in (
            ("generic", x, [x, _moved(rng, x), x * np.array([1.0, 1.0, -1.0])]),
            ("planar", planar, [planar, _moved(rng, planar), _moved(rng, planar + 0.1 * rng.normal(size=(n, 3)))]),
            ("collinear", line, [line, _moved(rng, line), line2, _moved(rng, line2)])):
        pos = np.stack(others).astype(np.float32)
        got, rmsd = align_conformers(pos, at, target)
        got, rmsd = got.cpu().numpy(), rmsd.cpu().numpy()
        assert np.isfinite(got).all(), name
        for g in range(pos.shape[0]):
            direct = _direct_rmsd(got[g], target, sel)
            best = CO.kabsch_rmsd(pos[g], target)
            print("alignment %s[%d]: rmsd %.3e (optimum %.3e)" % (name, g, direct, best))
            assert abs(direct - best) < ATOL, (name, g)
            assert abs(rmsd[g] - direct) < 1e-6
            assert np.abs(_pair_distances(got[g]) - _pair_distances(pos[g])).max() < 1e-5
        if name == "generic":
            assert rmsd[0] < 1e-5 and rmsd[1] < 1e-5 and rmsd[2] > 0.1


def test_pruned_conformers_are_superposed_on_the_first_kept_one():
    from agdiff_amd.ensemble import prune_conformers
    at, gen, heavy, perms, want, _ = _case(20, 37, False)
    res = prune_conformers(_item(at, gen), 0.45, align=True)
    raw = prune_conformers(_item(at, gen), 0.45, align=False)
    kept = res["kept"].cpu().numpy()
    assert 1 < kept.size < 37 and torch.equal(res["kept"], raw["kept"])
    assert torch.equal(raw["pos"].cpu(), torch.from_numpy(gen[kept]))
    assert torch.equal(res["pos"][0].cpu(), torch.from_numpy(gen[kept[0]]))
    pos = res["pos"].cpu().numpy()
    for k in range(1, kept.size):
        assert abs(_direct_rmsd(pos[k], pos[0], heavy) - CO.kabsch_rmsd(gen[kept[k]][heavy], gen[kept[0]][heavy])) < ATOL


# ------------------------------------------------------------------------------------------------ 8. driver
def test_run_job_saves_kept_and_cluster_with_the_prune_switch(tmp_path):
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
    res = driver.run_job(m, mols, str(tmp_path / "pruned"), confs, 10 ** 6, kw, "cuda:0", log=quiet, prune_rms=0.5)
    files = glob.glob(str(tmp_path / "pruned" / "samples_[0-9]*.npz"))
    assert len(files) == 1
    for z in (res, np.load(files[0]), np.load(str(tmp_path / "pruned" / "samples_all.npz"))):
        keys = set(z.keys() if isinstance(z, dict) else z.files)
        assert keys == {"%s_%d" % (k, i) for k in ("pos_gen", "name", "kept", "cluster") for i in range(2)}
        for x in mols:
            i = x["index"]
            pos = z["pos_gen_%d" % i]
            assert pos.shape == (6, len(x["atom_type"]), 3) and np.isfinite(pos).all()
            want = prune_conformers(dict(atom_type=x["atom_type"], pos_gen=pos, edge_index=x["edge_index"], edge_type=x["edge_type"]),
                                    0.5, align=False)
            assert z["kept_%d" % i].dtype == np.int32 and z["cluster_%d" % i].dtype == np.int32
            assert np.array_equal(z["kept_%d" % i], want["kept"].cpu().numpy())
            assert np.array_equal(z["cluster_%d" % i], want["leader"].cpu().numpy()) and z["cluster_%d" % i].shape == (6,)
    plain = driver.run_job(m, mols, str(tmp_path / "plain"), confs, 10 ** 6, kw, "cuda:0", log=quiet)
    assert set(plain.keys()) == {"%s_%d" % (k, i) for k in ("pos_gen", "name") for i in range(2)}
    assert set(np.load(glob.glob(str(tmp_path / "plain" / "samples_[0-9]*.npz"))[0]).files) == set(plain.keys())


def test_command_line_prunes_a_finished_job(tmp_path):
    from agdiff_amd import driver, ensemble, synth
    rng = np.random.default_rng(9)
    at, r, c, ty = synth.random_molecule(rng, 15)
    mol = dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=ty, num_refs=2, name="m0")
    driver.save_testset(str(tmp_path / "test.npz"), [mol])
    base = rng.normal(size=(2, 15, 3)) * 1.5
    gen = np.stack([_moved(rng, base[k % 2] + 0.02 * rng.normal(size=(15, 3))) for k in range(7)]).astype(np.float32)
    np.savez(str(tmp_path / "samples_all.npz"), pos_gen_0=gen)
    out = ensemble.main(["--samples", str(tmp_path / "samples_all.npz"), "--testset", str(tmp_path / "test.npz"), "--prune-rms", "0.5",
                         "--align", "--out", str(tmp_path / "pruned.npz")])
    z = np.load(str(tmp_path / "pruned.npz"))
    assert z["kept_0"].tolist() == [0, 1] and z["cluster_0"].tolist() == [0, 1, 0, 1, 0, 1, 0] and z["count_0"].tolist() == [4, 3]
    assert z["pos_0"].shape == (2, 15, 3) and np.array_equal(z["pos_0"][0], gen[0]) and np.array_equal(out["pos_0"], z["pos_0"])


# ------------------------------------------------------------------------------------------------ 9. a conformer that is not a number
def test_a_conformer_with_a_nan_is_kept_alone_and_changes_nobody_elses_leader():
    """prune_conformers does not mask a conformer with a coordinate that is not finite: it reaches the matrix, where by the header's
    rule it is +inf from everything (tests/test_hip_rmsd_kernels.py, section 5), so the walk keeps it as a leader of its own and
    the others come out as they do from the item without it.  Two planted families (intra 0.03-noise, centres 1.5 apart, threshold
    0.5), conformer 3 broken in a heavy atom; with and without a `valid` mask that removes conformer 0, the first leader."""
    from agdiff_amd.ensemble import prune_conformers
    rng = np.random.default_rng(31)
    n, G, bad, thr = 8, 6, 3, 0.5
    at = np.array([6, 6, 7, 6, 8, 1, 1, 6])
    label = np.array([0, 1, 0, 0, 1, 0])
    centres = rng.normal(size=(2, n, 3)) * 1.5
    gen = np.stack([_moved(rng, centres[c] + 0.03 * rng.normal(size=(n, 3))) for c in label]).astype(np.float32)
    gen[bad, 2, 1] = np.nan
    rest = np.delete(np.arange(G), bad)
    masked = np.ones(G, dtype=bool)
    masked[0] = False
    for valid, kept, leader, count in ((None, [0, 1, 3], [0, 1, 0, 3, 1, 0], [3, 2, 1]),
                                       (masked, [1, 2, 3], [-1, 1, 2, 3, 1, 2], [2, 2, 1])):
        res = prune_conformers(_item(at, gen), thr, valid=valid)
        assert res["kept"].cpu().tolist() == kept and res["leader"].cpu().tolist() == leader and res["count"].cpu().tolist() == count
        ref = prune_conformers(_item(at, gen[rest]), thr, valid=None if valid is None else valid[rest])
        own = lambda x: np.where(x < 0, -1, rest[np.maximum(x, 0)])         # the smaller item's indices in this one's
        finite = np.array(kept) != bad
        assert np.array_equal(own(ref["kept"].cpu().numpy()), np.array(kept)[finite])
        assert np.array_equal(own(ref["leader"].cpu().numpy()), np.array(leader)[rest])
        assert np.array_equal(ref["count"].cpu().numpy(), np.array(count)[finite])
        assert torch.equal(res["pos"][torch.from_numpy(finite).cuda()], ref["pos"])     # superposed on the same first conformer
