"""agdiff_flip_double_bonds and what is built on it (agdiff_amd/ezbonds.py) on the GPU: the kernel against the
float64 numpy restatement of its contract (tests/ez_ref.py, anchored in tests/test_ez_ref_cpu.py), the invariants of a rigid 180
degree rotation on the same outputs, the edge cases, the check (double_bond_verdict) and the layers above: fix_double_bonds,
ensemble.prune_conformers, planarity.repair_planarity after it, and driver.run_job.

The inputs (tests/ez_cases.py) are seeded: a planar skeleton, about half of the bonds turned over, 0.1 A of noise, a random frame.
Every test that compares states asserts first, with the restatement, that no tagged dihedral of its input lies within 5 degrees
of 90: the restatement alone decides every state.  No test feeds the kernel an atom index outside [0, n).
"""
import functools

import numpy as np
import pytest
import torch

import ez_cases as EC
import ez_ref as ER
from agdiff_amd import ezbonds as EZ

pytestmark = pytest.mark.gpu

FP32_COORD = 4 * 2.0 ** -24          # x max |coordinate|: the project's bound for a stored fp32 coordinate


def _gpu(pos):
    return torch.from_numpy(np.array(pos, dtype=np.float32)).cuda().contiguous()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _clear_of_ninety(pos, quads):
    """the property of the inputs that lets the restatement alone decide: every tagged dihedral at least 5 degrees from 90"""
    cos = ER.cos_phi(pos, quads)
    assert np.isfinite(cos).all() and (np.abs(cos) > np.cos(np.deg2rad(85.0))).all()
    return cos


@functools.lru_cache(maxsize=None)
def _run(name, G):
    """one launch per shape, shared by the tests below: (pos after, state, flipped) as numpy, read-only"""
    quads, target, ptr, idx = EC.tables(name)
    t = _gpu(EC.conformers(name, G))
    state, flipped = EZ.flip_double_bonds(t, quads, target, ptr, idx, want_flipped=True)
    assert state.dtype == torch.int8 and tuple(state.shape) == (G, quads.shape[0]) and state.is_cuda
    assert flipped.dtype == torch.int32 and tuple(flipped.shape) == (G,)
    out = (t.cpu().numpy(), state.cpu().numpy(), flipped.cpu().numpy())
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name,G", EC.SHAPES)
def test_kernel_matches_the_float64_restatement(name, G):
    """state and flipped exactly; the atoms no flip moved bit for bit; the atoms ONE flip moved within 4 x 2^-24 x max |coordinate| of
    the restatement that rounds to fp32 after every bond (an fp64 result rounded once, on either side of a tie); the atoms that two
    or more nested flips moved within 4 x max |restatement rounding - restatement exact| over these very shapes -- an axis atom
    that the first flip left one fp32 ulp elsewhere tilts the second axis, which has no closed-form bound, and the kernel may sum
    in another order and land on the other side of a rounding once per flip.  That maximum is measured on the CPU
    (ez_cases.nested_deviation, held to its record in tests/test_ezbonds_cpu.py): 4.9e-5 A when this was written, so the bound is
    2.0e-4 A; it comes from the restatement, never from the kernel's output."""
    quads, target, ptr, idx = EC.tables(name)
    pos = EC.conformers(name, G)
    _clear_of_ninety(pos, quads)
    want_pos, want_state, want_flipped, _ = EC.reference(name, G)
    if G == 65:                                  # about half of the conformers have a wrong bond (more with three bonds)
        assert 0.25 < (want_state < 0).any(axis=1).mean() < 0.95
    got, state, flipped = _run(name, G)
    assert np.array_equal(state, want_state) and np.array_equal(flipped, want_flipped)
    assert np.array_equal(flipped, (want_state < 0).sum(axis=1))
    moves = EC.moves(name, want_state)
    err = np.abs(got.astype(np.float64) - want_pos.astype(np.float64))
    assert np.array_equal(_bits(got)[moves == 0], _bits(pos)[moves == 0])
    once, many = moves == 1, moves >= 2
    nested, _ = EC.nested_deviation()
    print("%s G=%d: %d atoms moved once, max err %.3e (bar %.3e); %d moved more than once, max err %.3e (bar %.3e)"
          % (name, G, once.sum(), err[once].max() if once.any() else 0.0, FP32_COORD * np.abs(pos).max(), many.sum(),
             err[many].max() if many.any() else 0.0, 4 * nested))
    if once.any():
        assert err[once].max() <= FP32_COORD * np.abs(pos).max()
    if many.any():
        assert err[many].max() <= 4 * nested
    if G == 65:                                  # the nested rows are those of the triene and of the 600-atom chain
        assert many.any() == (name in ("c14", "big600")) and once.any()


@pytest.mark.parametrize("name,G", EC.SHAPES)
def test_a_flip_is_a_rigid_half_turn_of_one_side(name, G):
    (mol, _, _), (quads, target, ptr, idx) = EC.molecule(name), EC.tables(name)
    pos = EC.conformers(name, G)
    cos_in = _clear_of_ninety(pos, quads)
    got, state, flipped = _run(name, G)
    n, D = pos.shape[1], quads.shape[0]
    rows = [idx[ptr[c]:ptr[c + 1]] for c in range(D)]
    wrong = (state < 0).any(axis=1)                              # (every row of these molecules has atoms: wrong means flipped)
    # conformers without a wrong bond, the side that does not turn, and the bond's own two atoms: bit for bit
    assert np.array_equal(_bits(got)[~wrong], _bits(pos)[~wrong])
    for g in range(G):
        turned = np.zeros(n, dtype=bool)
        for c in np.nonzero(state[g] < 0)[0]:
            turned[np.setdiff1d(rows[c], quads[c, 1:3])] = True
        assert np.array_equal(_bits(got)[g, ~turned], _bits(pos)[g, ~turned])
        if flipped[g] == 1:
            c = int(np.nonzero(state[g] < 0)[0][0])
            assert np.array_equal(_bits(got)[g, quads[c, 1:3]], _bits(pos)[g, quads[c, 1:3]])
    # every bond length and every distance within a rigid fragment (two atoms no row separates) moves by less than 1e-5 A
    member = np.stack([np.isin(np.arange(n), r) for r in rows])
    same = (member[:, :, None] == member[:, None, :]).all(axis=0)
    bonds = mol[1][:, mol[2] < 22]
    some = range(G) if n <= 200 else range(min(G, 3))
    for g in some:
        a, b = pos[g].astype(np.float64), got[g].astype(np.float64)
        dist = lambda p: np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
        assert np.abs(dist(a) - dist(b))[same].max() < 1e-5
    length = lambda p: np.sqrt(((p[:, bonds[0]].astype(np.float64) - p[:, bonds[1]].astype(np.float64)) ** 2).sum(-1))
    assert np.abs(length(got) - length(pos)).max() < 1e-5
    # cos phi of a flipped bond is negated, that of every other tagged bond is unchanged
    cos_out = ER.cos_phi(got, quads)
    assert np.abs(np.where(state < 0, -cos_in, cos_in) - cos_out).max() < 1e-5
    # the check sees no wrong flippable bond any more, and a second call flips nothing and writes nothing
    again = _gpu(got)
    after = EZ.double_bond_verdict(again, quads, target).cpu().numpy()
    assert (after == 1).all()
    state2, flipped2 = EZ.flip_double_bonds(again, quads, target, ptr, idx, want_flipped=True)
    assert np.array_equal(state2.cpu().numpy(), after) and not flipped2.any().item()
    assert np.array_equal(_bits(again.cpu().numpy()), _bits(got))
    # tetrahedral centres keep their hand: a rotation is no reflection
    from agdiff_amd.stereo import signed_volumes, tetrahedral_centres
    centre, four = tetrahedral_centres(*mol)
    assert (centre.size > 0) == (name == "centre")
    if centre.size:
        vol_in, vol_out = signed_volumes(pos, four), signed_volumes(got, four)
        assert (np.abs(vol_in) > 0.1).all() and (np.sign(vol_in) == np.sign(vol_out)).all() and np.abs(vol_in - vol_out).max() < 1e-4
        assert np.isin(four, rows[0]).all() and (G < 65 or (state < 0).any())          # the centre's neighbours all turn


@pytest.mark.parametrize("name,G", EC.SHAPES)
def test_double_bond_verdict_is_the_restatements_state_of_the_input(name, G):
    quads, target, _, _ = EC.tables(name)
    pos = EC.conformers(name, G)
    _clear_of_ninety(pos, quads)
    state = EZ.double_bond_verdict(_gpu(pos), quads, target)
    assert state.dtype == torch.int8 and state.is_cuda and tuple(state.shape) == (G, quads.shape[0])
    assert np.array_equal(state.cpu().numpy(), ER.states(pos, quads, target))
    assert np.array_equal(state.cpu().numpy(), EC.reference(name, G)[1])         # the bonds are bridges: the walk's state is the input's
    assert np.array_equal(EZ.double_bond_verdict(_gpu(pos), quads, -target).cpu().numpy(), -ER.states(pos, quads, target))


# ---------------------------------------------------------------------------------------------------------------- edge cases
def test_no_bonds_is_an_empty_state_and_leaves_pos_alone():
    pos = EC.conformers("c6", 3)
    t = _gpu(pos)
    state, flipped = EZ.flip_double_bonds(t, np.zeros((0, 4), np.int32), np.zeros(0, np.int8), np.zeros(1, np.int32), np.zeros(0, np.int32),
                                          want_flipped=True)
    assert tuple(state.shape) == (3, 0) and state.dtype == torch.int8 and flipped.tolist() == [0, 0, 0]
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(pos))
    assert tuple(EZ.double_bond_verdict(t, np.zeros((0, 4), np.int32), np.zeros(0, np.int8)).shape) == (3, 0)
    empty = torch.empty((0, 6, 3), dtype=torch.float32, device="cuda")
    quads, target, ptr, idx = EC.tables("c6")
    assert tuple(EZ.flip_double_bonds(empty, quads, target, ptr, idx).shape) == (0, 1)


def test_untagged_rows_are_never_flipped():
    quads, target, ptr, idx = EC.tables("c14")
    pos = EC.conformers("c14", 65)
    _clear_of_ninety(pos, quads)
    some = target * np.array([1, 0, 1], dtype=np.int8)
    want_pos, want_state, want_flipped = ER.flip(pos, quads, some, ptr, idx)
    assert not want_state[:, 1].any() and (EC.reference("c14", 65)[1][:, 1] < 0).any()
    t = _gpu(pos)
    state, flipped = EZ.flip_double_bonds(t, quads, some, ptr, idx, want_flipped=True)
    assert np.array_equal(state.cpu().numpy(), want_state) and np.array_equal(flipped.cpu().numpy(), want_flipped)
    got = t.cpu().numpy()
    assert np.abs(got.astype(np.float64) - want_pos).max() <= FP32_COORD * np.abs(pos).max()     # (rows 0 and 2 are disjoint: one flip each)
    cos_in, cos_out = ER.cos_phi(pos, quads), ER.cos_phi(got, quads)
    assert np.abs(cos_in[:, 1] - cos_out[:, 1]).max() < 1e-5
    none = np.zeros(3, dtype=np.int8)
    t = _gpu(pos)
    assert not EZ.flip_double_bonds(t, quads, none, ptr, idx).any().item() and np.array_equal(_bits(t.cpu().numpy()), _bits(pos))


def _cyclooctene(G, seed=1):
    import planarity_ref as PR
    k = np.arange(8)
    ring = np.stack([1.75 * np.cos(2 * np.pi * k / 8), 1.75 * np.sin(2 * np.pi * k / 8), np.zeros(8)], axis=1)
    flat = np.concatenate([ring, 1.6 * ring[:2]])
    mol = PR.graph([6] * 8 + [1, 1], [(i, (i + 1) % 8, 2 if i == 0 else 1) for i in range(8)] + [(0, 8, 1), (1, 9, 1)])
    rng = np.random.default_rng(seed)
    return mol, np.stack([(flat + rng.uniform(-0.1, 0.1, size=flat.shape)) @ EC.random_rotation(rng).T for _ in range(G)]).astype(np.float32)


def test_a_ring_bond_is_judged_and_not_flipped():
    mol, pos = _cyclooctene(3)
    quads, in_ring = EZ.stereo_double_bonds(*mol)
    assert quads.tolist() == [[7, 0, 1, 2]] and in_ring.tolist() == [True]
    _clear_of_ninety(pos, quads)
    ptr, idx = EZ.flip_sides(10, mol[1], mol[2], quads)
    assert ptr.tolist() == [0, 0]
    t = _gpu(pos)
    state, flipped = EZ.flip_double_bonds(t, quads, [1], ptr, idx, want_flipped=True)             # tagged trans; the ring holds it cis
    assert state.cpu().numpy().tolist() == [[-1]] * 3 == ER.states(pos, quads, [1]).tolist() and flipped.tolist() == [0, 0, 0]
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(pos))
    item = dict(atom_type=mol[0], edge_index=mol[1], edge_type=mol[2], ez_quads=quads, ez=[1])
    assert EZ.fix_double_bonds(item, t).cpu().numpy().tolist() == [[-1]] * 3 and np.array_equal(_bits(t.cpu().numpy()), _bits(pos))


def test_a_quad_that_is_not_finite_or_collinear_is_undecided_and_its_conformer_untouched():
    quads, target, ptr, idx = EC.tables("c6")                 # row: atoms 2, 3 and hydrogen 5
    pos = np.array(EC.conformers("c6", 65)[:6])
    want = ER.states(pos, quads, target)[:, 0]
    assert (want[:5] < 0).any() and (want[:5] > 0).any()
    pos[:4] = pos[np.nonzero(want < 0)[0][0]]                 # four copies of a wrong conformer, then two as they are
    pos[0, 3, 1] = np.nan                                     # in the quad: undecided
    pos[1, 0, 2] = np.inf
    pos[2, :3] = [[-1.0, -1.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 0.0]]     # a - i - j collinear, exactly
    pos[3, 5, 0] = np.nan                                     # on the turning side, in no quad: the bond is flipped, this atom stays
    want_pos, want_state, want_flipped = ER.flip(pos, quads, target, ptr, idx)
    assert want_state[:4, 0].tolist() == [0, 0, 0, -1] and want_flipped[:4].tolist() == [0, 0, 0, 1]
    t = _gpu(pos)
    state, flipped = EZ.flip_double_bonds(t, quads, target, ptr, idx, want_flipped=True)
    got = t.cpu().numpy()
    assert np.array_equal(state.cpu().numpy(), want_state) and np.array_equal(flipped.cpu().numpy(), want_flipped)
    assert np.array_equal(_bits(got)[:3], _bits(pos)[:3])     # by bit pattern: NaN != NaN
    assert np.array_equal(_bits(got)[3, 5], _bits(pos)[3, 5]) and np.array_equal(_bits(got)[3, :3], _bits(pos)[3, :3])
    ok = np.isfinite(pos)
    assert np.abs(got.astype(np.float64)[ok] - want_pos.astype(np.float64)[ok]).max() <= FP32_COORD * np.abs(pos[ok]).max()
    assert np.abs(got[3, 3] - pos[3, 3]).max() > 0.5
    assert EZ.double_bond_verdict(_gpu(pos), quads, target).cpu().numpy()[:4, 0].tolist() == [0, 0, 0, -1]


def test_the_wrapper_refuses_bad_tables_before_any_launch():
    quads, target, ptr, idx = EC.tables("c14")
    pos = EC.conformers("c14", 3)
    t = _gpu(pos)
    bad_quads = quads.copy()
    bad_quads[1, 3] = 14
    neg_quads = quads.copy()
    neg_quads[0, 0] = -1
    late = ptr.copy()
    late[0] = 1
    back = ptr.copy()
    back[1], back[2] = back[2], back[1]
    far = idx.copy()
    far[-1] = 14
    for args, message in (((bad_quads, target, ptr, idx), r"outside \[0, 14\)"), ((neg_quads, target, ptr, idx), r"outside \[0, 14\)"),
                          ((quads, target[:2], ptr, idx), "3 quads but 2 targets"), ((quads, target, ptr[:3], idx), "side_ptr"),
                          ((quads, target, late, idx), "side_ptr"), ((quads, target, back, idx), "side_ptr"),
                          ((quads, target, ptr, idx[:-1]), "side_ptr"), ((quads, target, ptr, far), r"side_idx names atoms outside \[0, 14\)"),
                          ((quads, target, ptr, -idx - 1), "side_idx")):
        with pytest.raises(ValueError, match=message):
            EZ.flip_double_bonds(t, *args)
    for args in ((bad_quads, target), (quads, target[:2])):
        with pytest.raises(ValueError):
            EZ.double_bond_verdict(t, *args)
    for wrong in (t.cpu(), t.double(), t.reshape(-1, 3), t[:, :, [0, 2, 1]].transpose(1, 2)):
        with pytest.raises(ValueError, match="contiguous float32"):
            EZ.flip_double_bonds(wrong, quads, target, ptr, idx)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(pos))


# ------------------------------------------------------------------------------------------------------- through the layers
@pytest.mark.parametrize("name", ["c14", "centre", "side65"])
def test_fix_double_bonds_is_the_raw_call_with_the_items_tables(name):
    (mol, _, frozen), (quads, target, _, _) = EC.molecule(name), EC.tables(name)
    pos = EC.conformers(name, 3)
    got, state, _ = _run(name, 3)
    t = _gpu(pos)
    item = dict(atom_type=mol[0], edge_index=mol[1], edge_type=mol[2], ez_quads=quads, ez=target)
    res = EZ.fix_double_bonds(item, t, frozen=frozen)
    assert np.array_equal(res.cpu().numpy(), state) and np.array_equal(_bits(t.cpu().numpy()), _bits(got))
    with pytest.raises(ValueError, match="atoms per conformer"):
        EZ.fix_double_bonds(item, _gpu(pos[:, :-1]))
    with pytest.raises(ValueError, match="ez_quads"):
        EZ.fix_double_bonds({k: v for k, v in item.items() if k != "ez_quads"}, t)


def _isomer_mix(G=12, noise=0.02, seed=2):
    """c10 (two double bonds with disjoint sides): G conformers, the four combinations of right and wrong in turn, little noise"""
    (mol, skeleton, _), (quads, target, ptr, idx) = EC.molecule("c10"), EC.tables("c10")
    rng = np.random.default_rng(seed)
    pos = np.empty((G,) + skeleton.shape, dtype=np.float32)
    for g in range(G):
        p = skeleton.copy()
        for c in range(2):
            if (g >> c) & 1:
                ER.rotate_side(p, int(quads[c, 1]), int(quads[c, 2]), idx[ptr[c]:ptr[c + 1]])
        pos[g] = (p + noise * rng.normal(size=p.shape)) @ EC.random_rotation(rng).T
    return dict(atom_type=mol[0], edge_index=mol[1], edge_type=mol[2], ez_quads=quads, ez=target, pos_gen=pos)


def test_prune_with_the_fix_keeps_what_the_prune_of_the_hand_corrected_set_keeps():
    from agdiff_amd.ensemble import prune_conformers
    item = _isomer_mix()
    quads, target, ptr, idx = EC.tables("c10")
    _clear_of_ninety(item["pos_gen"], quads)
    by_hand, want_state, _ = ER.flip(item["pos_gen"], quads, target, ptr, idx)
    assert (want_state < 0).any(axis=1).sum() == 9
    before = item["pos_gen"].copy()
    raw = prune_conformers(item, 0.3, align=False)
    fixed = prune_conformers(item, 0.3, align=False, fix_double_bonds=True)
    hand = prune_conformers(dict(item, pos_gen=by_hand), 0.3, align=False)
    assert "ez_state" not in raw and np.array_equal(fixed["ez_state"].cpu().numpy(), want_state) and fixed["ez_state"].dtype == torch.int8
    # as sampled: one cluster per isomer -- the tagged one, one bond wrong (either: the chain read backwards maps the two onto each
    # other, and the RMSD honours the molecule's symmetry), both wrong -- so two of the three kept conformers are wasted
    assert raw["kept"].tolist() == [0, 1, 3]
    assert fixed["kept"].tolist() == hand["kept"].tolist() == [0] and len(fixed["kept"]) <= len(hand["kept"])
    assert fixed["leader"].tolist() == hand["leader"].tolist() == [0] * 12
    assert np.array_equal(item["pos_gen"], before)                 # the caller's conformers are never written
    tfd = prune_conformers(item, 0.3, align=False, fix_double_bonds=True, metric="tfd")
    assert np.array_equal(tfd["ez_state"].cpu().numpy(), want_state)


def test_the_ensemble_and_evaluation_command_lines(tmp_path, capsys):
    from agdiff_amd import driver, ensemble, evaluation
    item = _isomer_mix()
    quads, target, ptr, idx = EC.tables("c10")
    mol = dict(atom_type=item["atom_type"], edge_index=item["edge_index"], edge_type=item["edge_type"], num_refs=6, name="diene")
    driver.save_testset(str(tmp_path / "plain.npz"), [mol])
    driver.save_testset(str(tmp_path / "tagged.npz"), [dict(mol, ez_quads=quads, ez=target)])
    np.savez(str(tmp_path / "samples.npz"), pos_gen_0=item["pos_gen"], name_0=np.str_("diene"))
    out = ensemble.main(["--samples", str(tmp_path / "samples.npz"), "--testset", str(tmp_path / "tagged.npz"), "--prune-rms", "0.3",
                         "--fix-double-bonds", "--out", str(tmp_path / "pruned.npz")])
    z = np.load(str(tmp_path / "pruned.npz"))
    assert z["ez_state_0"].dtype == np.int8 and np.array_equal(z["ez_state_0"], ER.states(item["pos_gen"], quads, target))
    assert z["kept_0"].tolist() == [0] and np.array_equal(out["ez_state_0"], z["ez_state_0"])
    plain = ensemble.main(["--samples", str(tmp_path / "samples.npz"), "--testset", str(tmp_path / "tagged.npz"), "--prune-rms", "0.3",
                           "--out", str(tmp_path / "plain_pruned.npz")])
    assert "ez_state_0" not in plain and plain["kept_0"].tolist() == [0, 1, 3]
    with pytest.raises(ValueError, match="ez_quads_0"):
        ensemble.main(["--samples", str(tmp_path / "samples.npz"), "--testset", str(tmp_path / "plain.npz"), "--prune-rms", "0.3",
                       "--fix-double-bonds", "--out", str(tmp_path / "never.npz")])
    capsys.readouterr()
    shares = evaluation.ez_report(str(tmp_path / "samples.npz"), str(tmp_path / "tagged.npz"))
    assert shares == {0: 0.75} and "diene: 2 tagged double bonds, 0.7500 of 12 generated conformers" in capsys.readouterr().out
    assert evaluation.ez_report(str(tmp_path / "samples.npz"), str(tmp_path / "plain.npz")) == {}
    # --ez-report adds its lines below the COV / MAT table and changes nothing in it; the tags come from --testset or from the refs
    by_hand = ER.flip(item["pos_gen"], quads, target, ptr, idx)[0]
    refs = dict(pos_ref_0=by_hand[:3], atom_type_0=item["atom_type"], edge_index_0=item["edge_index"], edge_type_0=item["edge_type"])
    np.savez(str(tmp_path / "refs.npz"), **refs)
    np.savez(str(tmp_path / "refs_tagged.npz"), ez_quads_0=quads, ez_0=target, name_0=np.str_("diene"), **refs)
    base = ["--samples", str(tmp_path / "samples.npz")]
    capsys.readouterr()
    evaluation.main(base + ["--refs", str(tmp_path / "refs.npz")])
    table = capsys.readouterr().out
    for extra in (["--refs", str(tmp_path / "refs.npz"), "--ez-report", "--testset", str(tmp_path / "tagged.npz")],
                  ["--refs", str(tmp_path / "refs_tagged.npz"), "--ez-report"]):
        res = evaluation.main(base + extra)
        out = capsys.readouterr().out
        assert table and out.startswith(table) and "0.7500 of 12 generated conformers" in out[len(table):] and res.ez_wrong == {0: 0.75}


def test_the_fix_before_the_flattening_ends_in_the_tagged_isomer_and_without_it_in_the_other():
    """the gap planarity.py documents, closed: (E)-2-butene with C2's side turned to a dihedral of -60 degrees -- 120 degrees from
    where the tag says, on the wrong side of 90 -- flattens to cis as it is and to trans after the fix"""
    from agdiff_amd.planarity import repair_planarity
    mol, pos = EC.butene(120.0)
    quads, in_ring = EZ.stereo_double_bonds(*mol)
    assert quads.tolist() == [[0, 1, 2, 3]] and abs(abs(EC.signed_dihedral(pos, quads[0])) - 60.0) < 1e-6
    item = dict(atom_type=mol[0], edge_index=mol[1], edge_type=mol[2], ez_quads=quads, ez=[1])
    t = _gpu(pos[None])
    plain = repair_planarity(dict(item, pos_gen=t.clone()))
    assert plain["status"].tolist() == [1] and abs(EC.signed_dihedral(plain["pos"][0].cpu().numpy().astype(np.float64), quads[0])) < 45.0
    assert EZ.double_bond_verdict(plain["pos"], quads, [1]).tolist() == [[-1]]
    assert EZ.fix_double_bonds(item, t).tolist() == [[-1]]
    assert abs(abs(EC.signed_dihedral(t[0].cpu().numpy().astype(np.float64), quads[0])) - 120.0) < 1e-3
    fixed = repair_planarity(dict(item, pos_gen=t))
    assert fixed["status"].tolist() == [1] and abs(EC.signed_dihedral(fixed["pos"][0].cpu().numpy().astype(np.float64), quads[0])) > 135.0
    assert EZ.double_bond_verdict(fixed["pos"], quads, [1]).tolist() == [[1]]


def _gpu_model(cfg, head_scale=1e-3, precision="f16x3"):
    """the synthetic checkpoint of tests/test_hip_stereo.py's driver job"""
    from agdiff_amd import get_model
    from oracle import agdiff_oracle as O
    sd = O.synth_state_dict_for(cfg, head_scale=head_scale)
    m = get_model(cfg)
    m.precision = precision
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    return m.to("cuda:0").eval()


def _two_tagged_molecules():
    """that job's shape -- two molecules, 3 and 4 references -- with molecules that have double bonds to tag: c6 and the triene c14,
    the second with a core (carbons 0 .. 3 and their hydrogens) for the hold_core runs"""
    mols = []
    for i, name in enumerate(("c6", "c14")):
        (mol, skeleton, _), (quads, target, _, _) = EC.molecule(name), EC.tables(name)
        mols.append(dict(atom_type=mol[0], edge_index=mol[1], edge_type=mol[2], num_refs=3 + i, name="mol%d" % i, index=i,
                         ez_quads=quads, ez=target))
    mols[1]["core_pos"] = (EC.molecule("c14")[1] + 2.0).astype(np.float32)
    mols[1]["core_mask"] = np.isin(np.arange(14), [0, 1, 2, 3, 8, 9, 10])
    return mols


def _job(tmp_path):
    from agdiff_amd import driver, qm9_model_config
    m = _gpu_model(qm9_model_config(num_diffusion_timesteps=10))
    confs = driver.num_confs("2x")
    kw = dict(n_steps=10, step_lr=1e-6, w_global=1.0, global_start_sigma=0.5, clip=1000.0)
    logs = []
    run = lambda name, mols, **extra: driver.run_job(m, [dict(x) for x in mols], str(tmp_path / name), confs, 100000, kw, "cuda:0",
                                                     log=logs.append, noise="counter", seed=5, **extra)
    return run, logs, confs


def test_driver_writes_ez_state_and_leaves_the_plain_job_alone(tmp_path):
    run, logs, confs = _job(tmp_path)
    mols = [{k: v for k, v in x.items() if not k.startswith("core_")} for x in _two_tagged_molecules()]
    off, off2, on = run("off", mols), run("off2", mols), run("on", mols, fix_double_bonds=True)
    assert sorted(off) == sorted(off2) == ["name_0", "name_1", "pos_gen_0", "pos_gen_1"]
    assert sorted(on) == ["ez_state_0", "ez_state_1", "name_0", "name_1", "pos_gen_0", "pos_gen_1"]
    n_flipped = n_open = 0
    for x in mols:
        i, g, n = x["index"], confs(x["num_refs"]), len(x["atom_type"])
        for k in ("pos_gen_%d" % i, "name_%d" % i):
            assert off[k].dtype == off2[k].dtype and off[k].tobytes() == off2[k].tobytes()
        state, raw, fixed = on["ez_state_%d" % i], off["pos_gen_%d" % i], on["pos_gen_%d" % i]
        D = len(x["ez"])
        assert state.dtype == np.int8 and state.shape == (g, D) and fixed.shape == raw.shape == (g, n, 3) and fixed.dtype == np.float32
        # what was written is the raw conformers' state (the bonds are bridges), the conformers without a wrong bond are the sampler's bytes
        assert np.array_equal(state, EZ.double_bond_verdict(_gpu(raw), x["ez_quads"], x["ez"]).cpu().numpy())
        quiet = ~(state < 0).any(axis=1)
        assert fixed[quiet].tobytes() == raw[quiet].tobytes()
        after = EZ.double_bond_verdict(_gpu(fixed), x["ez_quads"], x["ez"]).cpu().numpy()
        assert (after >= 0).all() and (after[state != 0] == 1).all()              # every bond of these two molecules can be flipped
        n_flipped += int((state < 0).any(axis=1).sum())
        n_open += int((state == 0).sum())
    assert n_flipped > 0                                         # (14 conformers, 30 bonds, drawn with either parity)
    mine = [l for l in logs if "wrong E/Z parity" in l]
    assert len(mine) == 1 and "%d of %d conformers had" % (n_flipped, sum(confs(x["num_refs"]) for x in mols)) in mine[0]
    assert "0 bonds stay wrong" in mine[0] and "%d tagged bonds are undecided" % n_open in mine[0]
    import os
    for drop in ("ez", "ez_quads"):
        with pytest.raises(ValueError, match="ez_quads"):
            run("untagged_" + drop, [{k: v for k, v in x.items() if k != drop} for x in mols], fix_double_bonds=True)
        assert not os.path.exists(str(tmp_path / ("untagged_" + drop)))          # before sampling: not even the directory
    broken = [dict(x) for x in mols]
    broken[1]["ez_quads"] = np.array(broken[1]["ez_quads"])[:, ::-1][:, [0, 2, 1, 3]]
    with pytest.raises(ValueError, match="mol1"):
        run("broken", broken, fix_double_bonds=True)


def test_driver_with_a_held_core_flips_the_other_side_and_never_moves_the_core(tmp_path):
    run, logs, confs = _job(tmp_path)
    mols = _two_tagged_molecules()
    held, both = run("held", mols, hold_core=True), run("both", mols, hold_core=True, fix_double_bonds=True)
    assert sorted(set(both) - set(held)) == ["ez_state_0", "ez_state_1"]
    x = mols[1]
    core = x["core_mask"]
    raw, fixed, state = held["pos_gen_1"], both["pos_gen_1"], both["ez_state_1"]
    assert fixed[:, core].tobytes() == raw[:, core].tobytes()
    assert np.array_equal(held["core_rmsd_1"], both["core_rmsd_1"])
    # bond 0 has core atoms on both sides: judged, left as sampled; bonds 1 and 2 turn their free sides
    ptr, idx = EZ.flip_sides(14, x["edge_index"], x["edge_type"], x["ez_quads"], frozen=core)
    assert np.diff(ptr).tolist() == [0, 7, 3]
    assert np.array_equal(state, EZ.double_bond_verdict(_gpu(raw), x["ez_quads"], x["ez"]).cpu().numpy())
    after = EZ.double_bond_verdict(_gpu(fixed), x["ez_quads"], x["ez"]).cpu().numpy()
    assert (state[:, 1:] < 0).any() and fixed.tobytes() != raw.tobytes()
    assert np.array_equal(after[:, 0], state[:, 0]) and (after[:, 1:] >= 0).all() and (after[:, 1:][state[:, 1:] != 0] == 1).all()
    mine = [l for l in logs if "wrong E/Z parity" in l]
    assert len(mine) == 1 and "%d bonds stay wrong" % int((after < 0).sum()) in mine[0]
    assert held["pos_gen_0"].shape == both["pos_gen_0"].shape
