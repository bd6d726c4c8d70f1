"""No GPU: the host side of the planarity check (agdiff_amd/planarity.py) -- which groups of atoms the bond types name, on molecules
written out by hand --, the float64 restatement of the definition (tests/planarity_ref.py) on cases that are exact, the C ABI of the
entry point as the header declares it, its host-side argument checks (every one returns before any launch), and the wrappers' and
command lines' own refusals."""
import ctypes

import numpy as np
import pytest

import planarity_ref as PR
from agdiff_amd import _lib

VP, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
H, C, N, O, S = 1, 6, 7, 8, 16


def _item(mol, **kw):
    at, ei, et = mol
    return dict(atom_type=at, edge_index=ei, edge_type=et, **kw)


def _groups(atoms, bonds, order=3):
    from agdiff_amd.planarity import planar_groups
    ptr, idx, kind = planar_groups(_item(PR.graph(atoms, bonds, order)))
    assert ptr.dtype == idx.dtype == np.int32 and kind.dtype == np.int8
    assert ptr.shape == (kind.shape[0] + 1,) and ptr[0] == 0 and ptr[-1] == idx.shape[0]
    return PR.groups_of(ptr, idx, kind)


BENZENE = ([C] * 6 + [H] * 6, [(k, (k + 1) % 6, 12) for k in range(6)] + [(k, 6 + k, 1) for k in range(6)])


# ------------------------------------------------------------------------------------------------ 1. groups
def test_aromatic_rings():
    assert _groups(*BENZENE) == [(0, [0, 1, 2, 3, 4, 5])]                     # the hydrogens are in no group
    fused = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (4, 6), (6, 7), (7, 8), (8, 9), (9, 5)]
    assert _groups([C] * 10, [(a, b, 12) for a, b in fused]) == [(0, [0, 1, 2, 3, 4, 5]), (0, [4, 5, 6, 7, 8, 9])]      # naphthalene
    indole = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (4, 6), (6, 7), (7, 8), (8, 5)]
    assert _groups([C] * 8 + [N], [(a, b, 12) for a, b in indole]) == [(0, [0, 1, 2, 3, 4, 5]), (0, [4, 5, 6, 7, 8])]
    # a 7-membered aromatic cycle and a 4-membered one are not groups; cyclohexane has no aromatic bond
    assert _groups([C] * 7, [(k, (k + 1) % 7, 12) for k in range(7)]) == []
    assert _groups([C] * 4, [(k, (k + 1) % 4, 12) for k in range(4)]) == []
    assert _groups([C] * 6 + [H] * 12, [(k, (k + 1) % 6, 1) for k in range(6)] + [(k // 2, 6 + k, 1) for k in range(12)]) == []


def test_double_bonds():
    ethene = ([C, C] + [H] * 4, [(0, 1, 2), (0, 2, 1), (0, 3, 1), (1, 4, 1), (1, 5, 1)])
    assert _groups(*ethene) == [(1, [0, 1, 2, 3, 4, 5])]
    methyls = [(2, 4, 1), (2, 5, 1), (2, 6, 1), (3, 7, 1), (3, 8, 1), (3, 9, 1)]
    assert _groups([C, O, C, C] + [H] * 6, [(0, 1, 2), (0, 2, 1), (0, 3, 1)] + methyls) == [(1, [0, 1, 2, 3])]           # acetone
    assert _groups([S, O, O, C, C] + [H] * 6, [(0, 1, 2), (0, 2, 2), (0, 3, 1), (0, 4, 1)]
                   + [(3 + k // 3, 5 + k, 1) for k in range(6)]) == []                                                    # dimethyl sulfone
    assert _groups([S, O, C, C] + [H] * 6, [(0, 1, 2), (0, 2, 1), (0, 3, 1)] + methyls) == []                            # dimethyl sulfoxide
    # nitromethane, charge-separated (one N=O and one N-O): one group; drawn with two N=O: one group per double bond, the same atoms
    ch3 = [(0, 4, 1), (0, 5, 1), (0, 6, 1)]
    assert _groups([C, N, O, O] + [H] * 3, [(0, 1, 1), (1, 2, 2), (1, 3, 1)] + ch3) == [(1, [0, 1, 2, 3])]
    assert _groups([C, N, O, O] + [H] * 3, [(0, 1, 1), (1, 2, 2), (1, 3, 2)] + ch3) == [(1, [0, 1, 2, 3])] * 2
    allene = ([C] * 3 + [H] * 4, [(0, 1, 2), (1, 2, 2), (0, 3, 1), (0, 4, 1), (2, 5, 1), (2, 6, 1)])
    assert _groups(*allene) == [(1, [0, 1, 2, 3, 4]), (1, [0, 1, 2, 5, 6])]
    assert _groups([C, C, H, H], [(0, 1, 3), (0, 2, 1), (1, 3, 1)]) == []                                                 # a triple bond
    assert _groups([C, O], [(0, 1, 2)], order=1) == []                                                                   # C=O alone: 2 atoms
    assert _groups([C, O, H], [(0, 1, 2), (0, 2, 1)]) == []                                                              # 3 atoms
    # an imine with a terminal S on the far side of another double bond: thioketone C=S is fine (S has one neighbour)
    assert _groups([C, S, C, C], [(0, 1, 2), (0, 2, 1), (0, 3, 1)]) == [(1, [0, 1, 2, 3])]
    # a phosphate-like centre with four neighbours is out whatever the element
    assert _groups([C, O, C, C, C], [(0, 1, 2), (0, 2, 1), (0, 3, 1), (0, 4, 1)]) == []


def test_a_kekulised_ring_is_seen_through_its_double_bonds_only():
    bonds = [(k, (k + 1) % 6, 2 if k % 2 == 0 else 1) for k in range(6)] + [(k, 6 + k, 1) for k in range(6)]
    assert _groups([C] * 6 + [H] * 6, bonds) == [(1, [0, 1, 2, 5, 6, 7]), (1, [0, 3, 4, 5, 10, 11]), (1, [1, 2, 3, 4, 8, 9])]


def test_the_group_order_does_not_depend_on_how_the_bonds_are_listed():
    from agdiff_amd.planarity import MAX_ATOMS, planar_groups
    mol, _ = PR.styrene()
    want = [(0, [0, 1, 2, 3, 4, 5]), (1, [0, 6, 7, 13, 14, 15])]
    ptr, idx, kind = planar_groups(_item(mol))
    assert PR.groups_of(ptr, idx, kind) == want and np.diff(ptr).max() <= MAX_ATOMS
    rng = np.random.default_rng(1)
    for _ in range(3):
        order = rng.permutation(mol[2].shape[0])
        again = planar_groups(dict(atom_type=mol[0], bond_index=mol[1][:, order][::-1], bond_type=mol[2][order]))
        assert all(np.array_equal(a, b) for a, b in zip(again, (ptr, idx, kind)))
    # the 2- and 3-hop entries (types 23, 24) are ignored: the raw bonds give the same groups
    raw = PR.graph(mol[0], [(int(a), int(b), int(t)) for (a, b), t in zip(mol[1].T, mol[2]) if a < b and t < 22], order=1)
    assert all(np.array_equal(a, b) for a, b in zip(planar_groups(_item(raw)), (ptr, idx, kind)))
    # one-directional bond lists too, and an item given as an object
    half = mol[1][0] < mol[1][1]
    obj = type("Item", (), dict(atom_type=mol[0], edge_index=mol[1][:, half], edge_type=mol[2][half]))()
    assert all(np.array_equal(a, b) for a, b in zip(planar_groups(obj), (ptr, idx, kind)))


def test_bad_items_are_refused():
    from agdiff_amd.planarity import planar_groups
    with pytest.raises(ValueError, match="outside"):
        planar_groups(dict(atom_type=np.array([C, C]), bond_index=np.array([[0, 2], [2, 0]]), bond_type=np.array([2, 2])))
    with pytest.raises(ValueError, match="bonds"):
        planar_groups(dict(atom_type=np.array([C, C])))
    ptr, idx, kind = planar_groups(dict(atom_type=np.array([C, C]), bond_index=np.zeros((2, 0), np.int64), bond_type=np.zeros(0, np.int64)))
    assert ptr.tolist() == [0] and idx.shape == (0,) and kind.shape == (0,) and idx.dtype == np.int32


# ------------------------------------------------------------------------------------------------ 2. the reference
def test_reference_on_exact_cases():
    pos = np.concatenate([PR.square(0.5), PR.hexagon(), PR.square(0.25, (2, -4, 1))])[None]
    ptr, idx = [0, 4, 10, 14], np.arange(14)
    ref = PR.planar(pos, ptr, idx, 0.3)
    assert ref["dev"].tolist() == [[0.5, 0.0, 0.25]] and ref["dev"].dtype == np.float32
    assert ref["worst"].tolist() == [0.5] and ref["worst_group"].tolist() == [0] and ref["n_bent"].tolist() == [1]
    assert np.allclose(ref["gap"], [[0.75, 2.0, 0.9375]]) and not PR.left_out(ref).any()
    PR.assert_margins(ref, pos, 0.3)
    with pytest.raises(AssertionError):
        PR.assert_margins(ref, pos, 0.25)                                      # a dev on the threshold
    with pytest.raises(AssertionError):
        PR.assert_margins(PR.planar(pos, [0, 4, 8], [0, 1, 2, 3, 0, 1, 2, 3], 0.3), pos, 0.3)       # a tie
    PR.assert_margins(PR.planar(pos, [0, 4, 8], [0, 1, 2, 3, 0, 1, 2, 3], 0.3), pos, 0.3, ties=True)
    with pytest.raises(AssertionError):
        PR.assert_margins(ref, pos + 16, 0.3)
    # ties take the lowest index; P = 0; a group that is too small, too large or names an atom outside is NaN and takes no part
    assert PR.planar(pos, [0, 4, 8, 12], [10, 11, 12, 13, 0, 1, 2, 3, 0, 1, 2, 3], 0.3)["worst_group"].tolist() == [1]
    none = PR.planar(pos, [0], [], 0.3)
    assert none["dev"].shape == (1, 0) and (none["worst"].tolist(), none["worst_group"].tolist(), none["n_bent"].tolist()) == ([0.0], [-1], [0])
    odd = PR.planar(pos, [0, 2, 11, 15, 19], [0, 1] + list(range(9)) + [0, 1, 2, 14] + [10, 11, 12, 13], 0.2)
    assert np.isnan(odd["dev"][0, :3]).all() and odd["dev"][0, 3] == 0.25
    assert (odd["worst"].tolist(), odd["worst_group"].tolist(), odd["n_bent"].tolist()) == ([0.25], [3], [1])
    dead = PR.planar(pos, [0, 2], [0, 1], 0.2)
    assert (dead["worst"].tolist(), dead["worst_group"].tolist(), dead["n_bent"].tolist()) == ([0.0], [-1], [0])
    # a coordinate that is not finite: +inf, counted, and it wins
    for bad in (np.nan, np.inf):
        broken = pos.copy()
        broken[0, 12, 1] = bad
        r = PR.planar(broken, ptr, idx, 0.3)
        assert np.isposinf(r["dev"][0, 2]) and r["dev"][0, :2].tolist() == [0.5, 0.0]
        assert np.isposinf(r["worst"][0]) and r["worst_group"].tolist() == [2] and r["n_bent"].tolist() == [2]


def test_the_styrene_conformers_through_the_reference_alone():
    """the molecule of the GPU test: the lifted ring carbon bends the ring group only, the twisted CH2 the double-bond group only"""
    from agdiff_amd.planarity import planar_groups
    mol, pos = PR.styrene_conformers()
    ptr, idx, kind = planar_groups(_item(mol))
    ref = PR.planar(pos, ptr, idx, 0.25)
    PR.assert_margins(ref, pos, 0.25, ties=True)                              # (the flat conformer's two groups are both at 0)
    assert ref["n_bent"].tolist() == [0, 1, 1, 0] and ref["worst_group"][1:3].tolist() == [0, 1] and kind.tolist() == [0, 1]
    assert 0.28 < ref["dev"][1, 0] < 0.30 and ref["dev"][1, 1] < 1e-6 and ref["dev"][2, 0] < 1e-6 and 0.39 < ref["dev"][2, 1] < 0.40
    assert ref["dev"][0].max() < 1e-6 and ref["dev"][3].max() < 0.03


def test_the_random_cases_of_the_kernel_test_meet_their_own_conditions():
    """what tests/test_hip_planarity.py asks of its inputs, checked here so that a seed that stops meeting it fails without a GPU"""
    for n, G, P in PR.CASES:
        (pos, ptr, idx, shape), ref = PR.case(n, G, P)
        assert pos.shape == (G, n, 3) and pos.dtype == np.float32 and ptr.shape == (P + 1,)
        sizes = np.diff(ptr)
        assert P == 0 or (sizes.min() >= 3 and sizes.max() <= 8)
        assert all(len(set(idx[ptr[k]:ptr[k + 1]].tolist())) == sizes[k] for k in range(P))
        if P >= 64:
            assert sorted(set(sizes.tolist())) == [3, 4, 5, 6, 7, 8] and abs(np.bincount(shape, minlength=3) - P / 3).max() < 1
            assert 0 < ref["n_bent"].min() and ref["n_bent"].max() < P
        assert PR.left_out(ref).sum() <= 0.01 * G * P


# ------------------------------------------------------------------------------------------------ 3. exports and refusals
def test_export_define_and_abi_version():
    assert _lib.EXPORTS["agdiff_planar_groups"] == [VP, VP, VP, I32, I32, I32, F32, VP, VP, VP, VP, VP]
    assert _lib.DEFINES["AGDIFF_PLANAR_MAX_ATOMS"] == 8
    lib = _lib.load()
    assert lib.agdiff_abi_version() == _lib.DEFINES["AGDIFF_ABI_VERSION"]
    assert hasattr(lib, "agdiff_planar_groups") and list(lib.agdiff_planar_groups.argtypes) == _lib.EXPORTS["agdiff_planar_groups"]


def test_the_entry_point_checks_its_arguments_on_the_host():
    lib = _lib.load()
    keep = (ctypes.c_uint64 * 8)()
    p, null = ctypes.c_void_p(ctypes.addressof(keep)), ctypes.c_void_p(0)
    ok = dict(pos=p, grp_ptr=p, grp_idx=p, G=2, n=5, P=3, thresh=0.25, dev=null, worst=p, worst_group=p, n_bent=p)

    def planar(**kw):
        a = dict(ok, **kw)
        return lib.agdiff_planar_groups(a["pos"], a["grp_ptr"], a["grp_idx"], a["G"], a["n"], a["P"], a["thresh"], a["dev"], a["worst"],
                                        a["worst_group"], a["n_bent"], null)
    for bad in (dict(pos=null), dict(worst=null), dict(worst_group=null), dict(n_bent=null), dict(grp_ptr=null), dict(grp_idx=null),
                dict(G=-1), dict(P=-1), dict(n=-2), dict(n=0), dict(G=0, n=0), dict(thresh=float("nan")), dict(thresh=-0.1),
                dict(thresh=float("inf")), dict(G=0, thresh=float("nan")), dict(G=0, P=0, thresh=-1.0)):
        assert planar(**bad) == -1, bad
    assert planar(G=0) == 0 and planar(G=0, dev=p) == 0 and planar(G=0, thresh=0.0) == 0
    assert planar(G=0, P=0, grp_ptr=null, grp_idx=null) == 0
    del keep


def test_wrapper_checks_come_before_any_launch():
    import torch
    from agdiff_amd import planarity as PL
    ptr, idx = np.array([0, 3], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32)
    for bad_ptr, bad_idx, what in (([1, 4], [0, 1, 2, 0], "start at 0"), ([0, 3, 2], [0, 1, 2], "end at"), ([0, 3], [0, 1], "end at"),
                                   ([0, 2, 5], [0, 1, 2, 0, 1], "3 .. 8"), ([0, 9], list(range(9)), "3 .. 8"),
                                   ([0, 4, 3, 7], list(range(7)), "3 .. 8"), ([0, 3], [0, 1, 5], "outside"), ([0, 3], [-1, 1, 2], "outside"),
                                   ([], [], "P \\+ 1"), ([[0, 3]], [0, 1, 2], "one-dimensional")):
        with pytest.raises(ValueError, match=what):
            PL.check_groups(5, np.array(bad_ptr, dtype=np.int64), np.array(bad_idx, dtype=np.int32))
    with pytest.raises(ValueError, match="integer"):
        PL.check_groups(5, np.array([0.0, 3.0]), idx)
    got = PL.check_groups(3, ptr.astype(np.int64), torch.from_numpy(idx))
    assert all(g.dtype == np.int32 and np.array_equal(g, w) for g, w in zip(got, (ptr, idx)))
    assert PL.check_groups(3, [0], [])[0].tolist() == [0]
    pos = torch.zeros((2, 3, 3))
    for bad in (pos, pos.double(), pos.numpy()):
        with pytest.raises(ValueError, match="on the GPU"):
            PL.planar_deviation(bad, ptr, idx)
    mol, gen = PR.styrene_conformers()
    with pytest.raises(ValueError, match="threshold"):
        PL.check_planarity(_item(mol, pos_gen=gen), thresh=-0.1, device="cpu")
    with pytest.raises(ValueError, match="threshold"):
        PL.check_planarity(_item(mol, pos_gen=gen), thresh=float("nan"), device="cpu")
    with pytest.raises(ValueError, match="bonds"):
        PL.check_planarity(dict(atom_type=mol[0], pos_gen=gen), device="cpu")
    with pytest.raises(ValueError, match="outside"):
        PL.check_planarity(_item(mol, pos_gen=gen), groups=([0, 3], [0, 1, 16]), device="cpu")
    with pytest.raises(ValueError, match="kinds"):
        PL.check_planarity(_item(mol, pos_gen=gen), groups=([0, 3], [0, 1, 2], [0, 1]), device="cpu")
    with pytest.raises(ValueError, match="grp_ptr, grp_idx"):
        PL.check_planarity(_item(mol, pos_gen=gen), groups=([0, 3],), device="cpu")
    with pytest.raises(ValueError, match="on the GPU"):                       # (everything on the host passed: the launch is next)
        PL.check_planarity(_item(mol, pos_gen=gen), device="cpu")


def test_command_lines_and_signatures(tmp_path):
    import argparse
    import inspect
    from agdiff_amd import driver, ensemble, planarity
    missing, out = str(tmp_path / "none.npz"), str(tmp_path / "o.npz")
    for bad in ("-0.1", "nan", "inf"):
        with pytest.raises(SystemExit) as e:
            planarity.main(["--samples", missing, "--testset", missing, "--thresh", bad, "--out", out])
        assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        planarity.main(["--samples", missing, "--out", out])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        ensemble.main(["--samples", missing, "--prune-rms", "0.5", "--drop-bent", "--out", out])          # no test set: no bonds
    assert e.value.code == 2
    # (argument parsing only: each main gets past its parser and fails on the first file it opens)
    with pytest.raises(FileNotFoundError):
        planarity.main(["--samples", missing, "--testset", missing, "--thresh", "0.3", "--per-group", "--out", out])
    with pytest.raises(FileNotFoundError):
        ensemble.main(["--samples", missing, "--testset", missing, "--prune-rms", "0.5", "--drop-bent", "--drop-invalid", "--out", out])
    assert not (tmp_path / "o.npz").exists()
    seen = {}
    real = argparse.ArgumentParser.parse_args

    def spy(self, argv=None, namespace=None):
        seen["args"] = real(self, argv, namespace)
        raise KeyboardInterrupt                        # (stop driver.main right after its parser: no checkpoint, no GPU)
    argparse.ArgumentParser.parse_args = spy
    try:
        for extra, want in (([], False), (["--check-planarity"], True)):
            with pytest.raises(KeyboardInterrupt):
                driver.main(["--ckpt", missing, "--testset", missing, "--out", str(tmp_path)] + extra)
            assert seen["args"].check_planarity is want and seen["args"].check_geometry is False
    finally:
        argparse.ArgumentParser.parse_args = real
    from agdiff_amd import postprocess
    assert inspect.signature(driver.run_job).parameters["check_planarity"].default is False
    assert any("check_planarity" in step.switches for step in postprocess.STEPS)
    sig = inspect.signature(planarity.check_planarity).parameters
    assert list(sig) == ["item", "thresh", "groups", "device", "want_dev"]
    assert [sig[k].default for k in ("thresh", "groups", "device", "want_dev")] == [0.25, None, "cuda", False]
    sig = inspect.signature(planarity.planar_deviation).parameters
    assert list(sig) == ["pos", "grp_ptr", "grp_idx", "thresh", "want_dev"] and sig["thresh"].default == 0.25
