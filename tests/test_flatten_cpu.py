"""No GPU: the host side of the flattening repair (agdiff_amd/planarity.py: membership_csr, relax_planar's and repair_planarity's
checks), the C ABI of agdiff_relax_planar as the header declares it and its host-side argument checks (every one returns before any
launch), the switches of the command lines, and the float64 restatement of the rule (tests/flatten_ref.py) on hand-built molecules:
what it flattens, in how many updates.  The counts are what the restatement gives for these inputs on the CPU (table bounds, thresh
0.25, flat_to 0.10, pad 0.02, omega 1.0); the kernel is not asked here."""
import ctypes
import inspect

import numpy as np
import pytest

import flatten_ref as FR
import planarity_ref as PR
import relax_ref as RR
import validity_ref as VR
from agdiff_amd import _lib

VP, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float


def test_export_defines_and_abi_version():
    assert _lib.EXPORTS["agdiff_relax_planar"] == [VP] * 12 + [I32] * 4 + [F32] * 3 + [I32] + [F32] * 2 + [VP] * 6
    assert _lib.DEFINES["AGDIFF_FLATTEN_MAX_GROUPS"] == 192 and _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    # the 1024-atom instantiation's static LDS: two fp64 position buffers, the radii, six fp64 per group -- inside 64 KB
    assert 2 * 3 * 8 * _lib.DEFINES["AGDIFF_RELAX_MAX_ATOMS"] + 4 * _lib.DEFINES["AGDIFF_RELAX_MAX_ATOMS"] + 48 * 192 + 64 <= 65536
    lib = _lib.load()
    assert lib.agdiff_abi_version() == 48
    assert hasattr(lib, "agdiff_relax_planar") and list(lib.agdiff_relax_planar.argtypes) == _lib.EXPORTS["agdiff_relax_planar"]
    with pytest.raises(_lib.AgdiffLimitError, match="AGDIFF_FLATTEN_MAX_GROUPS = 192 planar groups for agdiff_relax_planar"):
        _lib.check(-2, "agdiff_relax_planar")


def test_the_entry_point_checks_its_arguments_on_the_host():
    lib = _lib.load()
    keep, other = (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)()
    p, q, null = ctypes.c_void_p(ctypes.addressof(keep)), ctypes.c_void_p(ctypes.addressof(other)), ctypes.c_void_p(0)
    names = ("pos", "bd_ptr", "bd_idx", "bd_lo", "bd_hi", "radius", "ex_ptr", "ex_idx", "grp_ptr", "grp_idx", "mb_ptr", "mb_grp", "G", "n",
             "K", "P", "clash", "pad", "omega", "max_iter", "thresh", "flat_to", "pos_out", "status", "iters", "resid", "moved")
    ok = dict(dict.fromkeys(names, p), G=2, n=5, K=3, P=2, clash=0.6, pad=0.02, omega=1.0, max_iter=200, thresh=0.25, flat_to=0.10,
              pos_out=q)

    def relax(**kw):
        a = dict(ok, **kw)
        return lib.agdiff_relax_planar(*[a[k] for k in names], null)
    nan, inf = float("nan"), float("inf")
    for bad in ([{k: null} for k in ("pos", "bd_ptr", "bd_idx", "bd_lo", "bd_hi", "radius", "ex_ptr", "grp_ptr", "grp_idx", "mb_ptr", "mb_grp",
                                     "pos_out", "status", "iters", "resid", "moved")]
                + [dict(pos_out=p), dict(G=-1), dict(n=0), dict(K=-1), dict(P=-1), dict(max_iter=0), dict(max_iter=10001), dict(pad=0.0),
                   dict(pad=nan), dict(omega=2.0), dict(clash=-0.1), dict(thresh=nan), dict(thresh=inf), dict(thresh=-0.25),
                   dict(flat_to=nan), dict(flat_to=inf), dict(flat_to=-0.1), dict(flat_to=0.24), dict(flat_to=0.2, pad=0.06),
                   dict(thresh=0.1), dict(G=0, thresh=nan), dict(G=0, flat_to=0.3), dict(G=0, P=-1)]):
        assert relax(**bad) == -1, bad
    cap, big = _lib.DEFINES["AGDIFF_FLATTEN_MAX_GROUPS"], _lib.DEFINES["AGDIFF_RELAX_MAX_ATOMS"] + 1
    assert relax(P=cap + 1) == -2 and relax(P=cap + 1, G=0) == -2 and relax(n=big) == -2 and relax(P=cap + 1, flat_to=0.3) == -1
    # G = 0 returns at once; P = 0 goes with null group tables; flat_to + pad may equal thresh
    assert relax(G=0) == 0 and relax(G=0, P=cap, n=big - 1) == 0 and relax(G=0, flat_to=0.0, thresh=0.02) == 0
    assert relax(G=0, P=0, grp_ptr=null, grp_idx=null, mb_ptr=null, mb_grp=null) == 0
    assert relax(G=0, K=0, bd_idx=null, bd_lo=null, bd_hi=null, ex_idx=null) == 0
    del keep, other


def test_membership_csr_lists_the_groups_of_every_atom_ascending():
    from agdiff_amd.planarity import membership_csr
    ptr, grp = membership_csr(4, np.zeros(1, np.int32), np.zeros(0, np.int32))
    assert ptr.tolist() == [0] * 5 and grp.shape == (0,) and ptr.dtype == grp.dtype == np.int32
    # three groups that share atoms, members not in atom order within the table
    ptr, grp = membership_csr(7, [0, 3, 7, 10], [4, 1, 2, 0, 1, 2, 6, 6, 2, 5])
    assert ptr.tolist() == [0, 1, 3, 6, 6, 7, 8, 10]
    assert [grp[ptr[i]:ptr[i + 1]].tolist() for i in range(7)] == [[1], [0, 1], [0, 1, 2], [], [0], [2], [1, 2]]
    # styrene: ring atom 0 carries the substituent and sits in both groups; the ring hydrogens are in none
    mol, _ = PR.styrene()
    tab = FR.tables(mol)
    ptr, grp = membership_csr(16, tab[0], tab[1])
    assert np.diff(ptr).tolist() == [2, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1] and grp[:2].tolist() == [0, 1]
    for case in ("naphthalene", "styrene_x20_full"):
        inputs = FR.solved(case)[0]
        got, want = membership_csr(inputs[0].shape[1], inputs[1], inputs[2]), FR.membership(inputs[0].shape[1], inputs[1], inputs[2])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for kw, what in ((dict(grp_ptr=[0, 2], grp_idx=[0, 1]), "3 .. 8"), (dict(grp_ptr=[0, 3], grp_idx=[0, 1, 7]), "outside"), (dict(grp_ptr=[1, 4]), "start at 0"),
                     (dict(grp_ptr=[0.0, 3.0]), "integer")):
        with pytest.raises(ValueError, match=what):
            membership_csr(7, **dict(dict(grp_ptr=[0, 3], grp_idx=[0, 1, 2]), **kw))


def test_the_new_functions_refuse_bad_input_before_any_launch():
    import torch
    from agdiff_amd import planarity as P
    for kw, what in ((dict(flat_to=-0.1), "flat_to"), (dict(flat_to=float("nan")), "flat_to"), (dict(flat_to=float("inf")), "flat_to"),
                     (dict(flat_to=0.24), "flat_to \\+ pad <= thresh"), (dict(thresh=0.1), "flat_to \\+ pad <= thresh"),
                     (dict(pad=0.2), "flat_to \\+ pad <= thresh"), (dict(thresh=float("nan")), "threshold"), (dict(thresh=-1.0), "threshold")):
        with pytest.raises(ValueError, match=what):
            P._flatten_params(**dict(dict(thresh=0.25, flat_to=0.10, pad=0.02), **kw))
    assert P._flatten_params(0.25, 0.10, 0.02) == (0.25, 0.10) and P._flatten_params(0.125, 0.10, 0.02) == (0.125, 0.10)
    mol, four = PR.styrene_conformers()
    tab = FR.tables(mol)
    with pytest.raises(ValueError, match="on the GPU"):
        P.relax_planar(torch.zeros((2, 16, 3)), *tab)
    item = FR.item_of(mol, pos_gen=four)
    # repair_planarity: the groups and the tables are built and checked first; on a CPU it ends at the launch's own demand
    with pytest.raises(ValueError, match="on the GPU"):
        P.repair_planarity(item, device="cpu")
    with pytest.raises(ValueError, match="groups must be"):
        P.repair_planarity(item, groups=(tab[0],), device="cpu")
    with pytest.raises(ValueError, match="3 .. 8"):
        P.repair_planarity(item, groups=([0, 2], [0, 1]), device="cpu")
    with pytest.raises(ValueError, match="outside"):
        P.repair_planarity(item, groups=([0, 3], [0, 1, 16]), device="cpu")
    with pytest.raises(ValueError, match="bounds"):
        P.repair_planarity(item, bounds="mmff", device="cpu")
    with pytest.raises(ValueError, match="pos_ref"):
        P.repair_planarity(item, bounds="references", device="cpu")
    # not MMFF: the evaluator's switch still refuses
    from agdiff_amd import evaluation
    assert "NotImplementedError" in inspect.getsource(evaluation) and "use_force_field" in inspect.getsource(evaluation)


def test_signatures_and_command_line_switches(tmp_path):
    import argparse
    from agdiff_amd import driver, planarity, postprocess
    for name in ("repair_planarity", "repair_geometry"):
        assert inspect.signature(driver.run_job).parameters[name].default is False
        assert any(name in step.switches for step in postprocess.STEPS)
    sig = inspect.signature(planarity.relax_planar).parameters
    assert list(sig) == ["pos", "grp_ptr", "grp_idx", "pairs", "lo", "hi", "radius", "ex_ptr", "ex_idx", "thresh", "flat_to", "clash", "pad",
                         "omega", "max_iter"]
    assert [sig[k].default for k in ("thresh", "flat_to", "clash", "pad", "omega", "max_iter")] == [0.25, 0.10, 0.60, 0.02, 1.0, 200]
    sig = inspect.signature(planarity.repair_planarity).parameters
    assert list(sig)[:3] == ["item", "groups", "bounds"] and sig["groups"].default is None and sig["bounds"].default == "table"
    assert [sig[k].default for k in ("thresh", "flat_to", "clash", "pad", "omega", "max_iter", "device")] == [0.25, 0.10, 0.60, 0.02, 1.0, 200,
                                                                                                                "cuda"]
    assert list(inspect.signature(planarity.membership_csr).parameters) == ["n", "grp_ptr", "grp_idx"]
    missing = str(tmp_path / "none.npz")
    base = ["--samples", missing, "--testset", missing, "--out", str(tmp_path / "o.npz"), "--repair", str(tmp_path / "r.npz")]
    with pytest.raises(FileNotFoundError):            # (past the parser: fails on the first file it opens)
        planarity.main(base + ["--flat-to", "0.05", "--pad", "0.03", "--omega", "1.5", "--max-iter", "50", "--thresh", "0.3"])
    for bad in (["--pad", "0"], ["--omega", "2"], ["--max-iter", "0"], ["--flat-to", "-0.1"], ["--flat-to", "0.24"], ["--thresh", "0.1"]):
        with pytest.raises(SystemExit) as e:
            planarity.main(base + bad)
        assert e.value.code == 2
    seen = {}
    real = argparse.ArgumentParser.parse_args

    def spy(self, argv=None, namespace=None):
        seen["args"] = real(self, argv, namespace)
        raise KeyboardInterrupt                        # (stop driver.main right after its parser: no checkpoint, no GPU)
    argparse.ArgumentParser.parse_args = spy
    try:
        for extra, want in (([], (False, False)), (["--repair-planarity"], (True, False)),
                            (["--repair-planarity", "--repair-geometry"], (True, True))):
            with pytest.raises(KeyboardInterrupt):
                driver.main(["--ckpt", missing, "--testset", missing, "--out", str(tmp_path)] + extra)
            assert (seen["args"].repair_planarity, seen["args"].repair_geometry) == want and seen["args"].check_planarity is False
    finally:
        argparse.ArgumentParser.parse_args = real
    assert not (tmp_path / "o.npz").exists() and not (tmp_path / "r.npz").exists()


def _judge(inputs, pos):
    """(n_bad, n_clash, n_bent) per conformer by the float64 restatements of the three CHECKS, at the true bounds and at thresh"""
    _, grp_ptr, grp_idx, pairs, lo, hi, radius, ex_ptr, ex_idx = inputs
    nbad = VR.pair_bounds(pos, pairs, lo, hi)[4]
    ncl = VR.clash_scan(pos, radius, VR.excluded_set(ex_ptr, ex_idx), RR.CLASH)[2]
    return nbad.tolist(), ncl.tolist(), PR.planar(pos, grp_ptr, grp_idx, FR.THRESH)["n_bent"].tolist()


# (case, max_iter) -> (status, iters) per conformer
PINNED = {
    ("styrene4", 200): ([0, 1, 1, 0], [0, 25, 14, 0]),
    ("boat", 200): ([1], [26]),
    ("boat_stretched", 200): ([1], [27]),
    ("acetone", 200): ([1], [21]),
    ("naphthalene", 200): ([1], [20]),
    ("vinyl85", 200): ([1], [14]),
    ("vinyl90", 200): ([1], [13]),
    ("mixed", 200): ([0, 1, 1, 1, 3, 1], [0, 27, 4, 27, 0, 25]),
    ("mixed", 5): ([0, 2, 1, 2, 3, 2], [0, 5, 4, 5, 0, 5]),
    ("styrene_x9", 200): ([1, 1], [25, 26]),
    ("styrene_x20", 200): ([1, 1], [26, 26]),
    ("styrene_x20_full", 200): ([1], [34]),
}


@pytest.mark.parametrize("key,max_iter", sorted(PINNED))
def test_the_reference_flattens_what_it_should(key, max_iter):
    inputs, fwd, rev = FR.solved(key, max_iter=max_iter)
    status, iters = PINNED[(key, max_iter)]
    assert fwd["status"].tolist() == status and fwd["iters"].tolist() == iters
    assert rev["status"].tolist() == status and rev["iters"].tolist() == iters
    pos = inputs[0]
    fin = [g for g, st in enumerate(status) if st != 3]
    before, after = _judge(inputs, pos[fin]), _judge(inputs, fwd["pos"][fin])
    for k, g in enumerate(fin):
        st = status[g]
        broken = before[0][k] > 0 or before[1][k] > 0 or before[2][k] > 0
        assert broken == (st != 0)
        if st == 0:
            assert np.array_equal(fwd["pos"][g], pos[g]) and fwd["resid"][g] == 0.0 and fwd["moved"][g] == 0.0
        if st == 1:                                    # repaired: the fp32 result passes all three checks, and little was moved
            assert (after[0][k], after[1][k], after[2][k]) == (0, 0, 0) and fwd["resid"][g] <= RR.PAD / 2 and 0.0 < fwd["moved"][g] < 0.5
            dev = PR.planar(fwd["pos"][g], inputs[1], inputs[2], FR.THRESH)["dev"]
            assert dev.max() <= FR.FLAT_TO + RR.PAD / 2 + 1e-6
        if st == 2:
            assert fwd["iters"][g] == max_iter and fwd["resid"][g] > RR.PAD / 2
    # the two routes (summation order, eigh against SVD) differ by accumulated float64 rounding only; the normals are well determined
    assert np.nanmax(np.abs(fwd["pos64"][fin] - rev["pos64"][fin])) < 1e-12 and fwd["gap"].min() >= 0.1


def test_without_groups_the_restatement_is_relax_ref_exactly():
    inputs, fwd, _ = RR.solved("tree23")
    none = (np.zeros(1, np.int32), np.zeros(0, np.int32))
    got = FR.relax(inputs[0], *none, *inputs[1:])
    assert fwd["status"].tolist() == [1, 1, 1, 1]
    for k in ("pos", "pos64", "status", "iters", "resid", "moved"):
        assert np.array_equal(got[k], fwd[k]), k


def test_a_double_bond_twisted_past_ninety_degrees_flattens_into_the_other_isomer():
    # nothing here knows E from Z: the CH2 end turned by 85 degrees falls back, turned by 95 degrees it falls over to the other side.
    # (Not to 0 and 180 exactly: a hydrogen may stay 0.11 A off the plane, which on a 1.09 A bond 0.94 A from the axis is 7 degrees for
    # each end's atoms against their own plane and more against each other: the halves of the circle are told apart at 45 and 135.)
    mol, _ = PR.styrene()
    tab = FR.tables(mol)
    torsion = []
    for deg in (85.0, 95.0):
        res = FR.relax(FR.vinyl_twist(deg)[1], *tab)
        assert res["status"].tolist() == [1]
        p = res["pos64"][0]
        b1, b2, b3 = p[6] - p[13], p[7] - p[6], p[14] - p[7]                       # H13 - C6 = C7 - H14
        n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
        torsion.append(np.degrees(np.arctan2(np.cross(n1, n2) @ b2 / np.linalg.norm(b2), n1 @ n2)))
    assert abs(torsion[0]) < 45.0 and abs(torsion[1]) > 135.0
