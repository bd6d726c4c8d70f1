"""CPU: the constraint table of the sampler (agdiff_amd/constraints.py): its order and keywords, what `build` makes of a run's
keywords and what it refuses, the shared prologue of the stand-alone launchers, and the two restrained command lines' defaults.
Nothing here computes on a GPU."""
import numpy as np
import pytest
import torch

from agdiff_amd import _lib, constraints, core, epsnet, restraints
from agdiff_amd import torsion_restraints as TR
from test_torsion_restraints_cpu import _batch3, _NoGpu

C = constraints


def _keywords():
    """Three conformers of test_torsion_restraints_cpu's chain molecule (12 atoms each): one distance restraint and one torsion
    restraint per conformer, and a core of atoms 0 and 6 (both on the 0 .. 2 side of the bond 2 - 3)."""
    N, bi, bt, batch = _batch3()
    off = 12 * np.arange(3)
    select = np.zeros(N, dtype=bool)
    select[np.concatenate([off, off + 6])] = True
    kw = dict(restraint_pairs=np.stack([off, off + 5], axis=1), restraint_lo=[1.0] * 3, restraint_hi=[2.0] * 3,
              torsion_quads=off[:, None] + np.array([[1, 2, 3, 4]]), torsion_target=[0.5] * 3, torsion_tol=[0.1] * 3,
              core_pos=np.zeros((N, 3), dtype=np.float32), core_select=select)
    return N, bi, bt, batch, kw


def test_order_and_keywords():
    assert C.ORDER == (C.PairRestraints, C.TorsionRestraints, C.CoreHold)
    names = [k for cls in C.ORDER for k in cls.KEYWORDS]
    assert len(names) == len(set(names)) == 16
    assert set(names) == {"restraint_pairs", "restraint_lo", "restraint_hi", "restraint_weight", "restraint_start_sigma", "restraint_sweeps",
                          "torsion_quads", "torsion_target", "torsion_tol", "torsion_sides", "torsion_weight", "torsion_start_sigma",
                          "core_pos", "core_select", "core_weight", "core_start_sigma"}
    assert restraints.SAMPLER_KEYWORDS == C.PairRestraints.KEYWORDS and TR.SAMPLER_KEYWORDS == C.TorsionRestraints.KEYWORDS
    for cls in C.ORDER:
        assert all(callable(getattr(cls, name)) for name in ("from_keywords", "attach", "after_update", "measure", "collect"))


def test_build_without_constraints_is_empty():
    N, bi, bt, batch, _ = _keywords()
    empty = [{}, dict(n_steps=5, save_traj=False),
             dict(restraint_pairs=np.zeros((0, 2), dtype=np.int32), restraint_lo=[], restraint_hi=[], restraint_weight=0.5),
             dict(torsion_quads=[], torsion_target=[], torsion_tol=[], torsion_weight=0.5, torsion_start_sigma=0.3),
             dict(core_pos=None, core_select=None, core_weight=0.5)]
    for kw in empty + [{k: v for d in empty for k, v in d.items()}]:
        assert C.build(N, batch, bi, bt, 3, kw) == []


def test_build_makes_the_constraints_in_order_and_hands_the_core_to_the_others():
    N, bi, bt, batch, kw = _keywords()
    made = C.build(N, batch, bi, bt, 3, dict(kw, restraint_sweeps=3, torsion_weight=0.5, core_start_sigma=0.7, n_steps=5))
    assert [type(c) for c in made] == list(C.ORDER)
    pairs, tors, hold = made
    assert (pairs.sweeps, pairs.weight, pairs.start, tors.weight, tors.start, hold.weight, hold.start) == (3, 1.0, float("inf"), 0.5,
                                                                                                            float("inf"), 1.0, 0.7)
    assert hold.select.dtype == np.uint8 and hold.select.tolist() == kw["core_select"].astype(int).tolist()
    assert pairs.fixed is hold.select                                   # the core's atoms stay where they are
    # the sides avoid the core: 0 and 6 lie on u's side of 2 - 3, so v's side turns although it is the larger one -- exactly what
    # batch_sides(frozen=...) gives
    want_q, want_sides = TR.batch_sides(N, bi, bt, batch, kw["torsion_quads"], frozen=kw["core_select"])
    assert tors.quads.tolist() == want_q.tolist() == kw["torsion_quads"].tolist()
    assert all(a.tolist() == b.tolist() for a, b in zip((tors.side_row, tors.side_ptr, tors.side_idx), want_sides))
    assert tors.side_idx.tolist() == [3, 4, 5, 7, 8, 9, 10, 11]
    free = C.build(N, batch, bi, bt, 3, {k: v for k, v in kw.items() if not k.startswith("core_")})
    assert [type(c) for c in free] == [C.PairRestraints, C.TorsionRestraints] and free[0].fixed is None
    assert free[1].quads.tolist() == kw["torsion_quads"][:, ::-1].tolist() and free[1].side_idx.tolist() == [0, 1, 2, 6]
    # a core atom on both sides of the bond: the quad is only measured
    both = kw["core_select"].copy()
    both[[10, 22, 34]] = True
    tors = C.build(N, batch, bi, bt, 3, dict(kw, core_select=both))[1]
    assert tors.side_row.tolist() == [-1, -1, -1] == TR.batch_sides(N, bi, bt, batch, kw["torsion_quads"], frozen=both)[1][0].tolist()
    # one kind alone
    assert [type(c) for c in C.build(N, batch, None, None, 3, {k: v for k, v in kw.items() if k.startswith("core_")})] == [C.CoreHold]


def test_the_sides_are_walked_once_per_run():
    N, bi, bt, batch, kw = _keywords()
    calls, real = [], TR.batch_sides
    TR.batch_sides = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        C.build(N, batch, bi, bt, 3, kw)
        assert len(calls) == 1
        at, T = torch.full((N,), 6), torch.from_numpy
        with pytest.raises(AssertionError, match="reached the device"):                     # the checks are done, the device is next
            epsnet.DualEncoderEpsNetwork.begin_sampling(_NoGpu(), at, None, T(bi), T(bt), T(batch), 3, False, **kw)
        assert len(calls) == 2
        made = C.build(N, batch, bi, bt, 3, kw)
        with pytest.raises(AssertionError, match="reached the device"):                     # a run that is handed its list builds none
            epsnet.LangevinRun(_NoGpu(), at, None, T(bi), T(bt), T(batch), 3, False, 2, 1e-6, 1000.0, None, None, 0.5, 1.0, constraints=made, **kw)
        assert len(calls) == 3
        with pytest.raises(AssertionError, match="reached the device"):                     # constructed directly: it builds its own, once
            epsnet.LangevinRun(_NoGpu(), at, None, T(bi), T(bt), T(batch), 3, False, 2, 1e-6, 1000.0, None, None, 0.5, 1.0, **kw)
        assert len(calls) == 4
    finally:
        TR.batch_sides = real


def test_build_refuses_what_the_argument_checks_refuse():
    N, bi, bt, batch, kw = _keywords()

    def message(fn, *a, **k):
        with pytest.raises((ValueError, _lib.AgdiffLimitError)) as e:
            fn(*a, **k)
        return type(e.value), str(e.value)

    for bad, direct in ((dict(core_weight=1.5), lambda k: core.core_arguments(N, k["core_pos"], k["core_select"], k["core_weight"])),
                        (dict(core_select=None), lambda k: core.core_arguments(N, k["core_pos"], None)),
                        (dict(restraint_lo=[3.0] * 3), lambda k: restraints.sampler_arguments(N, batch, **{n: k[n] for n in k if n.startswith("restr")})),
                        (dict(restraint_sweeps=0), lambda k: restraints.sampler_arguments(N, batch, **{n: k[n] for n in k if n.startswith("restr")})),
                        (dict(torsion_tol=[4.0] * 3), lambda k: TR.sampler_arguments(N, batch, **{n: k[n] for n in k if n.startswith("tors")})),
                        (dict(torsion_start_sigma=float("nan")), lambda k: TR.sampler_arguments(N, batch, **{n: k[n] for n in k if n.startswith("tors")}))):
        given = dict(kw, **bad)
        assert message(C.build, N, batch, bi, bt, 3, given) == message(direct, given), bad
    many = _lib.DEFINES["AGDIFF_RESTRAIN_MAX_ATOMS"] + 1
    crowd = dict(restraint_pairs=np.stack([np.zeros(many, dtype=np.int64), 1 + np.arange(many)], axis=1), restraint_lo=np.zeros(many),
                 restraint_hi=np.ones(many))
    kind, text = message(C.build, many + 1, np.zeros(many + 1, dtype=np.int64), None, None, 1, crowd)
    assert kind is _lib.AgdiffLimitError and text == message(restraints.sampler_arguments, many + 1, np.zeros(many + 1, dtype=np.int64), **crowd)[1]
    # torsion restraints without bonds and without a side table: nothing could turn
    no_bonds = {k: v for k, v in kw.items() if k.startswith("tors")}
    assert message(C.build, N, batch, None, None, 3, no_bonds) == (
        ValueError, "torsion restraints need the batch's bonds (bond_index, bond_type) or a side table (torsion_sides)")
    assert message(C.weight_and_start, 0.0, 1.0, "weight %r", "start") == (ValueError, "weight 0.0")
    assert message(C.weight_and_start, 0.5, float("nan"), "weight %r", "start") == (ValueError, "start")
    assert C.weight_and_start(1, float("inf"), "", "") == (1.0, float("inf"))


def test_launch_prologue_refuses_before_the_device():
    pos, batch = np.zeros((5, 3), dtype=np.float32), np.array([0, 0, 1, 1, 1])
    for bad, text in ((dict(pos=np.zeros((5, 2))), "pos must have shape [N, 3], got (5, 2)"),
                      (dict(pos=torch.zeros(15)), "pos must have shape [N, 3], got (15,)"),
                      (dict(batch=batch[:4]), "batch has 4 entries, pos 5 atoms"),
                      (dict(batch=batch[::-1]), "batch must hold sorted, non-negative graph ids"),
                      (dict(copy_out=torch.zeros(5, 3)), "copy_out must be a contiguous float32 tensor [N, 3] on the GPU"),
                      (dict(copy_out=np.zeros((5, 3), dtype=np.float32)), "copy_out must be a contiguous float32 tensor [N, 3] on the GPU"),
                      (dict(skip=[0, 1, 0]), "skip has 3 entries, the batch 2 graphs")):
        args = dict(dict(pos=pos, batch=batch, skip=None, copy_out=None), **bad)
        with pytest.raises(ValueError) as e:
            C.launch_prologue(args["pos"], args["batch"], args["skip"], args["copy_out"], "cuda")
        assert str(e.value) == text
        rest = dict(skip=args["skip"], copy_out=args["copy_out"])
        for launch in (lambda: core.hold_core(args["pos"], pos, np.ones(5), args["batch"], **rest),
                       lambda: restraints.restrain_pairs(args["pos"], [[0, 1]], [1.0], [2.0], args["batch"], **rest),
                       lambda: TR.restrain_torsions(args["pos"], [[0, 1, 2, 3]], [0.0], [0.1], args["batch"], None, **rest)):
            with pytest.raises(ValueError) as e:            # the launchers go through it first
                launch()
            assert str(e.value) == text


DEFAULTS = dict(ckpt=None, testset="t.npz", out="o", num_confs="2x", start_idx=0, end_idx=200, n_steps=5000, w_global=1.0, global_start_sigma=0.5,
                clip=1000.0, weight=1.0, start_sigma=float("inf"), seed=2021, noise="default", precision=None, trust_ckpt=False, report=False,
                samples=None, device="cuda")


def test_the_two_command_lines_keep_their_defaults():
    d = restraints.build_parser().parse_args(["--testset", "t.npz", "--out", "o"])
    assert vars(d) == dict(DEFAULTS, sweeps=1)
    t = TR.build_parser().parse_args(["--testset", "t.npz", "--out", "o"])
    assert vars(t) == DEFAULTS
    for ap, module in ((restraints.build_parser(), restraints), (TR.build_parser(), TR)):
        assert ap.description == module.main.__doc__
        with pytest.raises(SystemExit):
            ap.parse_args(["--out", "o"])                   # --testset and --out are required
    text = restraints.build_parser().format_help()
    assert "Jacobi sweeps per step, 1 .. 16" in text and text.index("--start-sigma") < text.index("--sweeps") < text.index("--seed")
    assert "--sweeps" not in TR.build_parser().format_help()
