"""CPU: the driver's public surface, and the post-sampling chain of agdiff_amd/postprocess.py -- which step runs when, what one hands
the next, which keys and log lines come out.  The sampler is a fake and the modules' entry points are recorders: nothing here
computes on a GPU."""
import inspect

import numpy as np
import pytest
import torch

import ez_cases as EC
from agdiff_amd import dist, driver, postprocess

INF = float("inf")
_REQUIRED = inspect.Parameter.empty

# (name, default) of every parameter, as released
RUN_JOB = [("model", _REQUIRED), ("mols", _REQUIRED), ("out_dir", _REQUIRED), ("confs_of", _REQUIRED), ("max_atoms", _REQUIRED),
           ("sampler_kwargs", _REQUIRED), ("device", _REQUIRED), ("save_traj", False), ("resume", False), ("rank", 0), ("world", 1),
           ("shard", False), ("log", print), ("noise", "default"), ("seed", 2021), ("prune_rms", None), ("fix_handedness", False),
           ("prune_tfd", None), ("track_rmsd", False), ("track_rmsd_mirror", False), ("repair_geometry", False), ("check_planarity", False),
           ("repair_planarity", False), ("hold_core", False), ("core_weight", 1.0), ("core_start_sigma", INF), ("fix_double_bonds", False),
           ("check_geometry", False)]
SAMPLE_BATCH = [("model", _REQUIRED), ("packed", _REQUIRED), ("device", _REQUIRED), ("sampler_kwargs", _REQUIRED), ("save_traj", False),
                ("max_retry", 2), ("log", print), ("pos_init", None), ("noise", None), ("topology", None), ("counter_seed", None),
                ("curves", None), ("core", None)]
SAMPLE_BATCH_SHARDED = [("model", _REQUIRED), ("packed", _REQUIRED), ("device", _REQUIRED), ("sampler_kwargs", _REQUIRED), ("save_traj", False),
                        ("max_retry", 2), ("log", print), ("group", None), ("pos_init", None), ("noise", None), ("topology", None),
                        ("counter_seed", None)]
# dest -> default of driver.main's parser (--ckpt, --testset and --out are required)
FLAGS = dict(num_confs="2x", start_idx=0, end_idx=200, n_steps=5000, w_global=1.0, global_start_sigma=0.5, clip=1000.0, save_traj=False,
             resume=False, extend_order=False, max_atoms=196608, seed=2021, noise="default", prune_rms=None, prune_tfd=None,
             fix_handedness=False, fix_double_bonds=False, check_geometry=False, check_planarity=False, repair_geometry=False,
             repair_planarity=False, track_rmsd=False, track_rmsd_mirror=False, hold_core=False, core_weight=1.0, core_start_sigma=INF,
             precision=None, dist_mode="shard", trust_ckpt=False)


def test_public_surface_is_the_released_one(tmp_path):
    import argparse
    for fn, want in ((driver.run_job, RUN_JOB), (driver.sample_batch, SAMPLE_BATCH), (dist.sample_batch_sharded, SAMPLE_BATCH_SHARDED)):
        assert [(p.name, p.default) for p in inspect.signature(fn).parameters.values()] == want, fn.__name__
    kinds = [p.kind for p in inspect.signature(driver.sample_batch).parameters.values()]
    assert kinds == [inspect.Parameter.POSITIONAL_OR_KEYWORD] * 11 + [inspect.Parameter.KEYWORD_ONLY] * 2
    seen = {}
    real = argparse.ArgumentParser.parse_args

    def spy(self, argv=None, namespace=None):
        seen["args"] = real(self, argv, namespace)
        raise KeyboardInterrupt                        # (stop driver.main right after its parser: no checkpoint, no GPU)
    argparse.ArgumentParser.parse_args = spy
    try:
        with pytest.raises(KeyboardInterrupt):
            driver.main(["--ckpt", "c", "--testset", "t", "--out", str(tmp_path)])
    finally:
        argparse.ArgumentParser.parse_args = real
    assert vars(seen["args"]) == dict(FLAGS, ckpt="c", testset="t", out=str(tmp_path))
    for name in ("prepare_batch", "pack_batch", "plan_batches", "subset_batch", "sharded_capacity", "SAMPLE_STATS", "stream_id", "with_attempt",
                 "load_testset", "save_testset", "merge_outputs", "num_confs"):
        assert hasattr(driver, name), name
    # no function of the three modules but the frozen public ones takes more than 12 parameters
    for mod in (driver, dist, postprocess):
        for name, fn in inspect.getmembers(mod, inspect.isfunction):
            if fn.__module__ == mod.__name__ and fn not in (driver.run_job, driver.sample_batch):
                assert len(inspect.signature(fn).parameters) <= 12, name


STEPS = 4           # denoising steps of the fake sampler
G, N, D = 3, 14, 3  # conformers per molecule (num_confs("3")), atoms and tagged double bonds of c14


class _Run:
    """Stands where epsnet.LangevinRun does: positions = the atom types; graphs whose lightest atom has type 3 fail every attempt."""

    def __init__(self, at, batch, num_graphs, save_traj, mirror, held):
        self.at, self.save_traj = at, save_traj
        first = torch.zeros(num_graphs, dtype=torch.long).scatter_reduce(0, batch, at, "amin", include_self=False)
        self.bad, self.range_graphs = first == 3, set()
        self.rmsd_curve = (torch.arange(STEPS)[:, None] + 10.0 * torch.arange(num_graphs)[None, :]).float()
        self.rmsd_curve_mirror = -self.rmsd_curve if mirror else None
        self.core_dev = torch.arange(num_graphs, dtype=torch.float32) + 0.5 if held else None

    def remaining(self):
        return STEPS

    def advance(self, m):
        self.pos = self.at.to(torch.float32)[:, None].repeat(1, 3)

    def finish(self):
        return self.pos, ([self.pos.clone() for _ in range(STEPS)] if self.save_traj else [])

    def nan_graphs(self):
        return self.bad


class _Sampler:
    def begin_sampling(self, at, pos_init, bi, bt, batch, num_graphs, extend_order, clip_local=None, save_traj=True, raise_on_nan=True,
                       noise=None, n_steps=2, rmsd_target=None, rmsd_mirror=False, **kw):
        return _Run(at, batch, num_graphs, save_traj, rmsd_mirror, "core_pos" in kw)


def _three_molecules():
    """c14 three times: 0 with a core, 1 fails every attempt (its hydrogens carry type 3), 2 plain; all tagged, all with a target"""
    (mol, skeleton, _), (quads, target, _, _) = EC.molecule("c14"), EC.tables("c14")
    mols = [dict(atom_type=np.array(mol[0]), edge_index=mol[1], edge_type=mol[2], num_refs=1, name="m%d" % i, index=i, ez_quads=quads,
                 ez=target, stereo=np.zeros(N, dtype=np.int8), pos_target=skeleton.astype(np.float32)) for i in range(3)]
    mols[1]["atom_type"][mols[1]["atom_type"] == 1] = 3
    mols[0]["core_pos"] = (skeleton + 2.0).astype(np.float32)
    mols[0]["core_mask"] = np.isin(np.arange(N), [0, 1, 2, 3, 8, 9, 10])
    return mols


HAND = [-1, 0, 1]
STATE, AFTER = [[-1, 1, 0], [1, 1, 1], [-1, -1, 1]], [[1, 1, 0], [1, -1, 1], [-1, 1, 1]]
STATUS, VALID, FLAT = [0, 1, 2], [True, False, True], [True, True, False]
CHAIN = ["to_template_frame", "fix_handedness", "fix_double_bonds", "double_bond_verdict", "repair_planarity", "check_geometry",
         "check_planarity", "prune_conformers"]


@pytest.fixture
def calls(monkeypatch):
    """Recorders in the modules' entry points: (name, the shift of the conformers it saw against the sampled ones, what it was handed).
    The ones that move conformers shift them by 1, 10, 100 and 1000, so every later one shows who ran before it."""
    from agdiff_amd import core, ensemble, ezbonds, planarity, stereo, validity
    seen = []

    def note(name, pos, **handed):
        assert torch.is_tensor(pos) and pos.dtype == torch.float32 and tuple(pos.shape) == (G, N, 3) and pos.is_contiguous()
        seen.append((name, float(pos[0, 0, 0]) - 6.0, handed))        # (atom 0 is a carbon: sampled at 6.0)

    def to_template_frame(pos, core_pos, core_mask, device="cuda"):
        note("to_template_frame", pos)
        return pos + 1.0

    def fix_handedness(item, pos):
        note("fix_handedness", pos, stereo=item["stereo"])
        pos += 10.0
        return torch.tensor(HAND, dtype=torch.int32)

    def fix_double_bonds(item, pos, frozen=None):
        note("fix_double_bonds", pos, frozen=frozen)
        pos += 100.0
        return torch.tensor(STATE, dtype=torch.int8)

    def double_bond_verdict(pos, quads, target):
        note("double_bond_verdict", pos)
        return torch.tensor(AFTER, dtype=torch.int8)

    def repair(name):
        def fn(item, device="cuda"):
            note(name, item["pos_gen"])
            return dict(pos=item["pos_gen"] + 1000.0, status=torch.tensor(STATUS, dtype=torch.int32), moved=torch.tensor([0.0, 0.5, 1.5]))
        return fn

    def check_geometry(item, device="cuda"):
        note("check_geometry", item["pos_gen"])
        return dict(valid=torch.tensor(VALID), bond_dev=torch.tensor([0.0, 0.3, 0.0]), clash=torch.tensor([1.0, 0.4, 1.0]))

    def check_planarity(item, device="cuda"):
        note("check_planarity", item["pos_gen"])
        return dict(flat=torch.tensor(FLAT), flat_dev=torch.tensor([0.0, 0.1, 0.9]))

    def prune_conformers(item, threshold, align=True, device="cuda", metric="rmsd", valid=None):
        note("prune_conformers", item["pos_gen"], threshold=threshold, align=align, metric=metric, valid=None if valid is None else valid.tolist())
        return dict(kept=torch.tensor([0], dtype=torch.int32), leader=torch.tensor([0, -1, -1], dtype=torch.int32))

    monkeypatch.setattr(core, "to_template_frame", to_template_frame)
    monkeypatch.setattr(stereo, "fix_handedness", fix_handedness)
    monkeypatch.setattr(ezbonds, "fix_double_bonds", fix_double_bonds)
    monkeypatch.setattr(ezbonds, "double_bond_verdict", double_bond_verdict)
    monkeypatch.setattr(validity, "repair_geometry", repair("repair_geometry"))
    monkeypatch.setattr(planarity, "repair_planarity", repair("repair_planarity"))
    monkeypatch.setattr(validity, "check_geometry", check_geometry)
    monkeypatch.setattr(planarity, "check_planarity", check_planarity)
    monkeypatch.setattr(ensemble, "prune_conformers", prune_conformers)
    return seen


def _job(tmp_path, name, logs, **switches):
    return driver.run_job(_Sampler(), _three_molecules(), str(tmp_path / name), driver.num_confs("3"), 10 ** 6, dict(n_steps=STEPS), "cpu",
                          log=logs.append, **switches)


def _summary(logs):
    """the steps' lines: rank 0's without the per-batch lines and the two about SAMPLE_STATS, which counts since the process started"""
    return [line for line in logs if line.startswith("rank 0: ") and not any(w in line for w in ("batch", "dropped", "split-fp16"))]


EVERY_SWITCH = dict(save_traj=True, prune_rms=0.5, fix_handedness=True, track_rmsd_mirror=True, repair_geometry=True, check_planarity=True,
                    repair_planarity=True, hold_core=True, fix_double_bonds=True, check_geometry=True)


def test_the_tuple_is_the_order():
    assert [s.__name__ for s in postprocess.STEPS] == ["CoreFrame", "Handedness", "DoubleBonds", "Repair", "CheckGeometry", "CheckPlanarity",
                                                       "Prune", "TrackedRmsd"]
    off = {name: default for name, default in RUN_JOB if default is not _REQUIRED}
    assert postprocess.enabled_steps(off) == []
    assert [type(s) for s in postprocess.enabled_steps(dict(off, **EVERY_SWITCH))] == list(postprocess.STEPS)
    assert [type(s) for s in postprocess.enabled_steps(dict(off, prune_tfd=0.0))] == [postprocess.Prune]       # (a threshold of 0 is on)
    assert [s.__name__ for s in postprocess.STEPS if not s.sharded] == ["CoreFrame", "TrackedRmsd"]


def test_every_switch_runs_the_chain_in_order_and_hands_on_what_it_should(tmp_path, calls):
    logs = []
    res = _job(tmp_path, "all", logs, **EVERY_SWITCH)
    # per molecule the literal order; the molecule without a core starts at the handedness; the failed one is never touched
    assert [c[0] for c in calls] == CHAIN + CHAIN[1:]
    # ... every recorder saw the conformers as the ones before it left them (template + 1, hand + 10, E/Z + 100, repair + 1000)
    assert [c[1] for c in calls] == [0.0, 1.0, 11.0, 111.0, 111.0, 1111.0, 1111.0, 1111.0] + [0.0, 10.0, 110.0, 110.0, 1110.0, 1110.0, 1110.0]
    by_name = lambda name: [c[2] for c in calls if c[0] == name]
    frozen0, frozen2 = (h["frozen"] for h in by_name("fix_double_bonds"))
    assert frozen0.dtype == np.bool_ and np.array_equal(frozen0, _three_molecules()[0]["core_mask"]) and frozen2 is None
    both = [v and f for v, f in zip(VALID, FLAT)]
    assert by_name("prune_conformers") == [dict(threshold=0.5, align=False, metric="rmsd", valid=both)] * 2
    keys = ["name", "pos_gen", "hand", "ez_state", "repair_status", "repair_moved", "valid", "bond_dev", "clash", "flat", "flat_dev", "kept",
            "cluster", "rmsd_traj", "rmsd_mirror_traj", "traj"]
    assert sorted(res) == sorted(["%s_0" % k for k in keys + ["core_rmsd"]] + ["%s_2" % k for k in keys])
    at = torch.from_numpy(_three_molecules()[0]["atom_type"]).float()[None, :, None].repeat(G, 1, 3).numpy()
    for i, shift in ((0, 1111.0), (2, 1110.0)):
        assert res["pos_gen_%d" % i].dtype == np.float32 and np.array_equal(res["pos_gen_%d" % i], at + shift)
        assert res["traj_%d" % i].shape == (STEPS, G, N, 3) and np.array_equal(res["traj_%d" % i][-1], at)          # as sampled
        for key, dtype, want in (("hand", np.int8, HAND), ("ez_state", np.int8, STATE), ("repair_status", np.int8, STATUS),
                                 ("repair_moved", np.float32, [0.0, 0.5, 1.5]), ("valid", np.int8, VALID), ("bond_dev", np.float32, [0.0, 0.3, 0.0]),
                                 ("clash", np.float32, [1.0, 0.4, 1.0]), ("flat", np.int8, FLAT), ("flat_dev", np.float32, [0.0, 0.1, 0.9]),
                                 ("kept", np.int32, [0]), ("cluster", np.int32, [0, -1, -1])):
            got = res["%s_%d" % (key, i)]
            assert got.dtype == dtype and np.array_equal(got, np.asarray(want, dtype=dtype)), key
        first = G * i                                                       # (the molecule's first graph in the one batch)
        curve = np.arange(STEPS, dtype=np.float32)[:, None] + 10.0 * np.arange(first, first + G, dtype=np.float32)[None, :]
        assert res["rmsd_traj_%d" % i].dtype == np.float32 and np.array_equal(res["rmsd_traj_%d" % i], curve)
        assert np.array_equal(res["rmsd_mirror_traj_%d" % i], -curve)
    assert res["core_rmsd_0"].dtype == np.float32 and res["core_rmsd_0"].tolist() == [0.5, 1.5, 2.5]
    assert "molecule m1 failed twice (NaN); skipped" in logs
    assert _summary(logs) == [
        "rank 0: 2 conformers were mirror images and were inverted; 2 match neither hand (verdict 0) and stay as sampled",
        "rank 0: 4 of 6 conformers had a double bond of the wrong E/Z parity flipped; 4 bonds stay wrong (in a ring, or held on "
        "both sides) and 2 tagged bonds are undecided (ez_state_<i> = 0)",
        "rank 0: 2 of 6 conformers were repaired (flattened and moved into their distance bounds); 2 more were not within the iteration "
        "limit (repair_status_<i> = 2)",
        "rank 0: 2 of 6 conformers are invalid (a bond length out of bounds or a steric clash) and are marked in valid_<i>",
        "rank 0: 2 of 6 conformers are bent (an aromatic ring or a double bond out of plane) and are marked in flat_<i>"]


def test_fewer_switches_fewer_calls(tmp_path, calls):
    logs = []
    plain = _job(tmp_path, "plain", logs)
    assert calls == [] and sorted(plain) == ["name_0", "name_2", "pos_gen_0", "pos_gen_2"]
    assert not _summary(logs)
    at = torch.from_numpy(_three_molecules()[0]["atom_type"]).float()[None, :, None].repeat(G, 1, 3).numpy()
    assert plain["pos_gen_0"].dtype == np.float32 and np.array_equal(plain["pos_gen_0"], at)
    # the distance repair alone is the distance repair; one check alone is the prune's mask; the TFD prune is a prune
    res = _job(tmp_path, "some", logs, repair_geometry=True, check_planarity=True, prune_tfd=0.25)
    assert [c[0] for c in calls] == ["repair_geometry", "check_planarity", "prune_conformers"] * 2
    assert calls[2][2] == dict(threshold=0.25, align=False, metric="tfd", valid=FLAT)
    assert "rank 0: 2 of 6 conformers were repaired (moved into their distance bounds); 2 more were not within the iteration limit " \
           "(repair_status_<i> = 2)" in logs
    assert sorted(k for k in res if k.endswith("_2")) == ["cluster_2", "flat_2", "flat_dev_2", "kept_2", "name_2", "pos_gen_2", "repair_moved_2",
                                                         "repair_status_2"]
    # hold_core alone: the molecule without a core is the sampler's bytes, and nothing is called for it
    del calls[:]
    held = _job(tmp_path, "held", logs, hold_core=True)
    assert [c[0] for c in calls] == ["to_template_frame"] and np.array_equal(held["pos_gen_2"], at) and np.array_equal(held["pos_gen_0"], at + 1.0)
    assert sorted(held) == ["core_rmsd_0", "name_0", "name_2", "pos_gen_0", "pos_gen_2"]
