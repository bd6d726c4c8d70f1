"""What driver.run_job does to a molecule's conformers once its batch's retries have settled: the steps, in the order users rely on.

STEPS below IS that order.  run_job builds the steps its keywords enable (enabled_steps), lets each check the job before anything is
sampled (require) and runs them over every saved molecule (run_chain), by the rank that writes the batch's file.  The conformers go
down the chain as ONE contiguous float32 tensor [G, n, 3] on the device, uploaded for the first step that reads them and downloaded
once, after the last; with no such step `pos_gen_<i>` is the sampler's bytes.  A step hands the next what it needs through the
molecule's MolContext.  A further step is a class here with its place in STEPS, a run_job keyword and a command-line flag.
"""
from dataclasses import dataclass

import numpy as np

from . import _lib, core, ensemble, ezbonds, planarity, stereo, validity


@dataclass
class MolContext:
    """One molecule's record for the chain.  bonds: the item the modules take (atom_type, edge_index, edge_type), built once; graphs:
    its graphs within the packed batch; sampled: what the steps' sampler_keywords gave driver.sample_batch, filled in by it; mask: bool
    [G] on the device, the conformers every check so far has passed (the prune walks over them); frozen: bool [n], atoms not to move."""
    bonds: dict
    device: object
    graphs: slice
    sampled: dict
    mask: object = None
    frozen: object = None


def has_core(m):
    """The molecule carries a template and a mask that selects an atom."""
    return m.get("core_pos") is not None and m.get("core_mask") is not None and bool(np.asarray(m["core_mask"]).any())


class Step:
    """One step, built from run_job's keywords `sw` when one of its `switches` is set.  needs: (fields every molecule of the test set
    must carry, the error's text).  sharded: whether it runs with graph-sharded sampling -- dist.sample_batch_sharded takes no
    sampler_keywords, so a step that returns any does not.  on_device: whether apply reads the conformers."""
    switches = ()
    needs = ((), "")
    sharded = True
    on_device = True
    thresholds = False                         # (its switches are thresholds, on unless None: 0 is a threshold)

    def __init__(self, sw):
        self.sw = sw

    def require(self, mols, shard, world):
        """ValueError unless the test set carries what the step needs and it runs with the job's way of sampling; before any sampling."""
        missing = [m["name"] for m in mols if any(m.get(k) is None for k in self.needs[0])]
        if missing:
            raise ValueError("%s; missing for %d molecules: %s" % (self.needs[1], len(missing), ", ".join(map(str, missing[:5]))
                                                                 + (" ..." if len(missing) > 5 else "")))
        if shard and not self.sharded:
            raise ValueError("%s does not work with graph-sharded sampling (shard=True, %d ranks: each rank updates only its "
                             "own graphs); use --dist-mode batches" % (self.switches[0], world))

    def sampler_keywords(self, packed):
        """What driver.sample_batch gets for this batch on the step's behalf; what it fills in comes back as ctx.sampled."""
        return {}

    def apply(self, mol, pos, out, ctx):
        """The step over one molecule's conformers `pos` [G, n, 3] on the device: writes its keys into `out`; moves the conformers in
        place, or returns the tensor that takes their place."""

    def summary(self, rank):
        """The step's line of the job's summary, or None on a rank that has nothing to say (one that wrote no file)."""


class CoreFrame(Step):
    """hold_core=True: conformers around a fixed core (agdiff_amd.core).  A molecule with `core_pos` / `core_mask`
    (load_testset: `core_pos_<i>`, `core_mask_<i>`; no molecule with one is an error) is sampled with those atoms held to the
    template's internal geometry (epsnet.LangevinRun: core_weight in (0, 1], core_start_sigma); the others are sampled as ever.  Its
    conformers are superposed on `core_pos_<i>` over the core atoms (`pos_gen_<i>` is in the template's frame); `core_rmsd_<i>` float32
    [G]: how far the last step had pulled each core out of shape before the closing hold.  The core atoms are `frozen` from here on."""
    switches = ("hold_core",)
    sharded = False

    def require(self, mols, shard, world):
        if not any(has_core(m) for m in mols):
            raise ValueError("hold_core needs `core_pos_<i>` and `core_mask_<i>` in the test set; none of the %d molecules has them"
                             % len(mols))
        super().require(mols, shard, world)
        for m in filter(has_core, mols):
            try:
                core.core_arguments(m["atom_type"].shape[0], m["core_pos"], m["core_mask"], self.sw["core_weight"], self.sw["core_start_sigma"])
            except ValueError as e:
                raise ValueError("hold_core, molecule %s: %s" % (m["name"], e))

    def sampler_keywords(self, packed):
        hold = dict(weight=float(self.sw["core_weight"]), start_sigma=float(self.sw["core_start_sigma"]))
        return {"core": hold} if packed.get("core_pos") is not None else {}       # (a batch without a core: sampled as ever)

    def apply(self, mol, pos, out, ctx):
        if not has_core(mol):
            return None
        out["core_rmsd_%d" % mol["index"]] = ctx.sampled["core"]["dev"][ctx.graphs].numpy().astype(np.float32)
        ctx.frozen = np.asarray(mol["core_mask"]).reshape(-1) != 0
        return core.to_template_frame(pos, mol["core_pos"], mol["core_mask"], device=ctx.device)


class Handedness(Step):
    """fix_handedness=True: the sampler cannot tell a molecule from its mirror image, so every conformer's stereocentres are read
    against the molecule's `stereo` tags (load_testset: `stereo_<i>`) and the mirror images are inverted (agdiff_amd.stereo.fix_handedness).
    `pos_gen_<i>` holds the mirrored conformers, `hand_<i>` int8 [G] the verdict before the fix: -1 was mirrored, 0 left as sampled, +1 right."""
    switches = ("fix_handedness",)
    needs = ("stereo",), "fix_handedness needs `stereo_<i>` in the test set (python -m agdiff_amd.stereo adds it)"
    mirrored = undecided = 0

    def apply(self, mol, pos, out, ctx):
        hand = out["hand_%d" % mol["index"]] = stereo.fix_handedness(dict(ctx.bonds, stereo=mol["stereo"]), pos).cpu().numpy().astype(np.int8)
        self.mirrored += int((hand < 0).sum())
        self.undecided += int((hand == 0).sum())

    def summary(self, rank):
        if rank == 0 or self.mirrored or self.undecided:
            return ("rank %d: %d conformers were mirror images and were inverted; %d match neither hand (verdict 0) and stay as sampled"
                    % (rank, self.mirrored, self.undecided))


class DoubleBonds(Step):
    """fix_double_bonds=True: the bond types say "double", not E or Z, so every conformer's tagged double bonds are read against the
    molecule's `ez_quads` / `ez` tags (load_testset: `ez_quads_<i>`, `ez_<i>`) and the wrong ones are turned over, one side of the bond
    by 180 degrees about it (agdiff_amd.ezbonds.fix_double_bonds).  BEFORE the repair: the rotation can bring the two
    sides into contact, which the repair then sees.  The `frozen` atoms never move: the other side turns, and a bond with frozen atoms
    on both sides is left as sampled.  `pos_gen_<i>` holds the flipped conformers, `ez_state_<i>` int8 [G, D] each bond's state before."""
    switches = ("fix_double_bonds",)
    needs = ("ez_quads", "ez"), "fix_double_bonds needs `ez_quads_<i>` and `ez_<i>` in the test set (python -m agdiff_amd.ezbonds adds them)"
    flipped = left = undecided = seen = 0

    def require(self, mols, shard, world):
        super().require(mols, shard, world)
        for m in mols:
            try:
                ezbonds.ez_table(m)
            except ValueError as e:
                raise ValueError("fix_double_bonds, molecule %s: %s" % (m["name"], e))

    def apply(self, mol, pos, out, ctx):
        item = dict(ctx.bonds, ez_quads=mol["ez_quads"], ez=mol["ez"])
        state = out["ez_state_%d" % mol["index"]] = ezbonds.fix_double_bonds(item, pos, frozen=ctx.frozen).cpu().numpy().astype(np.int8)
        after = ezbonds.double_bond_verdict(pos, *ezbonds.ez_table(item)).cpu().numpy()
        self.seen += int(state.shape[0])
        self.flipped += int(((state < 0) & (after > 0)).any(axis=1).sum())
        self.left += int((after < 0).sum())
        self.undecided += int(((state == 0) & (np.asarray(mol["ez"]).reshape(1, -1) != 0)).sum())

    def summary(self, rank):
        if rank == 0 or self.seen:
            return ("rank %d: %d of %d conformers had a double bond of the wrong E/Z parity flipped; %d bonds stay wrong (in a ring, or held on "
                    "both sides) and %d tagged bonds are undecided (ez_state_<i> = 0)" % (rank, self.flipped, self.seen, self.left, self.undecided))


class Repair(Step):
    """repair_geometry=True: the conformers check_geometry calls invalid are moved into their distance bounds (validity.repair_geometry
    with the table bounds and its defaults; NOT MMFF); what follows describes the repaired conformers.  `pos_gen_<i>` holds them (a
    valid one is unchanged bit for bit), `repair_status_<i>` int8 [G] that function's status (0 valid as sampled, 1 repaired, 2 not
    within the iteration limit, 3 not finite), `repair_moved_<i>` float32 [G] its RMS move.  repair_planarity=True: the same step with
    planes (planarity.repair_planarity, one launch): bent conformers are flattened too; giving both switches equals giving this one."""
    switches = ("repair_geometry", "repair_planarity")
    repaired = stuck = seen = 0

    def apply(self, mol, pos, out, ctx):
        repair = planarity.repair_planarity if self.sw["repair_planarity"] else validity.repair_geometry     # (planes hold the bonds too)
        res = repair(dict(ctx.bonds, pos_gen=pos), device=ctx.device)
        status = res["status"].cpu().numpy()
        out["repair_status_%d" % mol["index"]] = status.astype(np.int8)
        out["repair_moved_%d" % mol["index"]] = res["moved"].cpu().numpy()
        self.seen += int(status.shape[0])
        self.repaired += int((status == 1).sum())
        self.stuck += int((status == 2).sum())
        return res["pos"]

    def summary(self, rank):
        if rank == 0 or self.seen:
            return ("rank %d: %d of %d conformers were repaired (%s); %d more were not within the iteration limit (repair_status_<i> = 2)"
                    % (rank, self.repaired, self.seen, "flattened and moved into their distance bounds" if self.sw["repair_planarity"] else
                       "moved into their distance bounds", self.stuck))


class CheckGeometry(Step):
    """check_geometry=True: every saved molecule also gets `valid_<i>` int8 [G], `bond_dev_<i>` float32 [G] and `clash_<i>` float32 [G]
    of agdiff_amd.validity.check_geometry with the table bounds.  `pos_gen_<i>` is left as it is; the invalid conformers leave the
    `mask`, so a prune leaves them out of its walk (`cluster_<i>` is -1 for them)."""
    switches = ("check_geometry",)
    checked = invalid = 0

    def apply(self, mol, pos, out, ctx):
        res = validity.check_geometry(dict(ctx.bonds, pos_gen=pos), device=ctx.device)
        out["valid_%d" % mol["index"]] = res["valid"].cpu().numpy().astype(np.int8)
        out["bond_dev_%d" % mol["index"]] = res["bond_dev"].cpu().numpy()
        out["clash_%d" % mol["index"]] = res["clash"].cpu().numpy()
        self.checked += int(res["valid"].shape[0])
        self.invalid += int((~res["valid"]).sum())
        ctx.mask = res["valid"] if ctx.mask is None else ctx.mask & res["valid"]

    def summary(self, rank):
        if rank == 0 or self.checked:
            return ("rank %d: %d of %d conformers are invalid (a bond length out of bounds or a steric clash) and are marked in valid_<i>"
                    % (rank, self.invalid, self.checked))


class CheckPlanarity(Step):
    """check_planarity=True: every saved molecule also gets `flat_<i>` int8 [G] and `flat_dev_<i>` float32 [G] of
    agdiff_amd.planarity.check_planarity with its defaults; `valid_<i>` does not change.  The bent conformers leave the `mask` too
    (`cluster_<i>` is -1 for them): the prune's mask is `flat`, and `valid & flat` with check_geometry."""
    switches = ("check_planarity",)
    judged = bent = 0

    def apply(self, mol, pos, out, ctx):
        res = planarity.check_planarity(dict(ctx.bonds, pos_gen=pos), device=ctx.device)
        out["flat_%d" % mol["index"]] = res["flat"].cpu().numpy().astype(np.int8)
        out["flat_dev_%d" % mol["index"]] = res["flat_dev"].cpu().numpy()
        self.judged += int(res["flat"].shape[0])
        self.bent += int((~res["flat"]).sum())
        ctx.mask = res["flat"] if ctx.mask is None else ctx.mask & res["flat"]

    def summary(self, rank):
        if rank == 0 or self.judged:
            return ("rank %d: %d of %d conformers are bent (an aromatic ring or a double bond out of plane) and are marked in flat_<i>"
                    % (rank, self.bent, self.judged))


class Prune(Step):
    """prune_rms=T (Angstrom, >= 0): every saved molecule also gets `kept_<i>` int32 [K] -- the conformers RDKit's pruneRmsThresh rule
    keeps at T, indices into `pos_gen_<i>` (which holds them all either way) -- and `cluster_<i>` int32 [G], each one's kept conformer
    (agdiff_amd.ensemble.prune_conformers), over the `mask` when a check ran.  prune_tfd=T (in [0, 1]) instead: the same by the TFD."""
    switches = ("prune_rms", "prune_tfd")
    thresholds = True

    def require(self, mols, shard, world):
        rms, tfd = self.sw["prune_rms"], self.sw["prune_tfd"]
        if rms is not None and not float(rms) >= 0.0:
            raise ValueError("prune_rms must be >= 0 (an RMSD threshold in Angstrom) or None")
        if tfd is not None and rms is not None:
            raise ValueError("prune_rms and prune_tfd are two rules for one pair of keys (kept_<i>, cluster_<i>): give one of them")
        if tfd is not None and not float(tfd) >= 0.0:
            raise ValueError("prune_tfd must be >= 0 (a torsion fingerprint deviation, in [0, 1]) or None")

    def apply(self, mol, pos, out, ctx):
        rms, tfd = self.sw["prune_rms"], self.sw["prune_tfd"]
        res = ensemble.prune_conformers(dict(ctx.bonds, pos_gen=pos), float(rms if tfd is None else tfd), align=False, device=ctx.device,
                                        metric="rmsd" if tfd is None else "tfd", valid=ctx.mask)
        out["kept_%d" % mol["index"]] = res["kept"].cpu().numpy()
        out["cluster_%d" % mol["index"]] = res["leader"].cpu().numpy()


class TrackedRmsd(Step):
    """track_rmsd=True: every saved molecule also gets `rmsd_traj_<i>` float32 [steps, G]: each conformer's heavy-atom RMSD to the
    molecule's `pos_target` (load_testset: `pos_target_<i>`) after every denoising step, computed while the run samples
    (agdiff_amd.trajectory), with or without save_traj; track_rmsd_mirror=True adds `rmsd_mirror_traj_<i>`, the mirror image's RMSD."""
    switches = ("track_rmsd", "track_rmsd_mirror")
    needs = ("pos_target",), "track_rmsd needs `pos_target_<i>` in the test set"
    sharded = on_device = False

    def sampler_keywords(self, packed):
        return {"curves": {"mirror": bool(self.sw["track_rmsd_mirror"])}}

    def apply(self, mol, pos, out, ctx):
        for key, name in (("rmsd", "rmsd_traj_%d"), ("rmsd_mirror", "rmsd_mirror_traj_%d")):
            if ctx.sampled["curves"].get(key) is not None:
                out[name % mol["index"]] = ctx.sampled["curves"][key][:, ctx.graphs].numpy().copy()


# THE order: core frame -> handedness -> E/Z -> repair -> checks -> prune, then the tracked curves (and, by run_job, `traj_<i>`).
STEPS = (CoreFrame, Handedness, DoubleBonds, Repair, CheckGeometry, CheckPlanarity, Prune, TrackedRmsd)


def enabled_steps(sw):
    """The steps of STEPS, in its order, that run_job's keywords `sw` turn on."""
    return [cls(sw) for cls in STEPS if any(sw[k] is not None if cls.thresholds else sw[k] for k in cls.switches)]


def run_chain(steps, mol, out, ctx):
    """The enabled steps over one saved molecule: `out` holds its `pos_gen_<i>` as sampled and gets every step's keys."""
    key, pos = "pos_gen_%d" % mol["index"], None
    for step in steps:
        if step.on_device and pos is None:
            pos = _lib.conformers(out[key], out[key].shape[1], ctx.device)
        moved = step.apply(mol, pos, out, ctx)
        pos = pos if moved is None else moved
    if pos is not None:
        out[key] = pos.cpu().numpy()
