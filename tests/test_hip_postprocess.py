"""driver.run_job's post-sampling chain (agdiff_amd/postprocess.py) on the GPU: a job with every switch on saves, byte for byte, what
the modules' own functions give when they are applied BY HAND, in the documented order -- core frame, handedness, E/Z, repair, the
two checks, prune -- to the conformers of a job without any of them.  The hand chain below is this test's own statement of that order.
"""
import numpy as np
import pytest

import ez_cases as EC
from test_hip_ezbonds import _gpu, _gpu_model
from agdiff_amd import ensemble, ezbonds, planarity, stereo, validity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _two_c14():
    """the 14-atom triene twice, 3 and 4 references: E/Z tags and a target from its skeleton, stereo tags by agdiff_amd.stereo (it has
    no tetrahedral centre: all zero), and a core (carbons 0 .. 3 and their hydrogens) on the second"""
    (mol, skeleton, _), (quads, target, _, _) = EC.molecule("c14"), EC.tables("c14")
    centre, cq = stereo.tetrahedral_centres(*mol)
    tags = np.zeros(14, dtype=np.int8)
    tags[centre] = stereo.parities_from_conformers(skeleton[None], cq)[0]
    mols = [dict(atom_type=mol[0], edge_index=mol[1], edge_type=mol[2], num_refs=3 + i, name="mol%d" % i, index=i, ez_quads=quads, ez=target,
                 stereo=tags, pos_target=skeleton.astype(np.float32)) for i in range(2)]
    mols[1]["core_pos"] = (skeleton + 2.0).astype(np.float32)
    mols[1]["core_mask"] = np.isin(np.arange(14), [0, 1, 2, 3, 8, 9, 10])
    return mols


def _by_hand(x, sampled, frozen):
    """the keys the chain saves for molecule x, from its conformers as sampled (already in the template's frame when a core was held)"""
    i, pos = x["index"], _gpu(sampled)
    bonds = dict(atom_type=x["atom_type"], edge_index=x["edge_index"], edge_type=x["edge_type"])
    out = {"hand_%d" % i: stereo.fix_handedness(dict(bonds, stereo=x["stereo"]), pos).cpu().numpy().astype(np.int8)}
    out["ez_state_%d" % i] = ezbonds.fix_double_bonds(dict(bonds, ez_quads=x["ez_quads"], ez=x["ez"]), pos, frozen=frozen).cpu().numpy()
    fixed = planarity.repair_planarity(dict(bonds, pos_gen=pos), device=DEV)
    pos = fixed["pos"]
    out["repair_status_%d" % i], out["repair_moved_%d" % i] = fixed["status"].cpu().numpy().astype(np.int8), fixed["moved"].cpu().numpy()
    geo, flat = validity.check_geometry(dict(bonds, pos_gen=pos), device=DEV), planarity.check_planarity(dict(bonds, pos_gen=pos), device=DEV)
    out["valid_%d" % i], out["flat_%d" % i] = geo["valid"].cpu().numpy().astype(np.int8), flat["flat"].cpu().numpy().astype(np.int8)
    out["bond_dev_%d" % i], out["clash_%d" % i], out["flat_dev_%d" % i] = (t.cpu().numpy() for t in (geo["bond_dev"], geo["clash"], flat["flat_dev"]))
    kept = ensemble.prune_conformers(dict(bonds, pos_gen=pos), 0.5, align=False, device=DEV, valid=geo["valid"] & flat["flat"])
    out["kept_%d" % i], out["cluster_%d" % i] = kept["kept"].cpu().numpy(), kept["leader"].cpu().numpy()
    out["pos_gen_%d" % i] = pos.cpu().numpy()
    return out


def test_every_switch_equals_the_modules_applied_by_hand_in_the_documented_order(tmp_path):
    from agdiff_amd import driver, qm9_model_config
    m = _gpu_model(qm9_model_config(num_diffusion_timesteps=10))
    mols, confs = _two_c14(), driver.num_confs("2x")
    kw = dict(n_steps=10, step_lr=1e-6, w_global=1.0, global_start_sigma=0.5, clip=1000.0)
    run = lambda name, **sw: driver.run_job(m, [dict(x) for x in mols], str(tmp_path / name), confs, 100000, kw, DEV, log=lambda *_: None,
                                            noise="counter", seed=5, **sw)
    recorded = dict(save_traj=True, track_rmsd_mirror=True)                     # (what the sampler records: no step touches it)
    plain, held, along = run("plain"), run("held", hold_core=True), run("along", hold_core=True, **recorded)
    full = run("full", hold_core=True, fix_handedness=True, fix_double_bonds=True, repair_geometry=True, repair_planarity=True,
               check_geometry=True, check_planarity=True, prune_rms=0.5, **recorded)
    assert sorted(plain) == ["name_0", "name_1", "pos_gen_0", "pos_gen_1"]
    # molecule 0 starts from the plain job; molecule 1 is sampled around its core, so it starts from the hold_core-only job, whose
    # conformers are already in the template's frame (the chain's first step)
    want = {"name_0": plain["name_0"], "name_1": plain["name_1"], "core_rmsd_1": held["core_rmsd_1"]}
    want.update(_by_hand(mols[0], plain["pos_gen_0"], None))
    want.update(_by_hand(mols[1], held["pos_gen_1"], mols[1]["core_mask"]))
    want.update({k: along[k] for k in along if k.split("_")[0] in ("traj", "rmsd")})
    assert sorted(full) == sorted(want) and len(want) == 2 * 16 + 1
    for k in sorted(want):
        assert full[k].dtype == want[k].dtype and full[k].shape == want[k].shape and full[k].tobytes() == want[k].tobytes(), k
    # the chain had something to do
    both = lambda key: np.concatenate([full["%s_0" % key].reshape(-1), full["%s_1" % key].reshape(-1)])
    assert (both("ez_state") < 0).any() and (both("repair_status") > 0).any() and np.isfinite(both("pos_gen")).all()
    assert plain["pos_gen_0"].tobytes() == held["pos_gen_0"].tobytes() == along["pos_gen_0"].tobytes()
