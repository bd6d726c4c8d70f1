"""Sampling driver: the counterpart of the reference's scripts/test.py:116-195 for this build.

scripts/test.py needs PyG `Data` pickles, rdkit and easydict and samples ONE molecule per call
(`repeat_data(data, 2 * num_refs)`, 100-1000 conformers, test.py:135-141), which leaves an MI355X
mostly idle.  This driver keeps its contract -- per molecule `num_confs(num_refs)` conformers,
5000-step Langevin sampling with the same arguments, at most one retry with `clip_local=20` when a NaN
appears in a molecule (test.py:143-181; only that molecule is re-sampled), results saved after every batch, `--resume` skips finished molecules --
but reads/writes PyG-free `.npz` files and packs many molecules into each batch.

Input .npz (see `save_testset`): for molecule i: `atom_type_i` [n], `edge_index_i` [2, e] and `edge_type_i` [e]
(bond graph; already extended to order 3 like `AddHigherOrderEdges` does unless --extend-order),
`num_refs_i` scalar, `name_i` string.  Output: `samples_<first>_<last>.npz` per batch (named by the molecule
indices it holds) with `pos_gen_<i>` [num_samples, n, 3] (+ `traj_<i>` [steps, num_samples, n, 3] with
--save-traj; + `kept_<i>` [K] and `cluster_<i>` [num_samples] with --prune-rms T: the conformers that differ by more than T; + `hand_<i>` [num_samples] with --fix-handedness, which needs
`stereo_<i>` in the test set; + `ez_state_<i>` [num_samples, D] with --fix-double-bonds, which needs `ez_quads_<i>` and `ez_<i>` in the test set; + `valid_<i>`, `bond_dev_<i>` and `clash_<i>` [num_samples] with --check-geometry; + `rmsd_traj_<i>` [steps, num_samples] with --track-rmsd, which needs `pos_target_<i>` in the test set: every
conformer's heavy-atom RMSD to that target after every step, + `rmsd_mirror_traj_<i>` with --track-rmsd-mirror; + `core_rmsd_<i>`
[num_samples] with --hold-core for the molecules with `core_pos_<i>` / `core_mask_<i>` in the test set) and the merged
`samples_all.npz`, written by rank 0 after a barrier.

`--noise counter` draws every conformer's pos_init and noise from the counter-based generator under `--seed` and the conformer's
stream id (`stream_id`): the same numbers whatever --max-atoms, the packing, a --resume or the number of ranks.

    python -m agdiff_amd.driver --ckpt ckpt.pt --testset test.npz --out out_dir [--n-steps 5000]
    torchrun --nproc-per-node 8 -m agdiff_amd.driver ...      (each packed batch is sharded over the ranks by graph
                                                               ranges; one RCCL all-gather of positions per step)
"""
import argparse
import glob
import os

import numpy as np


def num_confs(spec):
    """scripts/test.py:15-24."""
    if str(spec).endswith("x"):
        return lambda x: x * int(str(spec)[:-1])
    if int(spec) > 0:
        return lambda x: int(spec)
    raise ValueError(spec)


def save_testset(path, molecules):
    """molecules: list of dicts with atom_type, edge_index, edge_type, num_refs, name; optionally stereo (int8 [n]: the target
    parity at the stereocentres, 0 elsewhere -- agdiff_amd.stereo), saved as `stereo_<i>` when present, ez_quads (int32 [D, 4]) with ez
    (int8 [D]: the stereogenic double bonds and their target parity -- agdiff_amd.ezbonds), saved as `ez_quads_<i>` and `ez_<i>`, and pos_target (float32
    [n, 3]: the structure --track-rmsd follows every conformer's RMSD to -- agdiff_amd.trajectory), saved as `pos_target_<i>`, and
    core_pos (float32 [n, 3]) with core_mask ([n], non-zero = the atom belongs to the core: the template --hold-core keeps those
    atoms on -- agdiff_amd.core; rows of core_pos outside the mask are not read), saved as `core_pos_<i>` and `core_mask_<i>` (uint8)."""
    out = {"count": np.int64(len(molecules))}
    for i, m in enumerate(molecules):
        out["atom_type_%d" % i] = np.asarray(m["atom_type"], dtype=np.int64)
        out["edge_index_%d" % i] = np.asarray(m["edge_index"], dtype=np.int64)
        out["edge_type_%d" % i] = np.asarray(m["edge_type"], dtype=np.int64)
        out["num_refs_%d" % i] = np.int64(m.get("num_refs", 1))
        out["name_%d" % i] = np.str_(m.get("name", "mol%d" % i))
        if m.get("stereo") is not None:
            out["stereo_%d" % i] = np.asarray(m["stereo"], dtype=np.int8)
        if m.get("ez_quads") is not None and m.get("ez") is not None:
            out["ez_quads_%d" % i] = np.asarray(m["ez_quads"], dtype=np.int32).reshape(-1, 4)
            out["ez_%d" % i] = np.asarray(m["ez"], dtype=np.int8).reshape(-1)
        if m.get("pos_target") is not None:
            n = np.asarray(m["atom_type"]).reshape(-1).shape[0]
            target = np.asarray(m["pos_target"], dtype=np.float32)
            if target.shape != (n, 3):
                raise ValueError("pos_target of molecule %d has shape %s, expected (%d, 3)" % (i, target.shape, n))
            out["pos_target_%d" % i] = target
        if m.get("core_pos") is not None or m.get("core_mask") is not None:
            n = np.asarray(m["atom_type"]).reshape(-1).shape[0]
            if m.get("core_pos") is None or m.get("core_mask") is None:
                raise ValueError("molecule %d: core_pos and core_mask come together" % i)
            core, mask = np.asarray(m["core_pos"], dtype=np.float32), np.asarray(m["core_mask"])
            if core.shape != (n, 3) or mask.shape != (n,):
                raise ValueError("core_pos / core_mask of molecule %d have shapes %s / %s, expected (%d, 3) / (%d,)"
                                 % (i, core.shape, mask.shape, n, n))
            out["core_pos_%d" % i] = core
            out["core_mask_%d" % i] = (mask != 0).astype(np.uint8)
    np.savez_compressed(path, **out)


def load_testset(path):
    z = np.load(path, allow_pickle=False)
    mols = []
    for i in range(int(z["count"])):
        mols.append(dict(atom_type=z["atom_type_%d" % i], edge_index=z["edge_index_%d" % i],
                         edge_type=z["edge_type_%d" % i], num_refs=int(z["num_refs_%d" % i]),
                         name=str(z["name_%d" % i]), index=i))
        if "stereo_%d" % i in z.files:
            mols[-1]["stereo"] = z["stereo_%d" % i]
        if "ez_quads_%d" % i in z.files and "ez_%d" % i in z.files:
            mols[-1]["ez_quads"], mols[-1]["ez"] = z["ez_quads_%d" % i], z["ez_%d" % i]
        if "pos_target_%d" % i in z.files:
            mols[-1]["pos_target"] = z["pos_target_%d" % i]
        if "core_pos_%d" % i in z.files and "core_mask_%d" % i in z.files:
            mols[-1]["core_pos"], mols[-1]["core_mask"] = z["core_pos_%d" % i], z["core_mask_%d" % i]
    return mols


def stream_id(molecule_index, conformer_index, attempt=0):
    """The 64-bit name of one conformer's random stream (--noise counter; include/agdiff_hip.h: agdiff_counter_noise):
    molecule_index << 32 | attempt << 24 | conformer_index.  molecule_index: the molecule's `index` field, which also names its
    output (pos_gen_<index>); conformer_index: the position within the molecule's repeat, below 2^24; attempt: 0 for the first
    sampling pass, + 1 for every NaN retry, below 256.  Takes ints or numpy arrays."""
    m, c, a = (np.asarray(x, dtype=np.int64) for x in (molecule_index, conformer_index, attempt))
    if np.any(m < 0) or np.any(m >= 1 << 31):
        raise ValueError("molecule index outside [0, 2^31)")
    if np.any(c < 0) or np.any(c >= 1 << 24):
        raise ValueError("conformer index outside [0, 2^24)")
    if np.any(a < 0) or np.any(a >= 256):
        raise ValueError("attempt outside [0, 256)")
    out = (m << 32) | (a << 24) | c
    return int(out) if out.ndim == 0 else out


def split_stream_id(sid):
    """(molecule_index, conformer_index, attempt) of a stream id (ints or numpy arrays)."""
    s = np.asarray(sid, dtype=np.int64)
    parts = (s >> 32, s & 0xFFFFFF, (s >> 24) & 0xFF)
    return tuple(int(p) for p in parts) if s.ndim == 0 else parts


def with_attempt(stream_ids, attempt):
    """The same conformers' ids with the attempt field set to `attempt`."""
    m, c, _ = split_stream_id(np.asarray(stream_ids, dtype=np.int64))
    return stream_id(m, c, attempt)


def sharded_capacity(max_atoms, world):
    """Atoms of one global batch that `world` ranks share by contiguous graph ranges (dist.shard_graphs balances EDGES, so the
    ranks' atom counts differ by a few per cent: profiles/r05_shard_balance.json): 3 % below max_atoms x world, so that no rank's
    share crosses max_atoms -- 196,608 by default = three full rounds of the node kernels' workgroups; a rank 2 % above it ran a
    fourth round and 4 % longer than its peers."""
    return max_atoms * world if world <= 1 else int(max_atoms * world * 0.97)


def plan_batches(mols, confs_of, max_atoms):
    """First-fit decreasing: molecules sorted by their atom count x conformers (largest first), each put into the first
    batch it still fits into (a molecule larger than `max_atoms` gets a batch of its own).  Packing in input order
    leaves many half-empty batches when a few molecules have hundreds of conformers (GEOM test molecules carry 50-500
    references, utils/datasets.py:720-721), and a half-empty batch costs nearly a full one per denoising step.
    Results are keyed by molecule index, so the order inside the batches does not matter; every batch keeps its
    molecules in ascending index order.  Molecules of more than AGDIFF_MAX_ATOMS_PER_GRAPH atoms share batches only with
    each other: one of them sends its whole batch down the large path (mask-free graph build, unfused sampler front), which
    Drugs-sized molecules have no reason to take."""
    from . import _lib
    need = [int(m["atom_type"].shape[0]) * confs_of(m["num_refs"]) for m in mols]
    large = [int(m["atom_type"].shape[0]) > _lib.MAX_ATOMS_PER_GRAPH for m in mols]
    order = sorted(range(len(mols)), key=lambda k: (-need[k], k))
    bins, room = [], []
    for k in order:
        for b in range(len(bins)):
            if need[k] <= room[b] and large[bins[b][0]] == large[k]:
                bins[b].append(k)
                room[b] -= need[k]
                break
        else:
            bins.append([k])
            room.append(max_atoms - need[k])
    batches = [[mols[k] for k in sorted(b)] for b in bins]
    batches.sort(key=lambda bm: bm[0].get("index", 0) if isinstance(bm[0], dict) else 0)
    return batches


def pack_batch(mols, confs_of):
    """repeat_data (utils/misc.py:88-90) for every molecule of the batch, concatenated.  When every molecule carries its `index`
    (load_testset), `stream_ids` [num_graphs] names each graph's random stream (stream_id, attempt 0): the ids travel with the
    graphs through subset_batch and dist.shard_of.  When every molecule carries a `pos_target` [n, 3], `pos_target` [N, 3] holds it
    once per conformer (float32): what the sampler tracks every graph's RMSD to (--track-rmsd).  When ANY molecule carries a core
    (`core_pos` [n, 3] + `core_mask` [n]), `core_pos` [N, 3] float32 and `core_select` [N] uint8 hold them once per conformer, zeros
    for the molecules without one: what the sampler holds (--hold-core)."""
    from .synth import repeat_molecule
    ats, rs, cs, ts, bs, spans, ids, targets, cores, masks = [], [], [], [], [], [], [], [], [], []
    node_off, g_off = 0, 0
    for m in mols:
        g = confs_of(m["num_refs"])
        n = int(m["atom_type"].shape[0])
        a, r, c, t, b = repeat_molecule(m["atom_type"], m["edge_index"][0], m["edge_index"][1], m["edge_type"], g,
                                        node_off, g_off)
        ats.append(a); rs.append(r); cs.append(c); ts.append(t); bs.append(b)
        spans.append((node_off, n, g))
        if isinstance(m, dict) and m.get("index") is not None:
            ids.append(stream_id(int(m["index"]), np.arange(g, dtype=np.int64)))
        if isinstance(m, dict) and m.get("pos_target") is not None:
            targets.append(np.tile(np.asarray(m["pos_target"], dtype=np.float32).reshape(n, 3), (g, 1)))
        if isinstance(m, dict) and m.get("core_pos") is not None and m.get("core_mask") is not None:
            cores.append(np.tile(np.asarray(m["core_pos"], dtype=np.float32).reshape(n, 3), (g, 1)))
            masks.append(np.tile((np.asarray(m["core_mask"]).reshape(n) != 0).astype(np.uint8), g))
        else:
            cores.append(None)
            masks.append(np.zeros(n * g, dtype=np.uint8))
        node_off += n * g
        g_off += g
    out = dict(atom_type=np.concatenate(ats), bond_index=np.stack([np.concatenate(rs), np.concatenate(cs)]),
               bond_type=np.concatenate(ts), batch=np.concatenate(bs), num_graphs=g_off, spans=spans)
    if len(ids) == len(mols):
        out["stream_ids"] = np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64)
    if mols and len(targets) == len(mols):
        out["pos_target"] = np.concatenate(targets)
    if any(c is not None for c in cores):
        out["core_pos"] = np.concatenate([np.zeros((k.shape[0], 3), dtype=np.float32) if c is None else c for c, k in zip(cores, masks)])
        out["core_select"] = np.concatenate(masks)
    return out


def prepare_batch(model, bmols, confs_of, rank=0, world=1, build=None):
    """(packed batch, its BatchTopology on the host or None) -- for world > 1 the topology of THIS rank's graph range of the
    batch (dist.shard_of), as sample_batch_sharded samples it.  Host work only (no GPU call): run_job calls it for the next
    batch from a background thread.  `build`: by default the model's prepare_topology; None without one (test stubs) or without graphs."""
    packed = pack_batch(bmols, confs_of)
    build = build or getattr(model, "prepare_topology", None)
    part = packed
    if world > 1 and build is not None:
        from .dist import shard_of
        part = shard_of(packed, rank, world)[0]
    if build is None or part is None:
        return packed, None
    try:
        return packed, build(part["atom_type"], part["bond_index"], part["bond_type"], part["batch"], num_graphs=part["num_graphs"],
                             extend_order=False, device="cpu")
    except Exception:
        # (a batch the topology refuses -- e.g. a molecule beyond the atom limit: the sampler builds it again and raises THERE, where
        # sample_batch_sharded keeps a failing rank's collectives in step with the others)
        return packed, None


def _prepare_in_worker(bmols, confs, rank, world, topo_opts):
    """prepare_batch in a worker PROCESS (run_job): the same packed batch and BatchTopology, built without the sampling
    process's interpreter lock -- a background THREAD hid 0.3 s of a batch's 1-4 s of numpy, because every Python-level step of
    the build waits for the launch loop's lock and vice versa.  Host work only: nothing here touches a GPU.  `confs`: conformers
    per molecule of the batch (the callable of scripts/test.py:15-24 does not pickle)."""
    import functools
    from .topology import BatchTopology
    it = iter(confs)
    return prepare_batch(None, bmols, lambda _num_refs: next(it), rank, world, build=functools.partial(BatchTopology, **topo_opts))


def sample_batch(model, packed, device, sampler_kwargs, save_traj=False, max_retry=2, log=print, pos_init=None,
                 noise=None, topology=None, counter_seed=None, *, curves=None, core=None):
    """test.py:143-181 for every molecule of a packed batch: a molecule in which a NaN appeared is sampled again
    (fresh pos_init) with clip_local=20, at most `max_retry` attempts in all, and dropped after that; the molecules
    packed with it keep their first result -- graphs are independent on the whole path, and the update kernel flags
    NaNs per graph (agdiff_ws_t.nan_flag).  Returns (pos [N,3] cpu, traj [steps,N,3] cpu or None, ok [num molecules]
    bool); rows of failed molecules are NaN.  `pos_init` [N,3] / `noise` [steps,N,3] replace the first attempt's
    random draws (parity tests).  `topology`: the batch's BatchTopology prepared ahead (prepare_batch; first attempt only).
    Models without begin_sampling (test stubs) take the reference's whole-batch retry.
    `counter_seed` (--noise counter): pos_init and the steps' noise come from the counter-based generator with this key and
    the batch's `stream_ids` instead of torch's generator -- a conformer's draws then depend on (seed, molecule index,
    conformer, attempt) alone.  A NaN retry draws with attempt + 1; a split-bf16 re-run of a range-only fault keeps its attempt
    (the same draws in wider arithmetic).
    `curves`: a dict to fill with the tracked RMSD curves (epsnet.LangevinRun: rmsd_target = the batch's `pos_target`, heavy atoms):
    curves["rmsd"] float32 [steps, num_graphs] and, when it came in with curves["mirror"] true, curves["rmsd_mirror"].
    `core`: a dict {"weight": w, "start_sigma": s}: the batch's `core_pos` / `core_select` are held while sampling (epsnet.LangevinRun;
    agdiff_amd/core.py) in every pass whose molecules include one with a core; it comes back with core["dev"] float32 [num_graphs],
    the runs' `core_dev`.  Both hold a molecule's values from the pass that succeeded, NaN for dropped molecules (and graphs without a core)."""
    import torch
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    n_mol = len(packed["spans"])
    check_counter(model, packed, counter_seed)
    if curves is not None:
        if packed.get("pos_target") is None:
            raise ValueError("tracking the RMSD needs `pos_target` in the packed batch (every molecule with its pos_target)")
        if not hasattr(model, "begin_sampling"):
            raise ValueError("tracking the RMSD needs a model with begin_sampling")
    if core is not None:
        if packed.get("core_pos") is None or packed.get("core_select") is None:
            raise ValueError("holding a core needs `core_pos` and `core_select` in the packed batch (a molecule with its core_pos / core_mask)")
        if not hasattr(model, "begin_sampling"):
            raise ValueError("holding a core needs a model with begin_sampling")
        core["dev"] = torch.full((int(packed["num_graphs"]),), float("nan"))
    if not hasattr(model, "begin_sampling"):
        at, bi, bt, ba = T(packed["atom_type"]), T(packed["bond_index"]), T(packed["bond_type"]), T(packed["batch"])
        clip_local = None
        for _ in range(max_retry):
            try:
                p0 = torch.randn(at.shape[0], 3).to(device) if pos_init is None else pos_init.to(device)
                pos_gen, traj = model.langevin_dynamics_sample_diffusion(
                    atom_type=at, pos_init=p0, bond_index=bi, bond_type=bt, batch=ba,
                    num_graphs=packed["num_graphs"], extend_order=False, clip_local=clip_local,
                    save_traj=save_traj, **sampler_kwargs)
                return pos_gen.cpu(), (torch.stack(traj) if save_traj else None), np.ones(n_mol, dtype=bool)
            except FloatingPointError:
                clip_local = 20
                log("Retrying with local clipping.")
        return None, None, np.zeros(n_mol, dtype=bool)

    def run_pass(sub, todo, clip_local, wide, tries, first):
        nonlocal topology
        extra = {"topology": topology} if (topology is not None and sub is packed) else {}
        topology = None                        # (moved to the device and owned by the run now)
        if curves is not None:
            extra.update(rmsd_target=sub["pos_target"], rmsd_mirror=bool(curves.get("mirror")))
        held = core is not None and bool(np.asarray(sub["core_select"]).any())      # (a retry of molecules without a core: as ever)
        if held:
            extra.update(core_pos=sub["core_pos"], core_select=sub["core_select"], core_weight=core.get("weight", 1.0),
                         core_start_sigma=core.get("start_sigma", float("inf")))
        run, pos, traj = run_part(model, sub, device, sampler_kwargs, counter_seed, tries, wide, pos_init if first else None,
                                  clip_local=clip_local, save_traj=save_traj, noise=(noise if first else None), **extra)
        per_graph = dict(rmsd=run.rmsd_curve, rmsd_mirror=run.rmsd_curve_mirror) if curves is not None else {}
        if held:
            per_graph["core_dev"] = run.core_dev
        return pos.cpu(), (torch.stack(traj) if save_traj else None), run.nan_graphs().numpy(), getattr(run, "range_graphs", ()), per_graph

    ok, got = sample_passes(packed, run_pass, max_retry, log)
    if curves is not None:
        curves.update({k: got[k] for k in ("rmsd", "rmsd_mirror") if k in got})
    if "core_dev" in got:
        core["dev"] = got["core_dev"]
    return got["pos"], got.get("traj"), ok


# what sample_batch / sample_batch_sharded met since the process started (run_job logs it with the job's summary)
SAMPLE_STATS = {"range_trips": 0, "bf16x3_retries": 0, "dropped": 0}


def sample_passes(packed, run_pass, max_retry, log):
    """The retry schedule of sample_batch and dist.sample_batch_sharded: (ok [num molecules] bool, results).  The queue holds the
    passes still to run: (molecule slots of `packed`, clip_local, split-bf16?, attempts counted so far).  A molecule in which a NaN
    appeared is sampled again with clip_local=20 and that pass counts against max_retry (test.py:143-181).  One whose ONLY fault was
    leaving the split-fp16 range (epsnet.check_nan) has not failed by the reference's lights: it is sampled again in split-bf16
    (fp32's exponent range; no range watch there, so nothing is range-only in a `wide` pass), settings unchanged, and not counted.
    run_pass(sub, todo, clip_local, wide, tries, first) samples `sub` (`packed` or its subset of the slots `todo`) and returns, on the host,
    (pos [rows, 3], traj [steps, rows, 3] or None, bad_graph bool [graphs], the graphs that left the range, {name: tensor [..., graphs] or
    None}).  results: "pos", "traj" and those names over the rows / graphs of `packed`, NaN where no pass succeeded."""
    import torch
    spans = packed["spans"]
    n_mol = len(spans)
    gfirst = np.concatenate([[0], np.cumsum([g for (_, _, g) in spans])])
    size = {-2: packed["atom_type"].shape[0], -1: int(gfirst[-1])}       # (rows [..., N, 3] are counted by dimension -2, graphs [..., G] by -1)
    ok, results = np.zeros(n_mol, dtype=bool), {}
    passes = [(list(range(n_mol)), None, False, 0)]
    first = True
    while passes:
        todo, clip_local, wide, tries = passes.pop(0)
        sub = packed if len(todo) == n_mol else subset_batch(packed, todo)
        pos, traj, bad_graph, out_of_range, per_graph = run_pass(sub, todo, clip_local, wide, tries, first)
        first = False
        parts = [(k, t, -2) for k, t in (("pos", pos), ("traj", traj)) if t is not None] + [(k, t, -1) for k, t in per_graph.items() if t is not None]
        for name, t, dim in parts:
            if name not in results:
                shape = list(t.shape)
                shape[dim] = size[dim]
                results[name] = torch.full(shape, float("nan"))
        in_range_set = set(int(g) for g in out_of_range)
        nan_failed, range_failed, g_off = [], [], 0
        for slot, (off_s, n, g) in zip(todo, sub["spans"]):
            bad = [k for k in range(g_off, g_off + g) if bad_graph[k]]
            if bad:
                (range_failed if (not wide and all(k in in_range_set for k in bad)) else nan_failed).append(slot)
            else:
                ok[slot] = True
                off = spans[slot][0]
                for name, t, dim in parts:           # one scatter by molecule slot
                    if dim == -2:
                        results[name][..., off:off + n * g, :] = t[..., off_s:off_s + n * g, :]
                    else:
                        results[name][..., gfirst[slot]:gfirst[slot] + g] = t[..., g_off:g_off + g]
            g_off += g
        SAMPLE_STATS["range_trips"] += len(in_range_set)
        if range_failed:
            SAMPLE_STATS["bf16x3_retries"] += 1
            log("%d conformers left the split-fp16 range: sampling their molecules (%d of %d) again in split-bf16."
                % (len(in_range_set), len(range_failed), len(sub["spans"])))
            passes.append((range_failed, clip_local, True, tries))
        if nan_failed:
            if tries + 1 < max_retry:
                log("NaN in %d of %d molecules: retrying those with local clipping." % (len(nan_failed), len(sub["spans"])))
                passes.append((nan_failed, 20, wide, tries + 1))
            else:
                SAMPLE_STATS["dropped"] += len(nan_failed)
    return ok, results


def check_counter(model, packed, counter_seed):
    """--noise counter needs the batch's stream ids (pack_batch: every molecule with its `index`) and a model that draws from
    the counter-based generator."""
    if counter_seed is None:
        return
    if packed.get("stream_ids") is None:
        raise ValueError("counter noise: the packed batch carries no stream_ids (every molecule needs its 'index')")
    if not (hasattr(model, "begin_sampling") and hasattr(model, "counter_normals")):
        raise ValueError("counter noise: the model has no counter-based generator (begin_sampling / counter_normals)")


def run_part(model, part, device, sampler_kwargs, counter_seed, attempt, wide, pos_init=None, hook=None, **kw):
    """One sampling run over `part` (a packed batch, a subset or a rank's range of one) in sampling pass `attempt`: (run, pos, traj).
    pos_init as given; else, with a `counter_seed`, from the counter-based generator and the part's stream ids with that attempt, like
    the steps' noise; else from torch's generator.  `wide`: the model in split-bf16 for both branches (fp32's exponent range) for
    the duration of the run.  hook(run): the run's on_step.  `kw` goes to begin_sampling."""
    import contextlib
    import torch
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    counter = {}
    if counter_seed is not None:
        counter = dict(noise_mode="counter", noise_seed=int(counter_seed), stream_ids=with_attempt(part["stream_ids"], attempt))
    with model.arithmetic("bf16x3", "bf16x3") if (wide and hasattr(model, "arithmetic")) else contextlib.nullcontext():
        if pos_init is not None:
            p0 = pos_init.to(device)
        elif counter:
            p0 = model.counter_normals(part["batch"], counter["stream_ids"], counter_seed, [-1])[0]
        else:
            p0 = torch.randn(part["atom_type"].shape[0], 3).to(device)
        run = model.begin_sampling(T(part["atom_type"]), p0, T(part["bond_index"]), T(part["bond_type"]), T(part["batch"]), part["num_graphs"],
                                   False, raise_on_nan=False, **kw, **counter, **sampler_kwargs)
        if hook is not None:
            run.on_step = hook(run)
        run.advance(run.remaining())
        return (run,) + tuple(run.finish())


def subset_batch(packed, slots):
    """The packed batch restricted to the molecule slots `slots` (re-based node / graph ids)."""
    keep_nodes, spans, batch, keep_graphs = [], [], [], []
    node_off = g_off = 0
    shift = np.zeros(packed["atom_type"].shape[0], dtype=np.int64)
    gfirst = np.concatenate([[0], np.cumsum([g for (_, _, g) in packed["spans"]])])
    for s in slots:
        off, n, g = packed["spans"][s]
        idx = np.arange(off, off + n * g)
        keep_nodes.append(idx)
        keep_graphs.append(np.arange(gfirst[s], gfirst[s] + g))
        shift[idx] = node_off - off
        batch.append(packed["batch"][idx] - gfirst[s] + g_off)
        spans.append((node_off, n, g))
        node_off += n * g
        g_off += g
    keep = np.concatenate(keep_nodes)
    mask = np.zeros(packed["atom_type"].shape[0], dtype=bool)
    mask[keep] = True
    bi = packed["bond_index"]
    esel = mask[bi[0]]
    sub = dict(atom_type=packed["atom_type"][keep], bond_index=bi[:, esel] + shift[bi[0][esel]][None, :],
               bond_type=packed["bond_type"][esel], batch=np.concatenate(batch), num_graphs=g_off, spans=spans)
    if packed.get("stream_ids") is not None:
        sub["stream_ids"] = np.asarray(packed["stream_ids"])[np.concatenate(keep_graphs).astype(np.int64)]
    if packed.get("pos_target") is not None:
        sub["pos_target"] = np.asarray(packed["pos_target"])[keep]
    if packed.get("core_pos") is not None:
        sub["core_pos"], sub["core_select"] = np.asarray(packed["core_pos"])[keep], np.asarray(packed["core_select"])[keep]
    return sub


def _done_indices(out_dir):
    done = set()
    for f in glob.glob(os.path.join(out_dir, "samples_[0-9]*.npz")):
        done.update(int(k.split("_")[-1]) for k in np.load(f).files if k.startswith("pos_gen_"))
    return done


def _batch_path(out_dir, bmols):
    """Output file of one batch, named by what it holds (smallest / largest molecule index of the batch), never by a
    batch counter: a --resume run plans its batches over the molecules still missing, and a counter restarting at 0
    would overwrite files of the earlier run that hold other, finished molecules."""
    base = os.path.join(out_dir, "samples_%05d_%05d" % (min(m["index"] for m in bmols), max(m["index"] for m in bmols)))
    path, k = base + ".npz", 0
    while os.path.exists(path):
        k += 1
        path = "%s_r%d.npz" % (base, k)
    return path


def _save_npz_atomic(path, arrays):
    # the temporary's name must not match the `samples_[0-9]*.npz` globs of _done_indices / merge_outputs: a run killed
    # mid-write leaves it behind, and np.load of a truncated archive would end the next --resume
    tmp = os.path.join(os.path.dirname(path), "." + os.path.basename(path) + ".tmp")
    with open(tmp, "wb") as f:
        np.savez_compressed(f, **arrays)
    os.replace(tmp, path)


def merge_outputs(out_dir):
    merged = {}
    for f in sorted(glob.glob(os.path.join(out_dir, "samples_[0-9]*.npz"))):
        z = np.load(f)
        merged.update({k: z[k] for k in z.files})
    _save_npz_atomic(os.path.join(out_dir, "samples_all.npz"), merged)
    return merged


def run_job(model, mols, out_dir, confs_of, max_atoms, sampler_kwargs, device, save_traj=False, resume=False,
            rank=0, world=1, shard=False, log=print, noise="default", seed=2021, prune_rms=None,
            fix_handedness=False, prune_tfd=None, track_rmsd=False, track_rmsd_mirror=False, repair_geometry=False,
            check_planarity=False, repair_planarity=False, hold_core=False, core_weight=1.0, core_start_sigma=float("inf"),
            fix_double_bonds=False, check_geometry=False):
    """Plan, sample and save (the loop of scripts/test.py:128-181 over packed batches).  Returns the merged result
    dict on rank 0 (None elsewhere).  noise="counter": every conformer's pos_init and noise are drawn from the counter-based
    generator under the key `seed` and the conformer's stream id (stream_id: molecule index, conformer, attempt) -- the same
    draws whatever `max_atoms`, the plan, a resume or the number of ranks put beside it; "default": torch's generator.
    Every other switch but save_traj (`traj_<i>`) turns on one step of agdiff_amd.postprocess.STEPS, the order in which they run over
    each saved molecule: CoreFrame (hold_core, core_weight, core_start_sigma), Handedness, DoubleBonds, Repair, CheckGeometry,
    CheckPlanarity, Prune, TrackedRmsd; each class names its switches, what it needs of the test set and the keys it saves."""
    keywords = dict(locals())                  # (first: the arguments and nothing else; each step reads its own switches)
    import contextlib
    from . import postprocess
    if noise not in ("default", "counter"):
        raise ValueError("noise must be 'default' or 'counter'")
    steps = postprocess.enabled_steps(keywords)
    for step in steps:
        step.require(mols, shard, world)
    counter_seed = int(seed) if noise == "counter" else None
    import torch.distributed as dist
    os.makedirs(out_dir, exist_ok=True)
    done = set()
    if resume:
        # every rank must plan the same batches: rank 0 lists the finished molecules, the others take its list
        box = [sorted(_done_indices(out_dir)) if rank == 0 else None]
        if world > 1:
            dist.broadcast_object_list(box, src=0)
        done = set(box[0])
    mols = [m for m in mols if m["index"] not in done]
    batches = plan_batches(mols, confs_of, sharded_capacity(max_atoms, world) if shard else max_atoms)
    mine = [bidx for bidx in range(len(batches)) if shard or bidx % world == rank]
    with contextlib.closing(_prepared_batches(model, batches, mine, confs_of, rank if shard else 0, world if shard else 1, log)) as prepared:
        for bidx, bmols, packed, topology in prepared:
            extras = {}                        # (what the steps ask of the sampler; it comes back filled in, for their apply)
            if shard:
                from .dist import sample_batch_sharded
                pos, traj, ok = sample_batch_sharded(model, packed, device, sampler_kwargs, save_traj=save_traj, log=log,
                                                     topology=topology, counter_seed=counter_seed)
                if rank != 0:
                    continue
            else:
                for step in steps:
                    extras.update(step.sampler_keywords(packed))
                pos, traj, ok = sample_batch(model, packed, device, sampler_kwargs, save_traj=save_traj, log=log, topology=topology,
                                             counter_seed=counter_seed, **extras)
            if not ok.any():
                log("batch %d: every molecule failed twice (NaN); skipped: %s" % (bidx, [m["name"] for m in bmols]))
                continue
            out = {}
            g_first = 0
            for m, (off, n, g), good in zip(bmols, packed["spans"], ok):
                g_first += g
                if not good:
                    log("molecule %s failed twice (NaN); skipped" % m["name"])
                    continue
                out["pos_gen_%d" % m["index"]] = pos[off:off + n * g].numpy().reshape(g, n, 3)
                out["name_%d" % m["index"]] = np.str_(m["name"])
                ctx = postprocess.MolContext(dict(atom_type=m["atom_type"], edge_index=m["edge_index"], edge_type=m["edge_type"]), device,
                                             slice(g_first - g, g_first), extras)
                postprocess.run_chain(steps, m, out, ctx)
                if traj is not None:
                    out["traj_%d" % m["index"]] = traj[:, off:off + n * g].numpy().reshape(traj.shape[0], g, n, 3)
            _save_npz_atomic(_batch_path(out_dir, bmols), out)
            log("rank %d: batch %d/%d (%d of %d molecules, %d conformers) saved" % (rank, bidx + 1, len(batches),
                                                                                   int(ok.sum()), len(bmols), packed["num_graphs"]))
    for line in filter(None, (step.summary(rank) for step in steps)):       # (None on a rank that wrote no file)
        log(line)
    if world > 1:
        dist.barrier()                       # every rank's batch files are on disk
    if SAMPLE_STATS["range_trips"]:
        log("rank %d: %d conformers left the split-fp16 range; their molecules were sampled again in split-bf16 (%d extra passes)"
            % (rank, SAMPLE_STATS["range_trips"], SAMPLE_STATS["bf16x3_retries"]))
    if SAMPLE_STATS["dropped"]:
        log("rank %d: %d molecules were dropped (a NaN in every attempt)" % (rank, SAMPLE_STATS["dropped"]))
    return merge_outputs(out_dir) if rank == 0 else None


def _prepared_batches(model, batches, mine, confs_of, rank, world, log):
    """Yields (bidx, bmols, packed, topology) for the batches `mine`, each prepared (prepare_batch for `rank` of `world`) while the
    GPU samples the one before it: in a background thread (the sampling loop spends its time inside library calls, which release
    the interpreter lock).  Four 196 k-atom batches x 600 steps on an MI355X (tools/job_wall.py, profiles/r06_job_wall.json):
    sampling + saving alone 10.13 s, preparation inline 11.3 s, thread 10.8 s, worker process 11.8 s.
    AGDIFF_PREPARE=process: a worker PROCESS (agdiff_amd/prep_worker.py; host work only) -- it shares nothing with the launch loop,
    but its reply (~100 MB of index arrays per batch) comes back through a pipe and a pickle; for hosts where the numpy build takes
    seconds per batch.  =inline: on the main thread, when the batch's turn comes (measurements, debugging)."""
    from concurrent.futures import ThreadPoolExecutor
    prep = lambda bidx: prepare_batch(model, batches[bidx], confs_of, rank, world)
    how = os.environ.get("AGDIFF_PREPARE", "inline" if os.environ.get("AGDIFF_PREPARE_INLINE", "0") not in ("", "0") else "thread")
    worker, pool = None, None
    if how == "process" and hasattr(model, "prepare_topology") and hasattr(model, "config") and len(mine) > 1:
        try:
            from .prep_worker import Client
            worker = Client()                         # (a child process: boots while the first batch is prepared here)
        except Exception as e:                        # (no worker: the thread)
            log("run_job: no worker process for the batch preparation (%s: %s); using a thread" % (type(e).__name__, e))
    if worker is None:
        pool = ThreadPoolExecutor(max_workers=1)
    if worker is not None:      # (what model.prepare_topology needs of the model, as plain values: they travel to the worker process)
        opts = dict(order=int(model.config.edge_order), group_targets=getattr(model, "group_targets", None),
                    radius_column=bool(getattr(model, "tuning", {}).get("group_radius_column", 1)))

    def request(bidx, first=False):
        """Starts the batch's preparation; returns the call that waits for it."""
        if how == "inline" or (first and worker is not None):
            return lambda: prep(bidx)          # (on the main thread, when the batch's turn comes)
        if worker is not None:
            worker.submit(batches[bidx], [confs_of(m["num_refs"]) for m in batches[bidx]], rank, world, opts)
            return worker.result
        return pool.submit(prep, bidx).result
    try:
        arrived = request(mine[0], first=True) if mine else None
        for k, bidx in enumerate(mine):
            # (first this batch's reply, THEN the next request: the worker writes a reply of ~100 MB into a pipe nobody reads until
            # here, and a request larger than the pipe's buffer sent before that would wait for a reader that is itself waiting)
            try:
                packed, topology = arrived()
            except Exception as e:                   # (a worker that died: this batch on the main thread)
                log("run_job: the prepared batch did not arrive (%s: %s); preparing it here" % (type(e).__name__, e))
                packed, topology = prep(bidx)
            try:
                arrived = request(mine[k + 1]) if k + 1 < len(mine) else None
            except Exception as e:                   # (the worker's pipe is gone: the next batch on the main thread, when its turn comes)
                log("run_job: the next batch could not be handed to the worker (%s: %s)" % (type(e).__name__, e))
                arrived = lambda b=mine[k + 1]: prep(b)
            yield bidx, batches[bidx], packed, topology
    finally:
        if worker is not None:
            worker.close()
        if pool is not None:
            pool.shutdown(wait=True)


def load_model(ckpt, precision, trust, device):
    """The score network of the reference checkpoint file `ckpt` (compat.load_checkpoint; trust: unpickle arbitrary classes) on
    `device`, in eval mode; precision None: the model's default."""
    from . import compat, get_model
    ckpt = compat.load_checkpoint(ckpt, trust=trust)
    model = get_model(compat.model_config(ckpt))
    if precision:
        model.precision = precision
    model.load_state_dict(ckpt["model"])
    return model.to(device).eval()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt", required=True, help="reference checkpoint (dict with 'config' and 'model', train.py:219-231)")
    ap.add_argument("--testset", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--num-confs", default="2x")
    ap.add_argument("--start-idx", type=int, default=0)
    ap.add_argument("--end-idx", type=int, default=200)
    ap.add_argument("--n-steps", type=int, default=5000)
    ap.add_argument("--w-global", type=float, default=1.0)
    ap.add_argument("--global-start-sigma", type=float, default=0.5)
    ap.add_argument("--clip", type=float, default=1000.0)
    ap.add_argument("--save-traj", action="store_true")
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--extend-order", action="store_true", help="input holds raw bonds: extend to order 3 first")
    ap.add_argument("--max-atoms", type=int, default=196608,
                    help="atoms per packed batch and GPU (≈200 k is where an MI355X samples fastest: fixed per-launch costs are "
                         "amortised and the node features still live in L2 / MALL; 196,608 = 3 full rounds of the node kernels' "
                         "256 x 16 x 16-node workgroups; --save-traj keeps n_steps x atoms x 12 bytes)")
    ap.add_argument("--seed", type=int, default=2021)
    ap.add_argument("--noise", default="default", choices=["default", "counter"],
                    help="'counter': pos_init and the steps' noise from the counter-based generator (Philox4x32-10 keyed by --seed, "
                         "counter = atom, step, conformer stream id): 'molecule i, conformer c, seed s' draws the same numbers whatever "
                         "--max-atoms, the packing, a --resume or the number of ranks; 'default': torch's generator seeded with "
                         "--seed + rank, drawn over the packed batch")
    ap.add_argument("--prune-rms", type=float, default=None,
                    help="also save, per molecule, which conformers RDKit's pruneRmsThresh rule keeps at this heavy-atom RMSD "
                         "(Angstrom; symmetry-aware): kept_<i> and cluster_<i> next to pos_gen_<i>, which still holds them all")
    ap.add_argument("--prune-tfd", type=float, default=None,
                    help="--prune-rms's keys by the torsion fingerprint deviation (in [0, 1]; agdiff_amd.torsions) instead of the RMSD; "
                         "not together with --prune-rms")
    ap.add_argument("--fix-handedness", action="store_true",
                    help="invert the conformers that came out as the mirror image (the sampler cannot tell the hands apart): needs "
                         "stereo_<i> in the test set (python -m agdiff_amd.stereo); pos_gen_<i> then holds the mirrored conformers and "
                         "hand_<i> the verdict before the fix (-1 mirrored, 0 neither hand: left as sampled, +1 right)")
    ap.add_argument("--fix-double-bonds", action="store_true",
                    help="turn over the double bonds that came out as the wrong E/Z isomer (the bond types do not say which one): needs "
                         "ez_quads_<i> and ez_<i> in the test set (python -m agdiff_amd.ezbonds); one side of each wrong bond is rotated by "
                         "180 degrees about it, after --fix-handedness and before the repairs and checks; pos_gen_<i> then holds the "
                         "flipped conformers and ez_state_<i> [num_samples, D] each bond's state before the fix (+1 right, -1 wrong, 0 "
                         "undecided or untagged); ring bonds are judged, never flipped; with --hold-core the core atoms stay")
    ap.add_argument("--check-geometry", action="store_true",
                    help="also save, per molecule, valid_<i>, bond_dev_<i> and clash_<i>: which conformers pass the bond-length bounds "
                         "and the steric clash scan of agdiff_amd.validity (pos_gen_<i> still holds them all); with --prune-rms / "
                         "--prune-tfd the invalid ones are left out of the walk (cluster_<i> = -1)")
    ap.add_argument("--check-planarity", action="store_true",
                    help="also save, per molecule, flat_<i> and flat_dev_<i>: which conformers keep their aromatic rings and double "
                         "bonds planar (agdiff_amd.planarity; distances cannot see a folded ring or a twisted C=C, so valid_<i> says "
                         "nothing about them); with --prune-rms / --prune-tfd the bent ones are left out of the walk (cluster_<i> = -1)")
    ap.add_argument("--repair-geometry", action="store_true",
                    help="move the atoms of the conformers that fail those two checks into their bounds before anything is saved "
                         "(agdiff_amd.validity.repair_geometry: a projection onto distance bounds from the topology alone, NOT MMFF): "
                         "pos_gen_<i> then holds the repaired conformers, repair_status_<i> (0 valid as sampled, 1 repaired, 2 not "
                         "repaired, 3 not finite) and repair_moved_<i> say what was done; --check-geometry and the prunes see the "
                         "repaired conformers")
    ap.add_argument("--repair-planarity", action="store_true",
                    help="--repair-geometry plus planes, in the same launch (agdiff_amd.planarity.repair_planarity; NOT MMFF): a folded "
                         "aromatic ring, a pyramidal sp2 centre and a twisted double bond are flattened while the bond lengths and "
                         "contacts are held, so a conformer that is bent but otherwise fine comes back usable instead of being dropped "
                         "by --check-planarity; includes --repair-geometry (giving both equals giving this one); the same keys "
                         "repair_status_<i> and repair_moved_<i>; E or Z is not chosen: a double bond twisted past 90 degrees flattens "
                         "into the other isomer, unless --fix-double-bonds ran first")
    ap.add_argument("--track-rmsd", action="store_true",
                    help="also save, per molecule, rmsd_traj_<i> [steps, num_samples]: every conformer's heavy-atom RMSD to the "
                         "molecule's pos_target_<i> of the test set after every denoising step, computed while the run samples "
                         "(agdiff_amd.trajectory) -- the convergence curve without --save-traj's steps x atoms x 12 bytes; not with "
                         "--dist-mode shard over several ranks")
    ap.add_argument("--track-rmsd-mirror", action="store_true",
                    help="--track-rmsd plus rmsd_mirror_traj_<i>: the RMSD of each conformer's mirror image to the target")
    ap.add_argument("--hold-core", action="store_true",
                    help="sample the molecules that carry core_pos_<i> / core_mask_<i> in the test set around that core: its atoms keep "
                         "the template's internal geometry through the run (agdiff_amd.core; the core floats rigidly with the rest), "
                         "pos_gen_<i> is superposed on the template over the core atoms and core_rmsd_<i> [num_samples] says how hard the "
                         "last step pulled against the hold; the other molecules are sampled as ever; not with --dist-mode shard over "
                         "several ranks")
    ap.add_argument("--core-weight", type=float, default=1.0,
                    help="with --hold-core: the fraction of the way the core atoms are moved to the fitted template after every step, in "
                         "(0, 1]; the last step is always held exactly")
    ap.add_argument("--core-start-sigma", type=float, default=float("inf"),
                    help="with --hold-core: hold only after steps whose noise level sigma is below this (default: from the first step)")
    ap.add_argument("--precision", default=None, choices=[None, "f32", "bf16x3", "f16x3"])
    ap.add_argument("--dist-mode", default="shard", choices=["shard", "batches"],
                    help="with several ranks: 'shard' = every packed batch (max-atoms x world atoms) is split into "
                         "contiguous graph ranges, one per rank, with an RCCL all-gather of the positions after each "
                         "denoising step (BASELINE.json north_star); 'batches' = whole batches dealt round-robin")
    ap.add_argument("--trust-ckpt", action="store_true", help="unpickle arbitrary classes from the checkpoint")
    args = ap.parse_args(argv)

    import torch
    import torch.distributed as dist
    from .synth import extend_graph_order_np

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    own_pg = False
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        own_pg = True
    torch.manual_seed(args.seed + rank)
    np.random.seed(args.seed + rank)
    model = load_model(args.ckpt, args.precision, args.trust_ckpt, device)

    mols = [m for m in load_testset(args.testset) if args.start_idx <= m["index"] < args.end_idx]
    if args.extend_order:
        for m in mols:
            r, c, t = extend_graph_order_np(m["atom_type"].shape[0], m["edge_index"][0], m["edge_index"][1],
                                            m["edge_type"], order=model.config.edge_order)
            m["edge_index"], m["edge_type"] = np.stack([r, c]), t
    kw = dict(n_steps=args.n_steps, step_lr=1e-6, w_global=args.w_global, global_start_sigma=args.global_start_sigma,
              clip=args.clip)
    run_job(model, mols, args.out, num_confs(args.num_confs), args.max_atoms, kw, device, save_traj=args.save_traj,
            resume=args.resume, rank=rank, world=world, shard=(world > 1 and args.dist_mode == "shard"), noise=args.noise,
            seed=args.seed, prune_rms=args.prune_rms, fix_handedness=args.fix_handedness, prune_tfd=args.prune_tfd,
            check_geometry=args.check_geometry, check_planarity=args.check_planarity, repair_geometry=args.repair_geometry, track_rmsd=args.track_rmsd, track_rmsd_mirror=args.track_rmsd_mirror,
            repair_planarity=args.repair_planarity, hold_core=args.hold_core, core_weight=args.core_weight,
            core_start_sigma=args.core_start_sigma, fix_double_bonds=args.fix_double_bonds)
    if own_pg:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
