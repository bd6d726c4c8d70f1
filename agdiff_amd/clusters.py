"""Conformer families -- what the sampler found, how populated each family is and which conformer stands for it: Taylor-Butina
clustering (RDKit's Butina.ClusterData) of a molecule's sampled conformers over the thresholded RMSD or TFD matrix.

Everything runs on the GPU (csrc/eval.hip), and there is no CPU fallback:
    agdiff_rmsd_self / agdiff_tfd_matrix   the symmetry-aware matrix and its adjacency under the threshold as a bit-matrix
    agdiff_butina_cluster                  the clustering over that bit-matrix, one workgroup
    agdiff_align_conformers                Kabsch superposition of the centroids

The rule (include/agdiff_hip.h): every conformer starts live; among the live ones the conformer with the most neighbours -- ties to
the LOWEST index -- becomes a centroid and takes its live neighbours with it; repeat until nobody is live.  reorder=True counts the
neighbours still live at each choice (Butina's algorithm, ClusterData(reordering=True)); reorder=False counts them once over all
conformers (reordering=False).  ensemble.prune_conformers answers "which conformers differ" and depends on the sampling order; this
answers "which families are there", and its centroid is the member in the middle of its family.

    python -m agdiff_amd.clusters --samples out/samples_all.npz --testset test.npz (--rms 0.5 | --tfd 0.2) [--static] [--align]
                                  [--fix-handedness] [--fix-double-bonds] [--drop-invalid] [--drop-bent] --out clusters.npz
"""
import numpy as np

from . import _lib
from .ensemble import MAX_CONFS, _align, _self_rmsd, _valid_mask
from .evaluation import selection_of
from .ezbonds import fix_double_bonds as _fix_double_bonds
from .molecule import check_threshold, num_atoms, sampled_items
from .planarity import check_planarity
from .stereo import fix_handedness as _fix_handedness
from .validity import check_geometry


def butina_cluster(bits, G, reorder=True):
    """agdiff_butina_cluster on a packed bit-matrix (int64 [G, pitch / 8] on the GPU, ensemble.bits_pitch): (leader, count, rank,
    n_clusters) int32 -- each conformer's centroid, the cluster size at a centroid (0 elsewhere), the creation order of each
    conformer's cluster, and the number of clusters [1].  More than AGDIFF_PRUNE_MAX_CONFS conformers: AgdiffLimitError."""
    import torch
    dev = bits.device
    leader, count, rank = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(3))
    n_clusters = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("agdiff_butina_cluster", bits, G, 1 if reorder else 0, leader, count, rank, n_clusters)
    return leader, count, rank, n_clusters


def _empty(total, gen, distances, hand, ez_state):
    """the result with no conformer to cluster: `total` conformers, all masked out"""
    import torch
    dev = gen.device
    none = lambda dtype: torch.empty(0, dtype=dtype, device=dev)
    res = {"centroids": none(torch.int32), "leader": torch.full((total,), -1, dtype=torch.int32, device=dev),
           "cluster": torch.full((total,), -1, dtype=torch.int32, device=dev), "count": none(torch.int32),
           "population": none(torch.float32), "pos": gen[:0]}
    if distances:
        res["dist"] = torch.full((total,), float("nan"), dtype=torch.float32, device=dev)
    if hand is not None:
        res["hand"] = hand
    if ez_state is not None:
        res["ez_state"] = ez_state
    return res


def cluster_conformers(item, threshold, metric="rmsd", reorder=True, align=True, device="cuda", valid=None, fix_handedness=False,
                       fix_double_bonds=False, distances=True, tfd_rings=False):
    """Taylor-Butina clustering of the item's generated conformers: two conformers are neighbours when their best RMSD (metric="tfd":
    their torsion fingerprint deviation, agdiff_amd.torsions; the item must carry its bonds) is at most `threshold`.  The item, the
    threshold, `valid`, `fix_handedness`, `fix_double_bonds` and `tfd_rings` (the rings as terms of the TFD) are those of
    ensemble.prune_conformers, and the fixes run first.
    Returns a dict of tensors on `device`:
        centroids  int32 [K]    the centroid of every cluster in creation order, as indices into the item's conformers
        leader     int32 [G]    every conformer's centroid (itself for a centroid); -1 for a conformer that `valid` masks out
        cluster    int32 [G]    the rank of every conformer's cluster: centroids[cluster[i]] == leader[i]; -1 when masked
        count      int32 [K]    the size of every cluster
        population float32 [K]  count / the number of clustered conformers
        pos        [K, n, 3]    the centroids; with align=True superposed on the first of them over the heavy atoms (that one is
                                returned as it is, bit for bit)
        dist       float32 [G]  (distances=True) every conformer's distance to its centroid as the matrix stores it; NaN when masked
        hand, ez_state          as prune_conformers returns them, when the fixes ran
    With no valid conformer the K-sized tensors are empty and `leader` is all -1.  At most AGDIFF_PRUNE_MAX_CONFS conformers."""
    import torch
    if metric not in ("rmsd", "tfd"):
        raise ValueError("metric must be 'rmsd' or 'tfd' (got %r)" % (metric,))
    if tfd_rings and metric != "tfd":
        raise ValueError("tfd_rings goes with metric='tfd'")
    t = check_threshold(threshold, "RMSD")
    gen = _lib.conformers(item["pos_gen"], num_atoms(item))
    G = total = gen.shape[0]
    if G == 0:
        raise ValueError("no conformers to cluster")
    if G > MAX_CONFS:
        raise _lib.AgdiffLimitError("cluster_conformers: %d conformers, more than AGDIFF_PRUNE_MAX_CONFS = %d" % (G, MAX_CONFS))
    mask = None if valid is None else _valid_mask(valid, G)
    hand = None
    if fix_handedness:
        gen = gen.to(device).contiguous().clone()        # (the caller's tensor is never written)
        hand = _fix_handedness(item, gen)
    ez_state = None
    if fix_double_bonds:
        gen = gen.to(device).contiguous()
        if not fix_handedness:
            gen = gen.clone()                            # (the caller's tensor is never written)
        ez_state = _fix_double_bonds(item, gen)
    sel = None
    if mask is not None:                                 # compacted on the device; the kernels below see the valid ones only
        gen = gen.to(device).contiguous()
        sel = torch.nonzero(torch.from_numpy(mask).to(gen.device), as_tuple=False).reshape(-1)
        G = int(sel.shape[0])
        if G == 0:
            return _empty(total, gen, distances, hand, ez_state)
        gen = gen[sel].contiguous()
    if metric == "tfd":
        from .torsions import _self_tfd
        # (the keyword is passed only when set: without the switch this is, argument for argument, the call it was before)
        gen, out, bits = _self_tfd(dict(item, pos_gen=gen), device, threshold=t, want_out=distances,
                                   **({"rings": True} if tfd_rings else {}))
        idx = torch.from_numpy(selection_of({"atom_type": item["atom_type"]})[1]).to(device)
    else:
        gen, idx, out, bits = _self_rmsd(dict(item, pos_gen=gen), device, threshold=t, want_out=distances)
    leader, count, rank, _ = butina_cluster(bits, G, reorder=reorder)
    cent = torch.nonzero(count, as_tuple=False).reshape(-1)
    cent = cent[torch.argsort(rank[cent])]               # creation order (the ranks of the centroids are 0 .. K - 1, each once)
    pos = gen[cent]
    if align and pos.shape[0] > 0:
        first = pos[0].clone()
        pos, _ = _align(pos, idx, first)
        pos[0] = first
    size = count[cent]
    res = {"centroids": cent.to(torch.int32), "leader": leader, "cluster": rank, "count": size,
           "population": size.to(torch.float32) / float(G), "pos": pos}
    if distances:
        res["dist"] = out[leader.long(), torch.arange(G, device=out.device)]
    if sel is not None:                                  # back to the item's own conformer indices
        lead = torch.full((total,), -1, dtype=torch.int32, device=leader.device)
        lead[sel] = sel[leader.long()].to(torch.int32)
        clus = torch.full((total,), -1, dtype=torch.int32, device=leader.device)
        clus[sel] = rank
        res["centroids"], res["leader"], res["cluster"] = sel[cent].to(torch.int32), lead, clus
        if distances:
            dist = torch.full((total,), float("nan"), dtype=torch.float32, device=leader.device)
            dist[sel] = res["dist"]
            res["dist"] = dist
    if hand is not None:
        res["hand"] = hand
    if ez_state is not None:
        res["ez_state"] = ez_state
    return res


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", required=True)
    ap.add_argument("--testset", required=True)
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--rms", type=float, default=None, help="RMSD threshold in Angstrom (heavy atoms)")
    how.add_argument("--tfd", type=float, default=None,
                     help="torsion fingerprint deviation threshold in [0, 1] (agdiff_amd.torsions) instead of an RMSD")
    ap.add_argument("--tfd-rings", action="store_true",
                    help="with --tfd: the rings are terms of the TFD too (agdiff_amd.rings): chair and boat are two families")
    ap.add_argument("--static", action="store_true",
                    help="count the neighbours once, over all conformers (ClusterData(reordering=False)); the default counts the "
                         "conformers still unclustered at every choice")
    ap.add_argument("--align", action="store_true", help="superpose the centroids on the first of them")
    ap.add_argument("--fix-handedness", action="store_true", help="invert the mirror-image conformers first (needs stereo_<i> in --testset)")
    ap.add_argument("--fix-double-bonds", action="store_true",
                    help="turn over the double bonds of the wrong E/Z parity first, after --fix-handedness (needs ez_quads_<i> and ez_<i> "
                         "in --testset: python -m agdiff_amd.ezbonds); also writes ez_state_<i> [G, D]")
    ap.add_argument("--drop-invalid", action="store_true",
                    help="leave the conformers with a bond out of bounds or a steric clash (agdiff_amd.validity) out of the clustering")
    ap.add_argument("--drop-bent", action="store_true",
                    help="leave the conformers with an aromatic ring or a double bond out of plane (agdiff_amd.planarity) out of it")
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None):
    """python -m agdiff_amd.clusters --samples samples_all.npz --testset test.npz (--rms T | --tfd T) [--static] [--align] --out clusters.npz
    Clusters a finished job's output (agdiff_amd.driver: `pos_gen_<i>`).  The bonds come from the test set, so the molecules'
    symmetry is honoured.  Writes per molecule `centroid_<i>` [K] (creation order), `cluster_<i>` [G] (the rank; -1 when left out),
    `leader_<i>` [G], `count_<i>` [K], `population_<i>` [K], `dist_<i>` [G] (to the centroid; NaN when left out), `pos_<i>` [K, n, 3]
    (+ `name_<i>`).  Exactly one of --rms / --tfd T.  --static: neighbour counts taken once (reorder=False).  --fix-handedness,
    --fix-double-bonds, --drop-invalid, --drop-bent: as in python -m agdiff_amd.ensemble, with the same `hand_<i>`, `ez_state_<i>`,
    `valid_<i>` and `flat_<i>`.  Prints the conformers, the clusters and the share of its conformers that a molecule's largest
    cluster holds, averaged over the molecules."""
    args = _parser().parse_args(argv)
    metric, threshold = ("rmsd", args.rms) if args.tfd is None else ("tfd", args.tfd)
    check_threshold(threshold, "RMSD")
    out, total, clusters, top = {}, 0, 0, []
    for mol, item in sampled_items(args.testset, args.samples):
        i = mol["index"]
        if args.fix_handedness:
            if mol.get("stereo") is None:
                raise ValueError("--fix-handedness: %s has no stereo_%d (python -m agdiff_amd.stereo adds it)" % (args.testset, i))
            item["stereo"] = mol["stereo"]
        if args.fix_double_bonds:
            if mol.get("ez_quads") is None or mol.get("ez") is None:
                raise ValueError("--fix-double-bonds: %s has no ez_quads_%d / ez_%d (python -m agdiff_amd.ezbonds adds them)"
                                 % (args.testset, i, i))
            item["ez_quads"], item["ez"] = mol["ez_quads"], mol["ez"]
        valid = None
        if args.drop_invalid:
            valid = check_geometry(item, device=args.device)["valid"]
            out["valid_%d" % i] = valid.cpu().numpy().astype(np.int8)
        if args.drop_bent:
            flat = check_planarity(item, device=args.device)["flat"]
            out["flat_%d" % i] = flat.cpu().numpy().astype(np.int8)
            valid = flat if valid is None else valid & flat
        res = cluster_conformers(item, threshold, metric=metric, reorder=not args.static, align=args.align, device=args.device,
                                 valid=valid, fix_handedness=args.fix_handedness, fix_double_bonds=args.fix_double_bonds,
                                 tfd_rings=args.tfd_rings)
        out["centroid_%d" % i] = res["centroids"].cpu().numpy()
        for key in ("cluster", "leader", "count", "population", "dist", "pos"):
            out["%s_%d" % (key, i)] = res[key].cpu().numpy()
        out["name_%d" % i] = np.str_(mol["name"])
        if "hand" in res:
            out["hand_%d" % i] = res["hand"].cpu().numpy().astype(np.int8)
        if "ez_state" in res:
            out["ez_state_%d" % i] = res["ez_state"].cpu().numpy().astype(np.int8)
        total += int(res["leader"].shape[0])
        clusters += int(res["centroids"].shape[0])
        if res["population"].shape[0]:
            top.append(float(res["population"].max()))
    np.savez_compressed(args.out, **out)
    print("clustered %d conformers into %d clusters at %s %.3f (%s counts); largest cluster: %.1f %% of a molecule's conformers on average"
          % (total, clusters, "TFD" if metric == "tfd" else "RMSD", threshold, "static" if args.static else "live",
             100.0 * float(np.mean(top)) if top else 0.0))
    return out


if __name__ == "__main__":
    main()
