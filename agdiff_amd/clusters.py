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
from .ensemble import _add_shared_flags, _attach, _checked_items, _chosen, _own, _scatter, _usable_matrix, _write_tail
from .molecule import check_threshold, sampled_items


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
    m = _usable_matrix(item, "cluster_conformers", metric, device, valid, fix_handedness, fix_double_bonds, tfd_rings,
                       threshold=threshold, want_out=distances, finite_only=False)
    if m.G == 0:                                         # no conformer to cluster: all masked out
        none = lambda dtype: torch.empty(0, dtype=dtype, device=m.gen.device)
        res = {"centroids": none(torch.int32), "leader": _scatter(m, none(torch.int32), -1),
               "cluster": _scatter(m, none(torch.int32), -1), "count": none(torch.int32), "population": none(torch.float32),
               "pos": m.gen[:0]}
        if distances:
            res["dist"] = _scatter(m, none(torch.float32), float("nan"))
        return _attach(m, res)
    leader, count, rank, _ = butina_cluster(m.bits, m.G, reorder=reorder)
    cent = torch.nonzero(count, as_tuple=False).reshape(-1)
    cent = cent[torch.argsort(rank[cent])]               # creation order (the ranks of the centroids are 0 .. K - 1, each once)
    size = count[cent]
    res = {"centroids": _own(m, cent), "leader": _scatter(m, _own(m, leader), -1), "cluster": _scatter(m, rank, -1), "count": size,
           "population": size.to(torch.float32) / float(m.G), "pos": _chosen(m, cent, align)}
    if distances:
        res["dist"] = _scatter(m, m.out[leader.long(), torch.arange(m.G, device=m.out.device)], float("nan"))
    return _attach(m, res)


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    _add_shared_flags(ap)
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--rms", type=float, default=None, help="RMSD threshold in Angstrom (heavy atoms)")
    how.add_argument("--tfd", type=float, default=None,
                     help="torsion fingerprint deviation threshold in [0, 1] (agdiff_amd.torsions) instead of an RMSD")
    ap.add_argument("--tfd-rings", action="store_true",
                    help="with --tfd: the rings are terms of the TFD too (agdiff_amd.rings): chair and boat are two families")
    ap.add_argument("--static", action="store_true",
                    help="count the neighbours once, over all conformers (ClusterData(reordering=False)); the default counts the "
                         "conformers still unclustered at every choice")
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
    for mol, item, valid in _checked_items(sampled_items(args.testset, args.samples), args, out):
        i = mol["index"]
        res = cluster_conformers(item, threshold, metric=metric, reorder=not args.static, align=args.align, device=args.device,
                                 valid=valid, fix_handedness=args.fix_handedness, fix_double_bonds=args.fix_double_bonds,
                                 tfd_rings=args.tfd_rings)
        out["centroid_%d" % i] = res["centroids"].cpu().numpy()
        for key in ("cluster", "leader", "count", "population", "dist", "pos"):
            out["%s_%d" % (key, i)] = res[key].cpu().numpy()
        _write_tail(out, mol, res)
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
