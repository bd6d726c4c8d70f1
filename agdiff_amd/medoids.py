"""K representative conformers of a molecule's sampled ensemble, with their populations -- "the five families that were sampled,
the structure in the middle of each and the share of the ensemble it stands for", for a docking run, a QM refinement or a report;
with K = 1, the most central conformer.  Alternating k-medoids (Voronoi iteration) over the float RMSD or TFD matrix.

Everything runs on the GPU (csrc/eval.hip), and there is no CPU fallback:
    agdiff_rmsd_self / agdiff_tfd_matrix   the symmetry-aware float matrix
    agdiff_maxmin_pick                     the seeds (init="maxmin")
    agdiff_kmedoids                        the walk over that matrix: three grid-wide launches per iteration
    agdiff_align_conformers                Kabsch superposition of the medoids

The rule (include/agdiff_hip.h): from K seeds, every conformer goes to its nearest medoid (ties to the LOWEST rank), then in
every cluster the member with the smallest sum of distances to the other members becomes the medoid (ties to the lowest index,
but an incumbent whose sum equals the minimum stays), until an update changes nothing or `max_iter` updates were made.  All sums
are made on a fixed-point image of the matrix (2^-28), so the result is exact and does not depend on any order.
picks.pick_conformers returns the extremes of the ensemble and clusters.cluster_conformers takes a threshold and returns
however many families it leaves; this takes the count and returns centres.

What this is not: it is not PAM's swap phase -- a medoid only ever moves inside its own cluster; PAM (BUILD + SWAP) is
agdiff_amd.pam, which needs no seeds and can polish this module's result -- and there is no k-means++
seeding.  The result is a local optimum that depends on the seeds; MaxMin seeds start from the outliers of the ensemble, and on
random point clouds they can end at a slightly worse optimum than plain seeds (init="first").  Agreement with any other
package's k-medoids is not claimed.  Whether K families are there at all is agdiff_amd.silhouette's question: it scores this
module's `labels` and sweeps K.

    python -m agdiff_amd.medoids --samples out/samples_all.npz --testset test.npz --count K [--tfd] [--tfd-rings]
                                 [--init maxmin|first] [--max-iter N] [--align] [--fix-handedness] [--fix-double-bonds]
                                 [--drop-invalid] [--drop-bent] --out medoids.npz
"""
import numpy as np

from . import _lib
from .ensemble import (_add_shared_flags, _add_tfd_flags, _attach, _check_tfd_flags, _checked_items, _chosen, _own, _scatter,
                       _usable_matrix, _write_tail)
from .molecule import sampled_items
from .picks import maxmin_pick

MAX_ITER = _lib.DEFINES["AGDIFF_KMEDOIDS_MAX_ITER"]
WORK_BYTES = _lib.DEFINES["AGDIFF_KMEDOIDS_WORK_BYTES"]


def _check_dist(dist, G):
    """the float matrix of every walk: a contiguous float32 tensor [G, G] on the GPU, or ValueError"""
    _lib.require_device_table(dist, "dist must be a contiguous float32 tensor [G, G] on the GPU")
    if tuple(dist.shape) != (G, G):
        raise ValueError("dist must be [%d, %d] (got %s)" % (G, G, tuple(dist.shape)))


def _check_init(init, at_least=0):
    """the seeds of kmedoids and pam.pam_swap: a contiguous int32 tensor [K] on the GPU, K >= at_least, or ValueError"""
    import torch
    if not (torch.is_tensor(init) and init.is_cuda and init.dtype == torch.int32 and init.dim() == 1 and init.is_contiguous()
            and init.shape[0] >= at_least):
        raise ValueError("init must be a contiguous int32 tensor [K] on the GPU" + (", K >= %d" % at_least if at_least else ""))


def _outputs(dist, G, K, work_bytes):
    """what agdiff_kmedoids, agdiff_pam_build and agdiff_pam_swap write, on dist's device: medoids, labels, near, size, within,
    cost, n_iter / n_swaps, status, and their `work`"""
    import torch
    new = lambda n, dtype: torch.empty(n, dtype=dtype, device=dist.device)
    return (new(K, torch.int32), new(G, torch.int32), new(G, torch.float32), new(K, torch.int32), new(K, torch.float64),
            new(1, torch.float64), new(1, torch.int32), new(1, torch.int32), new(work_bytes // 8, torch.int64))


def kmedoids(dist, G, init, max_iter=32):
    """agdiff_kmedoids on a float32 matrix [G, G] on the GPU from the seeds `init` (int32 tensor [K] on the GPU, the medoids of
    rank 0 .. K - 1): (medoids int32 [K], labels int32 [G], near float32 [G], size int32 [K], within float64 [K], cost float64
    [1], n_iter int32 [1], status int32 [1]) -- the medoid of each rank, the rank of every conformer's cluster and the distance
    to its medoid as the matrix stores it (-1 and NaN for a conformer that init[0]'s row marks as unusable), the members and the
    summed distance of each cluster, the total, the number of updates made and 0 (converged) / 1 (stopped at max_iter) / 2 (a seed
    out of range, twice, or unusable: nothing was computed).  More than AGDIFF_PRUNE_MAX_CONFS conformers: AgdiffLimitError."""
    _check_dist(dist, G)
    _check_init(init)
    if int(max_iter) != max_iter or not 1 <= max_iter <= MAX_ITER:
        raise ValueError("max_iter must be a count in 1 .. %d (got %r)" % (MAX_ITER, max_iter))
    K = int(init.shape[0])
    outs = _outputs(dist, G, K, WORK_BYTES)
    _lib.call("agdiff_kmedoids", dist, int(G), K, init, int(max_iter), *outs)
    return outs[:8]


def _explicit_seeds(init, k, names):
    """`init` of medoid_conformers and pam.pam_conformers, one of `names` or k distinct conformer indices (anything else:
    ValueError): (seeds, check) -- the indices as a list of ints, None for a name, and the check(G, mask, why) of theirs that
    ensemble._usable_matrix makes against the item's conformers"""
    listed = ", ".join(map(repr, names))
    seeds = None
    if not isinstance(init, str):
        seeds = np.asarray(init).reshape(-1).tolist()
        if len(seeds) != k or any(int(s) != s for s in seeds) or len(set(seeds)) != len(seeds):
            raise ValueError("init must be one of %s or %d distinct conformer indices (got %r)" % (listed, k, init))
        seeds = [int(s) for s in seeds]
    elif init not in names:
        raise ValueError("init must be one of %s or a sequence of conformer indices (got %r)" % (listed, init))

    def check_seeds(G, mask, why):
        for s in seeds or ():
            if not 0 <= s < G:
                raise ValueError("init: %d is not the index of a conformer, 0 .. %d" % (s, G - 1))
            if mask is not None and not mask[s]:
                raise ValueError("init: %d is a conformer %s" % (s, why))
    return seeds, check_seeds


def _seed_tensor(m, k, init, seeds):
    """The seeds of a walk over the usable conformers of the namespace m (at least one), in their compacted numbering: (int32
    tensor [K] on the device, K).  `seeds`: checked explicit ones in the item's own numbering (K = k); None: `init` says --
    "first", the first K = min(k, G); anything else, the first k MaxMin picks from the first usable conformer, K of them."""
    import torch
    dev, K = m.out.device, min(int(k), m.G)
    if seeds is not None:
        return torch.tensor(seeds if m.mask is None else [int(m.mask[:s].sum()) for s in seeds], dtype=torch.int32, device=dev), K
    if init == "first":
        return torch.arange(K, dtype=torch.int32, device=dev), K
    picks, _, _, _, n_picked, _ = maxmin_pick(m.out, m.G, K)
    K = int(n_picked.item())
    return picks[:K].contiguous(), K


def medoid_conformers(item, k, metric="rmsd", init="maxmin", max_iter=32, align=True, device="cuda", valid=None, fix_handedness=False,
                      fix_double_bonds=False, tfd_rings=False):
    """k-medoids among the item's generated conformers by their best RMSD (metric="tfd": their torsion fingerprint deviation,
    agdiff_amd.torsions; the item must carry its bonds).  The item, `valid`, `fix_handedness` and `fix_double_bonds` are those of
    ensemble.prune_conformers, `tfd_rings` makes the rings terms of the TFD, and the fixes run first.  A conformer with a coordinate
    that is not finite is left out like one that `valid` masks.
        k         the number of medoids (clamped to the number of usable conformers)
        init      the seeds: "maxmin", the first k MaxMin picks from the first usable conformer (fewer picks: that many medoids);
                  "first", the first k usable conformers; or a sequence of k distinct usable conformer indices in the item's own
                  numbering, the medoids of rank 0 .. k - 1 (a masked, repeated or out-of-range one: ValueError)
        max_iter  at most this many updates, 1 .. AGDIFF_KMEDOIDS_MAX_ITER
    Returns a dict in the item's own conformer indices, tensors on `device`:
        medoids     int32 [K]     the medoid of each rank; rank r descends from seed r
        labels      int32 [G]     the rank of every conformer's cluster; -1 when masked
        near        float32 [G]   the distance to its medoid as the matrix stores it, 0 for a medoid; NaN when masked
        count       int32 [K]     the members of each cluster, the medoid included
        population  float32 [K]   count / the number of usable conformers, one correctly rounded fp32 division
        within      float64 [K]   each cluster's summed distance to its medoid (on the 2^-28 grid)
        cost        float         their total: what the walk lowers
        iters       int           the updates made, counting the one that changed nothing
        converged   bool          False when max_iter updates were made and the last one still moved a medoid
        pos         [K, n, 3]     the medoids; with align=True superposed on rank 0 over the heavy atoms (that one is returned as it
                                  is, bit for bit)
        hand, ez_state            as prune_conformers returns them, when the fixes ran
    With no usable conformer the K-sized tensors are empty, `labels` is all -1 and `cost` is 0.  At most AGDIFF_PRUNE_MAX_CONFS
    conformers.  Not PAM (that is agdiff_amd.pam), no k-means++, a local optimum that depends on the seeds: see the module's
    docstring."""
    if int(k) != k or k < 1:
        raise ValueError("k must be a count of at least 1 (got %r)" % (k,))
    if int(max_iter) != max_iter or not 1 <= max_iter <= MAX_ITER:
        raise ValueError("max_iter must be a count in 1 .. %d (got %r)" % (MAX_ITER, max_iter))
    seeds, check_seeds = _explicit_seeds(init, k, ("maxmin", "first"))
    m = _usable_matrix(item, "medoid_conformers", metric, device, valid, fix_handedness, fix_double_bonds, tfd_rings, check=check_seeds)
    return _from_matrix(m, k, init, seeds, max_iter, align)


def _from_matrix(m, k, init, seeds, max_iter, align):
    """medoid_conformers after its matrix: the seeds, the walk and the result, from the namespace m of ensemble._usable_matrix.
    `seeds`: the checked explicit seeds in the item's own numbering, or None when `init` is "maxmin" or "first"."""
    import torch
    if m.G == 0:                                         # no usable conformer: all masked out
        none = lambda dtype: torch.empty(0, dtype=dtype, device=m.gen.device)
        return _attach(m, {"medoids": none(torch.int32), "labels": _scatter(m, none(torch.int32), -1),
                           "near": _scatter(m, none(torch.float32), float("nan")), "count": none(torch.int32),
                           "population": none(torch.float32), "within": none(torch.float64), "cost": 0.0, "iters": 0,
                           "converged": True, "pos": m.gen[:0]})
    first, _ = _seed_tensor(m, k, init, seeds)
    return _result(m, kmedoids(m.out, m.G, first, max_iter=max_iter), seeds, align)


def _result(m, walked, seeds, align):
    """what kmedoids returned for the usable conformers of m as medoid_conformers' dict, in the item's own numbering"""
    import torch
    medoids, labels, near, size, within, cost, n_iter, status = walked
    dev = m.out.device
    status = int(status.item())
    if status == 2:
        raise ValueError("init: a seed is as far from conformer %d as the matrix can say (not a number >= 0 and <= %d): the "
                         "seeds must be usable together" % (seeds[0] if seeds else 0, _lib.DEFINES["AGDIFF_KMEDOIDS_MAX_DIST"]))
    pos = _chosen(m, medoids, align)
    counts = size.cpu().numpy()                          # (the division on the host: one correctly rounded fp32 quotient each)
    population = torch.from_numpy(counts.astype(np.float32) / np.float32(max(int(counts.sum()), 1))).to(dev)
    return _attach(m, {"medoids": _own(m, medoids), "labels": _scatter(m, labels, -1), "near": _scatter(m, near, float("nan")),
                       "count": size, "population": population, "within": within, "cost": float(cost.item()),
                       "iters": int(n_iter.item()), "converged": status == 0, "pos": pos})


def _parser():
    import argparse

    class Parser(argparse.ArgumentParser):
        def parse_args(self, *a, **kw):
            args = super().parse_args(*a, **kw)
            if args.count < 1:
                self.error("--count must be at least 1")
            if not 1 <= args.max_iter <= MAX_ITER:
                self.error("--max-iter must be in 1 .. %d" % MAX_ITER)
            _check_tfd_flags(self, args)
            return args
    ap = Parser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    _add_shared_flags(ap)
    ap.add_argument("--count", type=int, required=True, help="the number of medoids per molecule")
    _add_tfd_flags(ap)
    ap.add_argument("--init", choices=("maxmin", "first"), default="maxmin",
                    help="the seeds: the first K MaxMin picks (agdiff_amd.picks), or the first K conformers that are not left out")
    ap.add_argument("--max-iter", type=int, default=32, help="at most this many updates (1 .. %d)" % MAX_ITER)
    return ap


def _write_medoids(out, i, res, steps_key, count=True):
    """molecule i's result of medoid_conformers (steps_key "iters") or pam.pam_conformers ("swaps") into `out`, as python -m
    agdiff_amd.medoids, .pam and .silhouette --sweep write it; count=False (the sweep, whose silhouette part writes the same
    `count_<i>`) leaves that key out"""
    for key, name in (("medoids", "medoid"), ("labels", "cluster"), ("near", "dist"), ("count", "count"),
                      ("population", "population"), ("within", "within"), ("pos", "pos")):
        if count or key != "count":
            out["%s_%d" % (name, i)] = res[key].cpu().numpy()
    out["cost_%d" % i] = np.float64(res["cost"])
    out["%s_%d" % (steps_key, i)] = np.int32(res[steps_key])
    out["converged_%d" % i] = np.int8(res["converged"])


def main(argv=None):
    """python -m agdiff_amd.medoids --samples samples_all.npz --testset test.npz --count K [--tfd] [--init maxmin|first] [--align] --out medoids.npz
    K representative conformers of a finished job's molecules (agdiff_amd.driver: `pos_gen_<i>`) with their populations:
    k-medoids over the RMSD or TFD matrix.  The bonds come from the test set, so the molecules' symmetry is honoured.  Writes per
    molecule `medoid_<i>` [K], `cluster_<i>` [G] (the rank of each conformer's cluster; -1 when left out), `dist_<i>` [G] (the
    distance to its medoid; NaN when left out), `count_<i>` [K], `population_<i>` [K] (the share of the conformers that were
    not left out), `within_<i>` float64 [K], `cost_<i>` float64, `iters_<i>` int32, `converged_<i>` int8, `pos_<i>` [K, n, 3]
    (+ `name_<i>`).  --fix-handedness, --fix-double-bonds, --drop-invalid, --drop-bent: as in python -m agdiff_amd.ensemble, with the
    same `hand_<i>`, `ez_state_<i>`, `valid_<i>` and `flat_<i>`.  Prints the conformers, the medoids, the molecules that did not
    converge and the largest population of a medoid."""
    args = _parser().parse_args(argv)
    metric = "tfd" if args.tfd else "rmsd"
    out, total, found, open_, top = {}, 0, 0, 0, 0.0
    for mol, item, valid in _checked_items(sampled_items(args.testset, args.samples), args, out):
        i = mol["index"]
        res = medoid_conformers(item, args.count, metric=metric, init=args.init, max_iter=args.max_iter, align=args.align,
                                device=args.device, valid=valid, fix_handedness=args.fix_handedness,
                                fix_double_bonds=args.fix_double_bonds, tfd_rings=args.tfd_rings)
        _write_medoids(out, i, res, "iters")
        _write_tail(out, mol, res)
        total += int(res["labels"].shape[0])
        found += int(res["medoids"].shape[0])
        open_ += 0 if res["converged"] else 1
        top = max([top] + res["population"].cpu().tolist())
    np.savez_compressed(args.out, **out)
    print("%d medoids of %d conformers by %s (%d per molecule, %s seeds, at most %d updates; %d molecules did not converge); "
          "largest population of a medoid: %.3f" % (found, total, "TFD" if args.tfd else "RMSD", args.count, args.init, args.max_iter,
                                                     open_, top))
    return out


if __name__ == "__main__":
    main()
