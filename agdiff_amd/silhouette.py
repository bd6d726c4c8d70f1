"""How good is a clustering of a molecule's sampled ensemble, and how many families are there -- the question after the first
`--count 5`: the silhouette coefficient (Rousseeuw 1987) of every conformer under a given clustering over the float RMSD or TFD
matrix, and a sweep of k-medoids over K that returns the count with the highest mean silhouette.

Everything runs on the GPU (csrc/eval.hip), and there is no CPU fallback:
    agdiff_rmsd_self / agdiff_tfd_matrix   the symmetry-aware float matrix
    agdiff_silhouette                      the coefficients: the matrix is streamed once, row i into one integer bin per cluster
    agdiff_maxmin_pick / agdiff_kmedoids   the sweep's seeds (made once: the first K MaxMin picks are a prefix) and its walks

The rule (include/agdiff_hip.h): a(i) is conformer i's mean distance to the other members of its cluster, b(i) its smallest mean
distance to the members of another cluster (ties to the LOWEST rank; empty clusters do not count), s(i) = (b - a) / max(a, b), and
s(i) = 0 for a singleton, with no other cluster, or when both are 0.  s near 1: i sits well inside its family; near 0: between
two; below 0: its neighbours are in the other one.  All sums are made on a fixed-point image of the matrix (2^-28) and the means of
s on one of s (2^-40), so every number is exact and does not depend on any order.  The labels are any clustering's: `cluster_<i>`
as python -m agdiff_amd.clusters, .medoids and .ensemble write it, `owner_<i>` of .picks; -1 is "left out".

What this is not: it is the full O(G^2) silhouette, not the simplified (medoid-based) one; there is no gap statistic and no
Davies-Bouldin index; the sweep is over k-medoids' K only, not over Butina thresholds, and it inherits k-medoids' dependence on
its seeds (a low curve may be a poor local optimum and not a poor K); the sampling driver has no flag for it.  Agreement with
scikit-learn's silhouette_samples is by definition only, not bit for bit.  The chemistry is unverified: nobody has run this on a
trained checkpoint's ensembles.

    python -m agdiff_amd.silhouette --samples out/samples_all.npz --testset test.npz
                                    (--labels clusters.npz [--label-key cluster] | --sweep LO HI [--init maxmin|first] [--max-iter N])
                                    [--tfd] [--tfd-rings] [--align] [--fix-handedness] [--fix-double-bonds] [--drop-invalid]
                                    [--drop-bent] --out sil.npz
"""
import numpy as np

from . import _lib
from .ensemble import (_add_shared_flags, _add_tfd_flags, _attach, _check_tfd_flags, _checked_items, _scatter, _usable_matrix,
                       _write_tail)
from .medoids import MAX_ITER, _check_dist, _result, _seed_tensor, _write_medoids, kmedoids
from .molecule import as_host, num_atoms, sampled_items

MAX_CONFS = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"]
WORK_BYTES = _lib.DEFINES["AGDIFF_SILHOUETTE_WORK_BYTES"]
MAX_SWEEP = 64                                           # most values of K per sweep_medoids call: a bound on the launches, not tuned


def silhouette(dist, G, labels, K):
    """agdiff_silhouette on a float32 matrix [G, G] on the GPU under the clustering `labels` (int32 tensor [G] on the GPU: -1 left
    out, 0 .. K - 1 the rank of a member's cluster): (a float64 [G], b float64 [G], s float64 [G], other int32 [G], size int32 [K],
    cluster_mean float64 [K], mean float64 [1], status int32 [1]) -- every conformer's mean distance to the other members of its
    cluster, to the members of the nearest other cluster, its silhouette coefficient and that other cluster's rank (NaN and -1 for
    a conformer that is left out; b NaN and other -1 with no other cluster), the members of each rank, the mean coefficient of each
    (NaN when empty) and of all members, and 0 / 2 (a label outside -1 .. K - 1: nothing was computed, everything is NaN, -1
    or 0).  The labels are checked on the device and never read here.  More than AGDIFF_PRUNE_MAX_CONFS conformers: AgdiffLimitError."""
    import torch
    _check_dist(dist, G)
    if not (torch.is_tensor(labels) and labels.is_cuda and labels.dtype == torch.int32 and labels.dim() == 1 and labels.is_contiguous()
            and labels.shape[0] == G):
        raise ValueError("labels must be a contiguous int32 tensor [%d] on the GPU" % G)
    if int(K) != K or not 1 <= K <= MAX_CONFS:
        raise ValueError("K must be a count in 1 .. %d (got %r)" % (MAX_CONFS, K))
    dev, K = dist.device, int(K)
    a, b, s = (torch.empty(G, dtype=torch.float64, device=dev) for _ in range(3))
    other = torch.empty(G, dtype=torch.int32, device=dev)
    size = torch.empty(K, dtype=torch.int32, device=dev)
    cluster_mean = torch.empty(K, dtype=torch.float64, device=dev)
    mean = torch.empty(1, dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    work = torch.empty(WORK_BYTES // 8, dtype=torch.int64, device=dev)
    _lib.call("agdiff_silhouette", dist, int(G), K, labels, a, b, s, other, size, cluster_mean, mean, status, work)
    return a, b, s, other, size, cluster_mean, mean, status


def label_ranks(labels):
    """(values int64 [K], ranks int32 [G]) of a clustering's labels: the distinct values >= 0 in ascending order and every
    conformer's rank among them, -1 for -1.  Anything but a one-dimensional integer array with values >= -1 that fit 32 bits is
    a ValueError.  `cluster_<i>` of python -m agdiff_amd.ensemble holds kept-conformer indices and not ranks: they map like any
    other values."""
    lab = as_host(labels)
    if lab.dtype.kind not in "iu" or lab.ndim != 1:
        raise ValueError("labels must be an integer array with one entry per conformer (got %s %s)" % (lab.dtype, tuple(lab.shape)))
    lab = lab.astype(np.int64)
    if lab.size and (lab.min() < -1 or lab.max() > 0x7fffffff):
        raise ValueError("labels must be -1 (left out) or a cluster's value in 0 .. 2^31 - 1 (got %d .. %d)" % (lab.min(), lab.max()))
    values = np.unique(lab[lab >= 0])
    ranks = np.where(lab >= 0, np.searchsorted(values, lab), -1).astype(np.int32)
    return values, ranks


def _scored(m, ranks, values):
    """silhouette of the usable conformers of the namespace m under `ranks` (int32 tensor on the device, one per usable conformer)
    as silhouette_conformers' dict, in the item's own numbering and the caller's label values"""
    import torch
    K, dev = int(values.shape[0]), m.gen.device
    nan = float("nan")
    if m.G == 0 or K == 0:                               # nothing to score: no launch
        none = torch.empty(0, dtype=torch.float64, device=dev)
        full = lambda fill, dtype: torch.full((m.total,), fill, dtype=dtype, device=dev)
        return _attach(m, {"s": full(nan, torch.float64), "a": full(nan, torch.float64), "b": full(nan, torch.float64),
                           "other": full(-1, torch.int32), "values": values, "count": torch.zeros(K, dtype=torch.int32, device=dev),
                           "cluster_mean": torch.full((K,), nan, dtype=torch.float64, device=dev) if K else none, "mean": nan})
    a, b, s, other, size, cluster_mean, mean, _ = silhouette(m.out, m.G, ranks, K)      # (status 0: the ranks were made here)
    table = torch.from_numpy(values.astype(np.int32)).to(dev)
    other = torch.where(other >= 0, table[other.clamp(min=0).long()], other)
    return _attach(m, {"s": _scatter(m, s, nan), "a": _scatter(m, a, nan), "b": _scatter(m, b, nan), "other": _scatter(m, other, -1),
                       "values": values, "count": size, "cluster_mean": cluster_mean, "mean": float(mean.item())})


def silhouette_conformers(item, labels, metric="rmsd", device="cuda", valid=None, fix_handedness=False, fix_double_bonds=False,
                          tfd_rings=False):
    """The silhouette coefficients of the item's generated conformers under the clustering `labels`, by their best RMSD
    (metric="tfd": their torsion fingerprint deviation, agdiff_amd.torsions; the item must carry its bonds).  The item, `valid`,
    `fix_handedness`, `fix_double_bonds` and `tfd_rings` are those of medoids.medoid_conformers, and the fixes run first.
        labels  any integer array (numpy or tensor) with one entry per conformer of the item: equal values are one cluster, -1 is
                left out.  The distinct values >= 0 become the ranks 0 .. K - 1 in ascending order, so ranks (`cluster_<i>` of
                clusters and medoids, `owner_<i>` of picks) and kept-conformer indices (`cluster_<i>` of ensemble) both serve.
                A value below -1 or a wrong shape: ValueError, before any device work.
    A conformer that `valid` masks, or one with a coordinate that is not finite, is left out even when it is labelled.
    Returns a dict in the item's own conformer indices, tensors on `device`:
        s, a, b       float64 [G]   the coefficient, the mean distance to the own cluster's other members and to the nearest other
                                    cluster's members (in the matrix's units, on the 2^-28 grid); NaN when left out; b NaN with
                                    no other cluster
        other         int32 [G]     that nearest other cluster, as the caller's label value; -1 for none or when left out
        values        int64 [K]     the distinct labels, ascending (numpy): what the K-sized entries are indexed by
        count         int32 [K]     the scored members of each cluster
        cluster_mean  float64 [K]   the mean coefficient of each cluster's members; NaN when none was scored
        mean          float         the mean coefficient of all scored conformers; NaN when there are none
        hand, ez_state              as prune_conformers returns them, when the fixes ran
    At most AGDIFF_PRUNE_MAX_CONFS conformers.  The full silhouette, not the simplified one: see the module's docstring."""
    import torch
    values, ranks = label_ranks(labels)

    def check_shape(G, mask, why):
        if ranks.shape[0] != G:
            raise ValueError("labels must have one entry per conformer: [%d] (got [%d])" % (G, ranks.shape[0]))
    m = _usable_matrix(item, "silhouette_conformers", metric, device, valid, fix_handedness, fix_double_bonds, tfd_rings,
                       check=check_shape)
    usable = ranks if m.mask is None else ranks[m.mask]
    return _scored(m, torch.from_numpy(np.ascontiguousarray(usable)).to(m.gen.device), values)


def _check_sweep(k_min, k_max, init, max_iter):
    if int(k_min) != k_min or int(k_max) != k_max or not 2 <= k_min <= k_max:
        raise ValueError("the sweep needs counts 2 <= k_min <= k_max (got %r, %r)" % (k_min, k_max))
    if k_max - k_min + 1 > MAX_SWEEP:
        raise ValueError("at most %d values of K per sweep (got %d .. %d)" % (MAX_SWEEP, k_min, k_max))
    if init not in ("maxmin", "first"):
        raise ValueError("init must be 'maxmin' or 'first' (got %r)" % (init,))
    if int(max_iter) != max_iter or not 1 <= max_iter <= MAX_ITER:
        raise ValueError("max_iter must be a count in 1 .. %d (got %r)" % (MAX_ITER, max_iter))


def sweep_medoids(item, k_min, k_max, metric="rmsd", init="maxmin", max_iter=32, align=True, device="cuda", valid=None,
                  fix_handedness=False, fix_double_bonds=False, tfd_rings=False):
    """"How many families": k-medoids (medoids.medoid_conformers, same arguments) for every K in k_min .. k_max over ONE matrix and
    from ONE set of seeds -- the first K MaxMin picks are a prefix of the first k_max (init="first": the first K usable
    conformers) -- each scored by its mean silhouette, all on the device.  2 <= k_min <= k_max, at most 64 values of K; k_max is
    clamped to the number of usable conformers and, with MaxMin seeds, to the number of picks there are.
    Returns a dict:
        k          int32 [n]     the values of K that were run (numpy, like the other curves)
        mean       float64 [n]   the mean silhouette at each K
        cost       float64 [n]   k-medoids' total cost at each K
        iters      int32 [n]     its updates
        converged  bool [n]      False where it stopped at max_iter
        best_k     int           the K with the highest mean silhouette, ties to the SMALLEST K, a NaN never wins; 0 when no K was
                                 run (fewer than k_min usable conformers or picks)
        medoids    dict          medoid_conformers' result at best_k, tensor for tensor (None when no K was run)
        silhouette dict          silhouette_conformers' result for that clustering's labels (None when no K was run)
    The curve inherits k-medoids' dependence on its seeds.  Not a gap statistic: see the module's docstring."""
    import torch
    _check_sweep(k_min, k_max, init, max_iter)
    m = _usable_matrix(item, "sweep_medoids", metric, device, valid, fix_handedness, fix_double_bonds, tfd_rings)
    hi = min(int(k_max), m.G)
    if hi >= k_min:                                      # the seeds of k_max, made once: those of every K are a prefix
        seeds, hi = _seed_tensor(m, hi, init, None)
    ks = list(range(int(k_min), hi + 1))
    if not ks:
        none = lambda dtype: np.zeros(0, dtype=dtype)
        return {"k": none(np.int32), "mean": none(np.float64), "cost": none(np.float64), "iters": none(np.int32),
                "converged": none(np.bool_), "best_k": 0, "medoids": None, "silhouette": None}
    walks, scores = [], []
    for K in ks:                                         # nothing in this loop synchronises
        walks.append(kmedoids(m.out, m.G, seeds[:K].contiguous(), max_iter=max_iter))
        scores.append(silhouette(m.out, m.G, walks[-1][1], K))
    column = lambda rows, j: torch.cat([r[j] for r in rows]).cpu().numpy()
    mean, cost, iters, status = column(scores, 6), column(walks, 5), column(walks, 6), column(walks, 7)
    best = 0
    for j in range(1, len(ks)):                          # the highest mean, ties to the smallest K; a NaN never wins
        if mean[j] > mean[best] or (np.isnan(mean[best]) and not np.isnan(mean[j])):
            best = j
    K = ks[best]
    res = _result(m, walks[best], None, align)           # (raises on a bad seed, as medoid_conformers does)
    values = np.arange(K, dtype=np.int64)
    return {"k": np.array(ks, dtype=np.int32), "mean": mean, "cost": cost, "iters": iters.astype(np.int32), "converged": status == 0,
            "best_k": K, "medoids": res, "silhouette": _scored(m, walks[best][1], values)}


def _parser():
    import argparse

    class Parser(argparse.ArgumentParser):
        def parse_args(self, *a, **kw):
            args = super().parse_args(*a, **kw)
            if (args.labels is None) == (args.sweep is None):
                self.error("exactly one of --labels and --sweep")
            if args.sweep is not None:
                lo, hi = args.sweep
                if lo < 2 or hi < lo:
                    self.error("--sweep LO HI needs 2 <= LO <= HI")
                if hi - lo + 1 > MAX_SWEEP:
                    self.error("--sweep runs at most %d values of K" % MAX_SWEEP)
            if not 1 <= args.max_iter <= MAX_ITER:
                self.error("--max-iter must be in 1 .. %d" % MAX_ITER)
            _check_tfd_flags(self, args)
            return args
    ap = Parser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    _add_shared_flags(ap)
    ap.add_argument("--labels", default=None, help="an .npz with one integer array per molecule, `<label-key>_<i>` [G]: the clustering to "
                                                    "score (what python -m agdiff_amd.clusters / .medoids / .ensemble / .picks wrote)")
    ap.add_argument("--label-key", default="cluster", help="the key of --labels: cluster (default), or owner for python -m agdiff_amd.picks")
    ap.add_argument("--sweep", type=int, nargs=2, metavar=("LO", "HI"), default=None,
                    help="no labels: run k-medoids for K = LO .. HI and keep the K with the highest mean silhouette")
    _add_tfd_flags(ap)
    ap.add_argument("--init", choices=("maxmin", "first"), default="maxmin", help="with --sweep: k-medoids' seeds (agdiff_amd.medoids)")
    ap.add_argument("--max-iter", type=int, default=32, help="with --sweep: at most this many updates per K (1 .. %d)" % MAX_ITER)
    return ap


def main(argv=None):
    """python -m agdiff_amd.silhouette --samples samples_all.npz --testset test.npz (--labels clusters.npz | --sweep 2 8) --out sil.npz
    Silhouette coefficients of a finished job's molecules (agdiff_amd.driver: `pos_gen_<i>`) under a clustering over the RMSD or
    TFD matrix.  --labels FILE: the clustering is `<label-key>_<i>` of FILE (one integer per conformer, -1 left out; default key
    `cluster`).  --sweep LO HI: k-medoids for every K in LO .. HI, and the K with the highest mean silhouette is kept.  Writes per
    molecule `sil_<i>`, `sil_a_<i>`, `sil_b_<i>` float64 [G] (NaN when left out), `sil_other_<i>` int32 [G] (the nearest other
    cluster's label; -1 for none), `sil_cluster_<i>` float64 [K] (the mean of each cluster, in ascending label order),
    `sil_mean_<i>` float64, `count_<i>` int32 [K] (+ `name_<i>`).  With --sweep also `sweep_k_<i>` int32 [n], `sweep_sil_<i>` and
    `sweep_cost_<i>` float64 [n], `best_k_<i>` int32 and, for that K, everything python -m agdiff_amd.medoids writes (`count_<i>`
    is the same array in both).  --fix-handedness, --fix-double-bonds, --drop-invalid, --drop-bent: as in python -m
    agdiff_amd.ensemble.  Prints the conformers scored, the mean silhouette over the molecules and, with --sweep, how often each
    K won."""
    args = _parser().parse_args(argv)
    metric = "tfd" if args.tfd else "rmsd"
    kw = dict(metric=metric, device=args.device, fix_handedness=args.fix_handedness, fix_double_bonds=args.fix_double_bonds,
              tfd_rings=args.tfd_rings)
    given = None if args.labels is None else np.load(args.labels)
    out, scored, means, wins = {}, 0, [], {}
    for mol, item, valid in _checked_items(sampled_items(args.testset, args.samples), args, out):
        i = mol["index"]
        if given is not None:
            key = "%s_%d" % (args.label_key, i)
            if key not in given.files:
                raise ValueError("--labels: %s has no %s" % (args.labels, key))
            sil = tail = silhouette_conformers(item, given[key], valid=valid, **kw)
        else:
            sweep = sweep_medoids(item, args.sweep[0], args.sweep[1], init=args.init, max_iter=args.max_iter, align=args.align,
                                  valid=valid, **kw)
            out["sweep_k_%d" % i], out["sweep_sil_%d" % i], out["sweep_cost_%d" % i] = sweep["k"], sweep["mean"], sweep["cost"]
            out["best_k_%d" % i] = np.int32(sweep["best_k"])
            wins[sweep["best_k"]] = wins.get(sweep["best_k"], 0) + 1
            if sweep["medoids"] is None:                 # too few conformers for LO clusters: nothing is scored
                everybody = _lib.conformers(item["pos_gen"], num_atoms(item)).shape[0]
                sil = tail = silhouette_conformers(item, np.full(everybody, -1), valid=valid, **kw)
            else:
                sil, tail = sweep["silhouette"], sweep["medoids"]
                _write_medoids(out, i, tail, "iters", count=False)     # (`count_<i>` is written below: the same array)
        for key, name in (("s", "sil"), ("a", "sil_a"), ("b", "sil_b"), ("other", "sil_other"), ("cluster_mean", "sil_cluster"),
                          ("count", "count")):
            out["%s_%d" % (name, i)] = sil[key].cpu().numpy()
        out["sil_mean_%d" % i] = np.float64(sil["mean"])
        _write_tail(out, mol, tail)
        scored += int(out["count_%d" % i].sum())
        if not np.isnan(sil["mean"]):
            means.append(sil["mean"])
    np.savez_compressed(args.out, **out)
    print("silhouette of %d conformers by %s (%s): mean over %d molecules %.4f%s"
          % (scored, "TFD" if args.tfd else "RMSD",
             "labels %s of %s" % (args.label_key, args.labels) if given is not None else "k-medoids for K = %d .. %d, %s seeds" % (
                 args.sweep[0], args.sweep[1], args.init),
             len(means), float(np.mean(means)) if means else float("nan"),
             "" if given is not None else "; best K: " + ", ".join("%d x K = %d" % (wins[k], k) for k in sorted(wins))))
    return out


if __name__ == "__main__":
    main()
