"""The family tree of a molecule's sampled ensemble: agglomerative (hierarchical) linkage clustering over the float RMSD or TFD
matrix -- what people who cluster conformers by RMSD mostly do (scipy.cluster.hierarchy.linkage on the RMSD matrix, then fcluster).
The other walks need a threshold (ensemble, clusters) or a count (picks, medoids, pam) BEFORE they run; a tree answers all thresholds
and all counts at once: any cut of it is a clustering, the clusterings of a sweep over K are nested, the merge heights show where
the natural gaps are, and the leaf order is the row order of the usual clustered RMSD heat map.

Everything runs on the GPU (csrc/eval.hip), and there is no CPU fallback:
    agdiff_rmsd_self / agdiff_tfd_matrix   the symmetry-aware float matrix
    agdiff_linkage                         the tree: two launches per merge (choose, update) over a uint64 square
    agdiff_linkage_cut                     a cut by count and / or height: labels, medoids and their sums
    agdiff_silhouette                      the sweep's scores
    agdiff_align_conformers                Kabsch superposition of the medoids

The rule (include/agdiff_hip.h): every conformer starts as a cluster, named by its lowest member; the two clusters with the
smallest key merge, ties to the LOWEST first slot, then to the lowest second; the key is the minimum ("single"), the maximum
("complete") or the mean ("average", UPGMA) of the distances between the two clusters' members.  Everything is made on the 2^-28
fixed-point image of the matrix that k-medoids uses: minima, maxima and sums are integers, and a mean is one correctly rounded
fp64 division, so a tree is exact and reproducible bit for bit.  A cut applies the merges in order while more than `count`
clusters remain and the merge height is <= `height`; each cluster's medoid is the member with the smallest summed distance to the
others (k-medoids' update), and `labels` goes to agdiff_amd.silhouette unchanged.

What this is not: no Ward, centroid or median linkage (the matrix is not Euclidean), no optimal leaf ordering, no driver flag.
Agreement with scipy.cluster.hierarchy.linkage is by the definition and on tie-free input only: its tie order is its own.  The
heights of "average" are not promised monotone above sums of 2^53 (one rounding): nothing here is defined through monotonicity.

    python -m agdiff_amd.linkage --samples out/samples_all.npz --testset test.npz (--count K | --height T | --sweep LO HI)
                                 [--method average|complete|single] [--tfd] [--tfd-rings] [--align] [--fix-handedness]
                                 [--fix-double-bonds] [--drop-invalid] [--drop-bent] --out tree.npz
"""
import numpy as np

from . import _lib
from .ensemble import (_add_shared_flags, _add_tfd_flags, _check_tfd_flags, _checked_items, _own, _scatter, _usable_matrix,
                       _write_tail)
from .medoids import _check_dist, _from_matrix, _result
from .molecule import as_host, sampled_items
from .silhouette import _check_sweep, _scored, silhouette

METHODS = ("single", "complete", "average")              # AGDIFF_LINKAGE_SINGLE, _COMPLETE, _AVERAGE
WORK_FIXED_BYTES = _lib.DEFINES["AGDIFF_LINKAGE_WORK_FIXED_BYTES"]
CUT_WORK_BYTES = _lib.DEFINES["AGDIFF_LINKAGE_CUT_WORK_BYTES"]
MAX_DIST = _lib.DEFINES["AGDIFF_KMEDOIDS_MAX_DIST"]
INF = float("inf")


def _method_code(method):
    if method not in METHODS:
        raise ValueError("method must be one of %s (got %r)" % (", ".join(map(repr, METHODS)), method))
    code = METHODS.index(method)
    assert _lib.DEFINES["AGDIFF_LINKAGE_" + method.upper()] == code
    return code


def _check_cut(count, height):
    """count >= 1; height +inf or a number in [0, AGDIFF_KMEDOIDS_MAX_DIST] as a float32: (int, float), or ValueError"""
    if isinstance(count, bool) or int(count) != count or count < 1:
        raise ValueError("count must be a count of at least 1 (got %r)" % (count,))
    try:
        h = float(np.float32(height))
    except (TypeError, ValueError):
        raise ValueError("height must be a number (got %r)" % (height,))
    if not (h == INF or 0.0 <= h <= MAX_DIST):
        raise ValueError("height must be +inf or a distance in 0 .. %d (got %r)" % (MAX_DIST, height))
    return int(count), h


def _new(dev, n, dtype):
    """an uninitialised tensor [n] on dev whose address is not null even for n == 0"""
    import torch
    return torch.empty(max(n, 1), dtype=dtype, device=dev)[:n]


def linkage(dist, G, method="average", anchor=0):
    """agdiff_linkage on a float32 matrix [G, G] on the GPU, of which only the strict upper triangle (and row `anchor`) is read:
    (left int32 [G], right int32 [G], height float64 [G], size int32 [G], order int32 [G], status int32 [1]) -- merge t joined the
    clusters named left[t] < right[t] (each by its lowest member) at height[t] into one of size[t] members that keeps the name
    left[t]; with M conformers that row `anchor` marks as usable there are M - 1 merges and the entries from M - 1 on are -1, -1,
    NaN, 0.  order[j] is conformer j's place in the tree's left-to-right leaf order, -1 when unusable.  status 0, or 2 (`anchor`
    outside 0 .. G - 1: an empty tree).  More than AGDIFF_PRUNE_MAX_CONFS conformers: AgdiffLimitError."""
    import torch
    code = _method_code(method)
    if isinstance(anchor, bool) or int(anchor) != anchor:
        raise ValueError("anchor must be a conformer index (got %r)" % (anchor,))
    _check_dist(dist, G)
    dev, G = dist.device, int(G)
    left, right, size, order = (_new(dev, G, torch.int32) for _ in range(4))
    height = _new(dev, G, torch.float64)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    work = torch.empty(G * G + WORK_FIXED_BYTES // 8, dtype=torch.int64, device=dev)
    _lib.call("agdiff_linkage", dist, G, code, int(anchor), left, right, height, size, order, status, work)
    return left, right, height, size, order, status


def cut_tree(dist, G, tree, count=1, height=INF):
    """agdiff_linkage_cut: the clustering that `tree` (what linkage returned for the same matrix) gives when its merges are applied
    in order while more than `count` clusters remain and the merge height is <= `height` (+inf: no bound; otherwise a distance in
    0 .. AGDIFF_KMEDOIDS_MAX_DIST, taken on the 2^-28 grid).  Returns k-medoids' tuple with n_clusters in n_iter's place:
    (medoids int32 [G], labels int32 [G], near float32 [G], size int32 [G], within float64 [G], cost float64 [1], n_clusters int32
    [1], status int32 [1]); the clusters are ranked by their lowest member, the arrays indexed by rank are filled up to n_clusters
    (then -1, 0, 0.0), each medoid is the member with the smallest summed distance to the other members (ties to the lowest index)
    and near, size, within and cost are relative to the medoids as agdiff_kmedoids has them.  status 0, or 2 (`tree` is not one)."""
    import torch
    count, h = _check_cut(count, height)
    _check_dist(dist, G)
    if len(tree) < 5:
        raise ValueError("tree must be what linkage returned: (left, right, height, size, order, ...)")
    left, right, hts, _, order = tree[:5]
    for t, dtype, what in ((left, torch.int32, "left"), (right, torch.int32, "right"), (hts, torch.float64, "height"),
                           (order, torch.int32, "order")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.dim() == 1 and t.is_contiguous() and t.shape[0] == G):
            raise ValueError("tree: %s must be a contiguous %s tensor [%d] on the GPU" % (what, str(dtype).replace("torch.", ""), G))
    dev, G = dist.device, int(G)
    medoids, labels, size = (_new(dev, G, torch.int32) for _ in range(3))
    near = _new(dev, G, torch.float32)
    within = _new(dev, G, torch.float64)
    cost = torch.empty(1, dtype=torch.float64, device=dev)
    n_clusters, status = (torch.empty(1, dtype=torch.int32, device=dev) for _ in range(2))
    work = torch.empty(CUT_WORK_BYTES // 8, dtype=torch.int64, device=dev)
    _lib.call("agdiff_linkage_cut", dist, G, left, right, hts, order, count, h, medoids, labels, near, size, within, cost, n_clusters,
              status, work)
    return medoids, labels, near, size, within, cost, n_clusters, status


def to_scipy(left, right, height, size, order):
    """A tree as scipy.cluster.hierarchy takes it, on the host: (Z float64 [M - 1, 4], leaves int64 [M]).  The M usable conformers
    (order >= 0) are the leaves 0 .. M - 1 in ascending conformer index and leaves[id] is the conformer; merge t makes the new
    cluster M + t; a row of Z holds the two ids that merged, the lower id first, the height and the size.  dendrogram(Z) draws
    it; fcluster(Z, ...) cuts it by scipy's own rules."""
    left, right, height, size, order = (as_host(x) for x in (left, right, height, size, order))
    leaves = np.flatnonzero(order >= 0).astype(np.int64)
    M = int(leaves.shape[0])
    Z = np.zeros((max(M - 1, 0), 4), dtype=np.float64)
    ident = {int(c): i for i, c in enumerate(leaves)}    # the id of the cluster that holds each live slot
    for t in range(M - 1):
        a, b = int(left[t]), int(right[t])
        lo, hi = sorted((ident[a], ident.pop(b)))
        Z[t] = (lo, hi, height[t], size[t])
        ident[a] = M + t
    return Z, leaves


def _tree_result(m, tree, cut, method, align):
    """linkage_conformers' dict from a tree and one cut of it over the usable conformers of the namespace m"""
    left, right, height, size, order, _ = tree
    K = int(cut[6].item())
    M = int((order >= 0).sum().item())
    res = _result(m, (cut[0][:K], cut[1], cut[2], cut[3][:K], cut[4][:K], cut[5], cut[6], cut[7]), None, align)
    res["n_clusters"] = res.pop("iters")
    del res["converged"]
    import torch
    n = max(M - 1, 0)
    res["merges"] = torch.stack([_own(m, left[:n]), _own(m, right[:n])], dim=1)
    res["heights"], res["merge_sizes"] = height[:n], size[:n]
    res["order"] = _scatter(m, order, -1)
    res["linkage"] = method
    return res


def _empty_result(m, method, align):
    """the result with no usable conformer: medoid_conformers' empty one and an empty tree"""
    import torch
    res = _from_matrix(m, 1, "first", None, 1, align)
    res["n_clusters"] = res.pop("iters")
    del res["converged"]
    dev = m.gen.device
    res["merges"] = torch.empty((0, 2), dtype=torch.int32, device=dev)
    res["heights"] = torch.empty(0, dtype=torch.float64, device=dev)
    res["merge_sizes"] = torch.empty(0, dtype=torch.int32, device=dev)
    res["order"] = torch.full((m.total,), -1, dtype=torch.int32, device=dev)
    res["linkage"] = method
    return res


def linkage_conformers(item, method="average", count=1, height=INF, metric="rmsd", align=True, device="cuda", valid=None,
                       fix_handedness=False, fix_double_bonds=False, tfd_rings=False):
    """The tree of the item's generated conformers by their best RMSD (metric="tfd": their torsion fingerprint deviation) and one
    cut of it.  The item, `valid`, the fixes, `tfd_rings` and `align` are those of medoids.medoid_conformers.
        method  "single", "complete" or "average" (UPGMA)
        count   the cut stops when this many clusters are left (1: only `height` stops it)
        height  the cut stops at the first merge above this distance (+inf: only `count` stops it); both defaults: one cluster
    Returns medoid_conformers' dict in the item's own conformer indices -- medoids, labels, near, count, population, within, cost,
    pos (the medoids, superposed on the first with align=True), hand / ez_state -- with `n_clusters` in `iters`' place and no
    `converged`, the clusters ranked by their lowest member, and the tree:
        merges       int32 [M - 1, 2]   the two clusters of every merge, each named by its lowest member; the union keeps the first
        heights      float64 [M - 1]    the merge heights (on the 2^-28 grid for single and complete)
        merge_sizes  int32 [M - 1]      the members after each merge
        order        int32 [G]          every conformer's place in the left-to-right leaf order; -1 when left out
        linkage      str                the method
    M is the number of usable conformers (with a distance to the first usable one that is a number in 0 .. 4096).  At most
    AGDIFF_PRUNE_MAX_CONFS conformers.  Not Ward, no optimal leaf ordering: see the module's docstring."""
    _method_code(method)
    count, height = _check_cut(count, height)
    m = _usable_matrix(item, "linkage_conformers", metric, device, valid, fix_handedness, fix_double_bonds, tfd_rings)
    if m.G == 0:
        return _empty_result(m, method, align)
    tree = linkage(m.out, m.G, method)
    return _tree_result(m, tree, cut_tree(m.out, m.G, tree, count, height), method, align)


def sweep_linkage(item, k_min, k_max, method="average", metric="rmsd", align=True, device="cuda", valid=None, fix_handedness=False,
                  fix_double_bonds=False, tfd_rings=False):
    """"How many families" from ONE tree: a cut at every K in k_min .. k_max, each scored by its mean silhouette, all on the device;
    the clusterings are nested.  2 <= k_min <= k_max, at most 64 values of K; k_max is clamped to the number of usable conformers.
    Returns silhouette.sweep_medoids' dict without `iters` and `converged`: k int32 [n], mean float64 [n], cost float64 [n] (the
    summed distance to the cuts' medoids), best_k (the highest mean, ties to the SMALLEST K, a NaN never wins; 0 when no K was run),
    `medoids` (linkage_conformers' result at best_k, the tree included; None when no K was run) and `silhouette`
    (silhouette_conformers' result for that cut)."""
    import torch
    _method_code(method)
    _check_sweep(k_min, k_max, "first", 1)
    m = _usable_matrix(item, "sweep_linkage", metric, device, valid, fix_handedness, fix_double_bonds, tfd_rings)
    tree, hi = None, 0
    if m.G >= k_min:
        tree = linkage(m.out, m.G, method)
        hi = min(int(k_max), int((tree[4] >= 0).sum().item()))
    ks = list(range(int(k_min), hi + 1))
    if not ks:
        none = lambda dtype: np.zeros(0, dtype=dtype)
        return {"k": none(np.int32), "mean": none(np.float64), "cost": none(np.float64), "best_k": 0, "medoids": None,
                "silhouette": None}
    cuts, scores = [], []
    for K in ks:                                         # nothing in this loop synchronises
        cuts.append(cut_tree(m.out, m.G, tree, count=K))
        scores.append(silhouette(m.out, m.G, cuts[-1][1], K))
    column = lambda rows, j: torch.cat([r[j] for r in rows]).cpu().numpy()
    mean, cost = column(scores, 6), column(cuts, 5)
    best = 0
    for j in range(1, len(ks)):                          # the highest mean, ties to the smallest K; a NaN never wins
        if mean[j] > mean[best] or (np.isnan(mean[best]) and not np.isnan(mean[j])):
            best = j
    K = ks[best]
    return {"k": np.array(ks, dtype=np.int32), "mean": mean, "cost": cost, "best_k": K,
            "medoids": _tree_result(m, tree, cuts[best], method, align),
            "silhouette": _scored(m, cuts[best][1], np.arange(K, dtype=np.int64))}


def _parser():
    import argparse

    class Parser(argparse.ArgumentParser):
        def parse_args(self, *a, **kw):
            args = super().parse_args(*a, **kw)
            if args.count is not None and args.count < 1:
                self.error("--count must be at least 1")
            if args.height is not None and not (args.height == INF or 0.0 <= args.height <= MAX_DIST):
                self.error("--height must be a distance in 0 .. %d (or inf)" % MAX_DIST)
            if args.sweep is not None:
                lo, hi = args.sweep
                if lo < 2 or hi < lo:
                    self.error("--sweep LO HI needs 2 <= LO <= HI")
                if hi - lo + 1 > 64:
                    self.error("--sweep runs at most 64 values of K")
            _check_tfd_flags(self, args)
            return args
    ap = Parser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    _add_shared_flags(ap)
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--count", type=int, default=None, help="cut the tree where this many clusters are left")
    how.add_argument("--height", type=float, default=None, help="cut the tree below the first merge above this distance")
    how.add_argument("--sweep", type=int, nargs=2, metavar=("LO", "HI"), default=None,
                     help="cut at every K = LO .. HI and keep the K with the highest mean silhouette")
    ap.add_argument("--method", choices=("average", "complete", "single"), default="average",
                    help="the distance of two clusters: the mean (UPGMA), the maximum or the minimum over their pairs")
    _add_tfd_flags(ap)
    return ap


def main(argv=None):
    """python -m agdiff_amd.linkage --samples samples_all.npz --testset test.npz (--count K | --height T | --sweep LO HI) [--method average|complete|single] [--tfd] [--align] --out tree.npz
    The family tree of a finished job's molecules (agdiff_amd.driver: `pos_gen_<i>`) over the RMSD or TFD matrix and one cut of it:
    where K clusters are left, below the first merge above T, or at the K of LO .. HI with the highest mean silhouette.  Writes
    python -m agdiff_amd.medoids' keys without `iters_<i>` / `converged_<i>` -- `medoid_<i>`, `cluster_<i>`, `dist_<i>`,
    `count_<i>`, `population_<i>`, `within_<i>`, `cost_<i>`, `pos_<i>` (+ `name_<i>`) -- so python -m agdiff_amd.silhouette
    --labels scores the file as it is; the tree: `merge_<i>` int32 [M - 1, 2], `height_<i>` float64 [M - 1], `merge_size_<i>`
    int32 [M - 1], `order_<i>` int32 [G] (-1 when left out), `linkage_<i>` (the method) and `leaves_<i>` int64 [M] (the conformers
    that are scipy's leaves 0 .. M - 1: linkage.to_scipy); with --sweep `sweep_k_<i>` int32 [n], `sweep_sil_<i>` float64 [n] and
    `best_k_<i>` int32.  The shared flags are those of python -m agdiff_amd.ensemble.  Prints the conformers, the clusters and the
    largest population of a cluster."""
    args = _parser().parse_args(argv)
    metric = "tfd" if args.tfd else "rmsd"
    kw = dict(method=args.method, metric=metric, align=args.align, device=args.device, fix_handedness=args.fix_handedness,
              fix_double_bonds=args.fix_double_bonds, tfd_rings=args.tfd_rings)
    out, total, found, top = {}, 0, 0, 0.0
    for mol, item, valid in _checked_items(sampled_items(args.testset, args.samples), args, out):
        i = mol["index"]
        if args.sweep is not None:
            sweep = sweep_linkage(item, args.sweep[0], args.sweep[1], valid=valid, **kw)
            out["sweep_k_%d" % i], out["sweep_sil_%d" % i] = sweep["k"], sweep["mean"]
            out["best_k_%d" % i] = np.int32(sweep["best_k"])
            res = sweep["medoids"]
            if res is None:                              # too few conformers for LO clusters: the whole tree, one cluster
                res = linkage_conformers(item, valid=valid, **kw)
        else:
            res = linkage_conformers(item, count=1 if args.count is None else args.count,
                                     height=INF if args.height is None else args.height, valid=valid, **kw)
        for key, name in (("medoids", "medoid"), ("labels", "cluster"), ("near", "dist"), ("count", "count"),
                          ("population", "population"), ("within", "within"), ("pos", "pos"), ("merges", "merge"),
                          ("heights", "height"), ("merge_sizes", "merge_size"), ("order", "order")):
            out["%s_%d" % (name, i)] = res[key].cpu().numpy()
        out["cost_%d" % i] = np.float64(res["cost"])
        out["linkage_%d" % i] = np.str_(res["linkage"])
        out["leaves_%d" % i] = np.flatnonzero(out["order_%d" % i] >= 0).astype(np.int64)
        _write_tail(out, mol, res)
        total += int(res["labels"].shape[0])
        found += int(res["medoids"].shape[0])
        top = max([top] + res["population"].cpu().tolist())
    np.savez_compressed(args.out, **out)
    how = ("%d per molecule" % args.count if args.count is not None else
           "cut at %g" % args.height if args.height is not None else "the best of K = %d .. %d by silhouette" % tuple(args.sweep))
    print("%d clusters of %d conformers by %s (%s linkage, %s); largest population of a cluster: %.3f"
          % (found, total, "TFD" if args.tfd else "RMSD", args.method, how, top))
    return out


if __name__ == "__main__":
    main()
