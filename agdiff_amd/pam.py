"""K representative conformers of a molecule's sampled ensemble that do not depend on seeds: PAM (Kaufman & Rousseeuw), a greedy
BUILD that needs no seeds and a steepest-descent SWAP that tries every (medoid, non-medoid) exchange, so that a medoid can leave
its cluster altogether.  agdiff_amd.medoids is the alternating walk, whose result changes with its seeds; this one costs a pass
over the matrix per swap and ends at a cost that is usually several per cent lower, and always at a fixed point of that walk.

Everything runs on the GPU (csrc/eval.hip), and there is no CPU fallback:
    agdiff_rmsd_self / agdiff_tfd_matrix   the symmetry-aware float matrix
    agdiff_pam_build                       K medoids in rank order from nothing: two launches per rank
    agdiff_pam_swap                        the exchanges: three grid-wide launches per swap, the candidate's row streamed once
    agdiff_maxmin_pick / agdiff_kmedoids   the other seeds (init="maxmin", "alternate")
    agdiff_align_conformers                Kabsch superposition of the medoids

The rule (include/agdiff_hip.h): every exchange of a medoid of rank r for a candidate c changes the total cost by delta(c, r); an
iteration applies the smallest one (ties to the lowest candidate, then the lowest rank) while it is negative.  All sums are made
on the 2^-28 fixed-point image of the matrix, as in agdiff_amd.medoids, so the result is exact and bit-reproducible, and the
rule is memoryless: the swaps are made in chunks, with one 4-byte read of the status between chunks, and no chunk size shows in
the result.  `labels` goes to agdiff_amd.silhouette unchanged.

What this is not: FasterPAM's eager variant (several swaps per pass), CLARA / CLARANS sampling, k-means++ / LAB seeding.  There
is no switch for it in `silhouette --sweep` and no driver flag.  Agreement with any other package's PAM is by the definition only.

    python -m agdiff_amd.pam --samples out/samples_all.npz --testset test.npz --count K [--tfd] [--tfd-rings]
                             [--init build|maxmin|first|alternate] [--max-swaps N] [--align] [--fix-handedness]
                             [--fix-double-bonds] [--drop-invalid] [--drop-bent] --out pam.npz
"""
import numpy as np

from . import _lib
from .ensemble import _add_shared_flags, _add_tfd_flags, _check_tfd_flags, _checked_items, _usable_matrix, _write_tail
from .medoids import (MAX_ITER, _check_dist, _check_init, _explicit_seeds, _from_matrix, _outputs, _result, _seed_tensor,
                      _write_medoids, kmedoids)
from .molecule import sampled_items

MAX_SWAPS = _lib.DEFINES["AGDIFF_PAM_MAX_SWAPS"]
WORK_BYTES = _lib.DEFINES["AGDIFF_PAM_WORK_BYTES"]
INITS = ("build", "maxmin", "first", "alternate")


def pam_build(dist, G, k, anchor=0):
    """agdiff_pam_build on a float32 matrix [G, G] on the GPU: k medoids in rank order from nothing, among the conformers that row
    `anchor` marks as usable.  Returns kmedoids' tuple (medoids int32 [k], labels int32 [G], near float32 [G], size int32 [k],
    within float64 [k], cost float64 [1], n_swaps int32 [1] = 0, status int32 [1]): status 0, or 2 (k above the number of usable
    conformers, or `anchor` outside 0 .. G - 1: nothing was computed).  More than AGDIFF_PRUNE_MAX_CONFS conformers:
    AgdiffLimitError."""
    if int(k) != k or k < 1:
        raise ValueError("k must be a count of at least 1 (got %r)" % (k,))
    if int(anchor) != anchor:
        raise ValueError("anchor must be a conformer index (got %r)" % (anchor,))
    _check_dist(dist, G)
    outs = _outputs(dist, G, int(k), WORK_BYTES)
    _lib.call("agdiff_pam_build", dist, int(G), int(k), int(anchor), *outs)
    return outs[:8]


def pam_swap(dist, G, init, anchor=None, max_swaps=64):
    """agdiff_pam_swap on a float32 matrix [G, G] on the GPU from the seeds `init` (int32 tensor [K] on the GPU, the medoids of
    rank 0 .. K - 1): at most `max_swaps` (0 .. AGDIFF_PAM_MAX_SWAPS) steepest-descent exchanges.  `anchor`: the conformer whose
    row marks the usable ones; None: init[0], as kmedoids has it (one synchronising read).  Returns kmedoids' tuple with n_swaps
    in n_iter's place; status 0 (no exchange lowers the cost), 1 (max_swaps were made and nothing was looked for after the last)
    or 2 (a seed or the anchor out of range, a seed twice or unusable: nothing was computed).  Calling again with the returned
    medoids and the same anchor continues the same walk."""
    _check_init(init, at_least=1)
    if int(max_swaps) != max_swaps or not 0 <= max_swaps <= MAX_SWAPS:
        raise ValueError("max_swaps must be a count in 0 .. %d (got %r)" % (MAX_SWAPS, max_swaps))
    if anchor is not None and int(anchor) != anchor:
        raise ValueError("anchor must be a conformer index or None (got %r)" % (anchor,))
    K = int(init.shape[0])
    _check_dist(dist, G)
    outs = _outputs(dist, G, K, WORK_BYTES)
    if anchor is None:
        anchor = int(init[0].item())
    _lib.call("agdiff_pam_swap", dist, int(G), K, init, int(anchor), int(max_swaps), *outs)
    return outs[:8]


def pam_conformers(item, k, metric="rmsd", init="build", max_swaps=4096, chunk=64, align=True, device="cuda", valid=None,
                   fix_handedness=False, fix_double_bonds=False, tfd_rings=False):
    """PAM among the item's generated conformers by their best RMSD (metric="tfd": their torsion fingerprint deviation).  The
    item, `valid`, the fixes, `tfd_rings` and `align` are those of medoids.medoid_conformers.
        k          the number of medoids (clamped to the number of usable conformers)
        init       where the swaps start: "build", PAM's own greedy BUILD from nothing (the first usable conformer's row marks
                   the usable ones); "maxmin", "first" or a sequence of k distinct usable conformer indices, as medoid_conformers
                   has them; "alternate", what medoid_conformers ends at from MaxMin seeds, polished
        max_swaps  at most this many exchanges in all; 0: the assignment to the seeds (init="build": BUILD alone)
        chunk      the exchanges enqueued per call, 1 .. AGDIFF_PAM_MAX_SWAPS: one 4-byte read of the status follows each.  It
                   does not show in the result.
    Returns medoid_conformers' dict with `swaps` (the exchanges made) in `iters`' place, `converged` False when max_swaps were made
    and nothing was looked for after the last, and, with init="build", `build_cost`: the cost BUILD ended at."""
    if int(k) != k or k < 1:
        raise ValueError("k must be a count of at least 1 (got %r)" % (k,))
    if int(max_swaps) != max_swaps or max_swaps < 0:
        raise ValueError("max_swaps must be a count of at least 0 (got %r)" % (max_swaps,))
    if int(chunk) != chunk or not 1 <= chunk <= MAX_SWAPS:
        raise ValueError("chunk must be a count in 1 .. %d (got %r)" % (MAX_SWAPS, chunk))
    seeds, check_seeds = _explicit_seeds(init, k, INITS)
    m = _usable_matrix(item, "pam_conformers", metric, device, valid, fix_handedness, fix_double_bonds, tfd_rings, check=check_seeds)
    return _walk(m, k, init, seeds, max_swaps, chunk, align)


def _walk(m, k, init, seeds, max_swaps, chunk, align):
    """pam_conformers after its matrix: the seeds, the chunks of swaps and the result, from the namespace m of
    ensemble._usable_matrix.  `seeds`: the checked explicit seeds in the item's own numbering, or None when `init` is a name."""
    import torch
    if m.G == 0:                                         # no usable conformer: medoid_conformers' empty result
        res = _from_matrix(m, k, "first", None, 1, align)
        res["swaps"] = res.pop("iters")
        if init == "build":
            res["build_cost"] = 0.0
        return res
    G, out = m.G, m.out
    anchor, build_cost = 0, None                         # (the first usable conformer's row marks the usable ones)
    if seeds is None and init == "build":
        K = min(int(k), G)
        built = pam_build(out, G, K, anchor)
        if int(built[7].item()) == 2:
            raise ValueError("pam_conformers: fewer than %d conformers are usable together with conformer 0 (a distance to it that "
                             "is not a number >= 0 and <= %d)" % (K, _lib.DEFINES["AGDIFF_KMEDOIDS_MAX_DIST"]))
        med, build_cost = built[0], float(built[5].item())
    else:                                                # explicit seeds, the first K, or MaxMin seeds ("maxmin", "alternate")
        med, _ = _seed_tensor(m, k, init, seeds)
        if seeds is not None:
            anchor = int(med[0].item())
        elif init == "alternate":
            med = kmedoids(out, G, med, max_iter=MAX_ITER)[0]
    total = 0
    while True:                                          # (memoryless: the chunks are one walk)
        walked = pam_swap(out, G, med, anchor, min(int(chunk), int(max_swaps) - total))
        med, status = walked[0], int(walked[7].item())
        total += int(walked[6].item()) if status != 2 else 0
        if status != 1 or total >= max_swaps:
            break
    res = _result(m, walked[:6] + (torch.tensor([total], dtype=torch.int32), walked[7]), seeds, align)
    res["swaps"] = res.pop("iters")
    if build_cost is not None:
        res["build_cost"] = build_cost
    return res


def _parser():
    import argparse

    class Parser(argparse.ArgumentParser):
        def parse_args(self, *a, **kw):
            args = super().parse_args(*a, **kw)
            if args.count < 1:
                self.error("--count must be at least 1")
            if args.max_swaps < 0:
                self.error("--max-swaps must be at least 0")
            _check_tfd_flags(self, args)
            return args
    ap = Parser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    _add_shared_flags(ap)
    ap.add_argument("--count", type=int, required=True, help="the number of medoids per molecule")
    _add_tfd_flags(ap)
    ap.add_argument("--init", choices=INITS, default="build",
                    help="where the swaps start: PAM's BUILD, the first K MaxMin picks, the first K conformers that are not left out, "
                         "or what python -m agdiff_amd.medoids ends at from MaxMin seeds")
    ap.add_argument("--max-swaps", type=int, default=4096, help="at most this many exchanges (0: the seeds' assignment)")
    return ap


def main(argv=None):
    """python -m agdiff_amd.pam --samples samples_all.npz --testset test.npz --count K [--tfd] [--init build|maxmin|first|alternate] [--align] --out pam.npz
    K representative conformers of a finished job's molecules (agdiff_amd.driver: `pos_gen_<i>`) with their populations: PAM
    (BUILD + SWAP) over the RMSD or TFD matrix.  Writes python -m agdiff_amd.medoids' keys -- `medoid_<i>`, `cluster_<i>`,
    `dist_<i>`, `count_<i>`, `population_<i>`, `within_<i>`, `cost_<i>`, `converged_<i>`, `pos_<i>` (+ `name_<i>`) -- with
    `swaps_<i>` int32 in `iters_<i>`'s place and, with --init build, `build_cost_<i>` float64; python -m agdiff_amd.silhouette
    --labels scores the file as it is.  The shared flags are those of python -m agdiff_amd.ensemble.  Prints the conformers, the
    medoids, the swaps, the molecules that did not converge and the largest population of a medoid."""
    args = _parser().parse_args(argv)
    metric = "tfd" if args.tfd else "rmsd"
    out, total, found, swaps, open_, top = {}, 0, 0, 0, 0, 0.0
    for mol, item, valid in _checked_items(sampled_items(args.testset, args.samples), args, out):
        i = mol["index"]
        res = pam_conformers(item, args.count, metric=metric, init=args.init, max_swaps=args.max_swaps, align=args.align,
                             device=args.device, valid=valid, fix_handedness=args.fix_handedness,
                             fix_double_bonds=args.fix_double_bonds, tfd_rings=args.tfd_rings)
        _write_medoids(out, i, res, "swaps")
        if "build_cost" in res:
            out["build_cost_%d" % i] = np.float64(res["build_cost"])
        _write_tail(out, mol, res)
        total += int(res["labels"].shape[0])
        found += int(res["medoids"].shape[0])
        swaps += res["swaps"]
        open_ += 0 if res["converged"] else 1
        top = max([top] + res["population"].cpu().tolist())
    np.savez_compressed(args.out, **out)
    print("%d medoids of %d conformers by %s (%d per molecule, PAM from %s, %d swaps, at most %d per molecule; %d molecules did not "
          "converge); largest population of a medoid: %.3f" % (found, total, "TFD" if args.tfd else "RMSD", args.count, args.init,
                                                                swaps, args.max_swaps, open_, top))
    return out


if __name__ == "__main__":
    main()
