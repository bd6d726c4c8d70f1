"""A diverse subset of a molecule's sampled conformers, of a given size -- "give me exactly 10 conformers that span what was sampled",
for a docking run, a QM refinement or a shape screen with a budget: MaxMin picking (farthest-point sampling, what rdkit's
MaxMinPicker is used for) over the float RMSD or TFD matrix.

Everything runs on the GPU (csrc/eval.hip), and there is no CPU fallback:
    agdiff_rmsd_self / agdiff_tfd_matrix   the symmetry-aware float matrix
    agdiff_maxmin_pick                     the walk over that matrix, one workgroup
    agdiff_align_conformers                Kabsch superposition of the picks

The rule (include/agdiff_hip.h): pick 0 is given; after every pick each conformer's distance to its nearest pick is updated (a strict
<, so on ties a conformer stays with the EARLIER pick); the next pick is the conformer farthest from all picks -- ties to the
LOWEST index -- as long as fewer than k are picked and that distance is above the stop threshold.  The distance at which each
pick was taken is the k-centre covering radius before it: how many conformers cover the ensemble to within r is read off `radius`.
ensemble.prune_conformers and clusters.cluster_conformers take a threshold and return however many conformers it leaves; this
takes the count.  Agreement with rdkit's MaxMinPicker is not claimed: that one draws its first pick at random.

    python -m agdiff_amd.picks --samples out/samples_all.npz --testset test.npz (--count K and/or --radius T) [--tfd] [--tfd-rings]
                               [--first I] [--align] [--fix-handedness] [--fix-double-bonds] [--drop-invalid] [--drop-bent]
                               --out picks.npz
"""
import numpy as np

from . import _lib
from .ensemble import (_add_shared_flags, _add_tfd_flags, _attach, _check_tfd_flags, _checked_items, _chosen, _own, _scatter,
                       _usable_matrix, _write_tail)
from .molecule import check_threshold, sampled_items


def maxmin_pick(dist, G, k, stop=-1.0, first=0):
    """agdiff_maxmin_pick on a float32 matrix [G, G] on the GPU: (picks int32 [k], radius float32 [k], owner int32 [G], near
    float32 [G], n_picked int32 [1], cover float32 [1]) -- the picks in order (-1 from n_picked on), the distance at which each
    was taken (+inf for pick 0, NaN from n_picked on), the rank of every conformer's nearest pick and the distance to it (-1 and
    NaN for a conformer the matrix marks as unusable), the number of picks, and the covering radius they leave.  A negative
    `stop` is no threshold.  More than AGDIFF_PRUNE_MAX_CONFS conformers: AgdiffLimitError."""
    import torch
    _lib.require_device_table(dist, "dist must be a contiguous float32 tensor [G, G] on the GPU")
    if tuple(dist.shape) != (G, G):
        raise ValueError("dist must be [%d, %d] (got %s)" % (G, G, tuple(dist.shape)))
    dev = dist.device
    picks = torch.empty(k, dtype=torch.int32, device=dev)
    radius = torch.empty(k, dtype=torch.float32, device=dev)
    owner = torch.empty(G, dtype=torch.int32, device=dev)
    near = torch.empty(G, dtype=torch.float32, device=dev)
    n_picked = torch.empty(1, dtype=torch.int32, device=dev)
    cover = torch.empty(1, dtype=torch.float32, device=dev)
    _lib.call("agdiff_maxmin_pick", dist, int(G), int(k), int(first), float(stop), picks, radius, owner, near, n_picked, cover)
    return picks, radius, owner, near, n_picked, cover


def pick_conformers(item, k=None, radius=None, metric="rmsd", first=None, align=True, device="cuda", valid=None, fix_handedness=False,
                    fix_double_bonds=False, tfd_rings=False):
    """MaxMin picking among the item's generated conformers by their best RMSD (metric="tfd": their torsion fingerprint deviation,
    agdiff_amd.torsions; the item must carry its bonds).  The item, `valid`, `fix_handedness` and `fix_double_bonds` are those of
    ensemble.prune_conformers, `tfd_rings` makes the rings terms of the TFD, and the fixes run first.  A conformer with a coordinate
    that is not finite is left out like one that `valid` masks.
        k       at most this many picks (clamped to the number of usable conformers)
        radius  stop once every usable conformer is within `radius` of a pick: a conformer is picked only while the farthest one
                is farther than that.  At least one of k and radius; radius alone picks until cover <= radius.
        first   pick 0, an index into the item's conformers; default: the first usable one.  A masked `first`: ValueError.
    Returns a dict of tensors on `device`, in the item's own conformer indices:
        picks   int32 [K']    the picks in pick order
        radius  float32 [K']  the distance from the picks before it at which each was taken (+inf for pick 0), non-increasing: the
                              covering radius of the first r picks is radius[r]
        owner   int32 [G]     the rank (index into picks) of every conformer's nearest pick, the earlier one on ties; -1 when masked
        near    float32 [G]   the distance to it as the matrix stores it, 0 for a pick; NaN when masked
        count   int32 [K']    the conformers each pick owns, itself included
        cover   float         the covering radius of all K' picks: every usable conformer is within it of a pick
        pos     [K', n, 3]    the picks; with align=True superposed on pick 0 over the heavy atoms (that one is returned as it is,
                              bit for bit)
        hand, ez_state        as prune_conformers returns them, when the fixes ran
    With no usable conformer the K'-sized tensors are empty, `owner` is all -1 and `cover` is 0.  At most AGDIFF_PRUNE_MAX_CONFS
    conformers."""
    import torch
    if k is None and radius is None:
        raise ValueError("at least one of k and radius must be given")
    if k is not None and (int(k) != k or k < 1):
        raise ValueError("k must be a count of at least 1 (got %r)" % (k,))
    stop = -1.0 if radius is None else check_threshold(radius, "RMSD")

    def check_first(G, mask, why):
        if first is None:
            return
        if int(first) != first or not 0 <= first < G:
            raise ValueError("first must be the index of a conformer, 0 .. %d (got %r)" % (G - 1, first))
        if mask is not None and not mask[int(first)]:
            raise ValueError("first = %d is a conformer %s" % (first, why))
    m = _usable_matrix(item, "pick_conformers", metric, device, valid, fix_handedness, fix_double_bonds, tfd_rings, check=check_first)
    if m.G == 0:                                         # no conformer to pick from: all masked out
        none = lambda dtype: torch.empty(0, dtype=dtype, device=m.gen.device)
        return _attach(m, {"picks": none(torch.int32), "radius": none(torch.float32), "owner": _scatter(m, none(torch.int32), -1),
                           "near": _scatter(m, none(torch.float32), float("nan")), "count": none(torch.int32), "cover": 0.0,
                           "pos": m.gen[:0]})
    start = 0 if first is None else (int(first) if m.mask is None else int(m.mask[:int(first)].sum()))
    limit = m.G if k is None else min(int(k), m.G)
    picks, rad, owner, near, n_picked, cover = maxmin_pick(m.out, m.G, limit, stop=stop, first=start)
    n = int(n_picked.item())
    picks, rad = picks[:n], rad[:n]
    pos = _chosen(m, picks, align)
    count = torch.bincount(owner[owner >= 0].long(), minlength=n).to(torch.int32)
    return _attach(m, {"picks": _own(m, picks), "radius": rad, "owner": _scatter(m, owner, -1),
                       "near": _scatter(m, near, float("nan")), "count": count, "cover": float(cover.item()), "pos": pos})


def _parser():
    import argparse

    class Parser(argparse.ArgumentParser):
        def parse_args(self, *a, **kw):                  # (an "at least one of" group: argparse has only "exactly one of")
            args = super().parse_args(*a, **kw)
            if args.count is None and args.radius is None:
                self.error("at least one of --count and --radius is required")
            _check_tfd_flags(self, args)
            return args
    ap = Parser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    _add_shared_flags(ap)
    ap.add_argument("--count", type=int, default=None, help="pick at most this many conformers per molecule")
    ap.add_argument("--radius", type=float, default=None,
                    help="stop once every conformer is within this distance of a pick (Angstrom of heavy-atom RMSD; with --tfd a TFD "
                         "in [0, 1]); with --count, whichever comes first")
    _add_tfd_flags(ap)
    ap.add_argument("--first", type=int, default=None, help="the conformer picked first (default: the first one that is not left out)")
    return ap


def main(argv=None):
    """python -m agdiff_amd.picks --samples samples_all.npz --testset test.npz (--count K and/or --radius T) [--tfd] [--align] --out picks.npz
    Picks a diverse subset of a finished job's conformers (agdiff_amd.driver: `pos_gen_<i>`), MaxMin over the RMSD or TFD matrix.
    The bonds come from the test set, so the molecules' symmetry is honoured.  Writes per molecule `pick_<i>` [K'] (pick order),
    `radius_<i>` [K'] (the distance at which each pick was taken; +inf for the first), `owner_<i>` [G] (the rank of the nearest
    pick; -1 when left out), `near_<i>` [G] (the distance to it; NaN when left out), `count_<i>` [K'], `cover_<i>` (the covering
    radius of the picks), `pos_<i>` [K', n, 3] (+ `name_<i>`).  At least one of --count / --radius.  --fix-handedness,
    --fix-double-bonds, --drop-invalid, --drop-bent: as in python -m agdiff_amd.ensemble, with the same `hand_<i>`, `ez_state_<i>`,
    `valid_<i>` and `flat_<i>`.  Prints the conformers, the picks and the largest covering radius over the molecules."""
    args = _parser().parse_args(argv)
    metric = "tfd" if args.tfd else "rmsd"
    if args.radius is not None:
        check_threshold(args.radius, "RMSD")
    out, total, picked, covers = {}, 0, 0, []
    for mol, item, valid in _checked_items(sampled_items(args.testset, args.samples), args, out):
        i = mol["index"]
        res = pick_conformers(item, k=args.count, radius=args.radius, metric=metric, first=args.first, align=args.align,
                              device=args.device, valid=valid, fix_handedness=args.fix_handedness,
                              fix_double_bonds=args.fix_double_bonds, tfd_rings=args.tfd_rings)
        out["pick_%d" % i] = res["picks"].cpu().numpy()
        for key in ("radius", "owner", "near", "count", "pos"):
            out["%s_%d" % (key, i)] = res[key].cpu().numpy()
        out["cover_%d" % i] = np.float32(res["cover"])
        _write_tail(out, mol, res)
        total += int(res["owner"].shape[0])
        picked += int(res["picks"].shape[0])
        covers.append(res["cover"])
    np.savez_compressed(args.out, **out)
    print("picked %d of %d conformers by %s (%s); largest covering radius over the molecules: %.3f"
          % (picked, total, "TFD" if args.tfd else "RMSD",
             ", ".join(([] if args.count is None else ["at most %d per molecule" % args.count])
                       + ([] if args.radius is None else ["until within %.3f" % args.radius])),
             max(covers) if covers else 0.0))
    return out


if __name__ == "__main__":
    main()
