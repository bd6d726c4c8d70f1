"""Conformer ensembles -- the step after the sampler: prune the 2 x num_refs raw conformers of a molecule to the ones that
differ (RDKit's EmbedMultipleConfs(pruneRmsThresh=...) rule) and superpose what is kept (AlignMolConformers).

Everything runs on the GPU (csrc/eval.hip), and there is no CPU fallback:
    agdiff_rmsd_self         gen x gen symmetry-aware RMSD, every pair once (upper-triangular tiles), with the adjacency
                             under the threshold as a bit-matrix
    agdiff_leader_prune      the greedy leader walk over that bit-matrix, in conformer order
    agdiff_align_conformers  Kabsch superposition that writes coordinates

Items are the plain dicts of agdiff_amd.evaluation: atom_type [n], pos_gen [G*n, 3] or [G, n, 3], and optionally the bonds
(bond_index + bond_type, or edge_index + edge_type) or perms [P, m] -- with them the RMSD is the minimum over the molecule's
heavy-atom self-matches (GetBestRMS), without them the identity mapping only.  Hydrogens take no part in the RMSD and ride
along in the alignment.

    python -m agdiff_amd.ensemble --samples out/samples_all.npz --testset test.npz --prune-rms 0.5 [--align] [--fix-handedness]
                                  [--drop-invalid] [--drop-bent] --out pruned.npz
    (--prune-tfd 0.2 in --prune-rms's place: the same walk over the torsion fingerprint deviation, agdiff_amd.torsions)
"""
import numpy as np

from . import _lib
from .evaluation import selection_of, selection_on_device
from .molecule import as_host, check_threshold, heavy_atoms, num_atoms, sampled_items
from .planarity import check_planarity
from .ezbonds import fix_double_bonds as _fix_double_bonds
from .stereo import fix_handedness as _fix_handedness
from .validity import check_geometry

MAX_CONFS = _lib.DEFINES["AGDIFF_PRUNE_MAX_CONFS"]


def bits_pitch(G):
    """Bytes per row of the threshold bit-matrix of G conformers: 16-bit pieces, rounded up to 8 bytes."""
    return ((((G + 15) // 16) * 2 + 7) // 8) * 8


def _self_rmsd(item, device, threshold=None, want_out=True):
    """(gen [G, n, 3] on the device, heavy index tensor, out [G, G] or None, bits int64 [G, pitch / 8] or None)"""
    import torch
    at, idx, P, pt = selection_on_device(item, device)
    n, m = at.shape[0], idx.shape[0]
    gen = _lib.conformers(item["pos_gen"], n, device)
    G = gen.shape[0]
    out = torch.empty((G, G), dtype=torch.float32, device=device) if want_out else None
    bits = None
    if threshold is not None:
        bits = torch.empty((G, bits_pitch(G) // 8), dtype=torch.int64, device=device)
    scratch = torch.empty(max(G, 1) * (3 * m + 1), dtype=torch.float32, device=device)
    _lib.call("agdiff_rmsd_self", gen, idx, pt, G, n, m, P, 0.0 if threshold is None else threshold, scratch, out, bits)
    return gen, idx, out, bits


def self_rmsd_matrix(item, device="cuda"):
    """The [G, G] matrix of best RMSDs between the item's generated conformers (float32 tensor on `device`): what
    evaluation.get_rmsd_confusion_matrix gives with pos_ref = pos_gen, each pair computed once -- exactly symmetric, zero
    diagonal.  The mirror is exact when the mappings form a group (heavy_atom_automorphisms does; so must `perms`)."""
    return _self_rmsd(item, device)[2]


def threshold_bits(item, threshold, device="cuda"):
    """(out [G, G], adjacency bool [G, 8 * pitch]): the matrix and the kernel's packed `out <= threshold`, unpacked (columns
    from G on are padding)."""
    t = check_threshold(threshold, "RMSD")
    gen, _, out, bits = _self_rmsd(item, device, threshold=t)
    return out, unpack_bits(bits, gen.shape[0])


def unpack_bits(bits, G):
    """bool [G, 8 * pitch] from the packed rows (int64 [G, pitch / 8]; little-endian: bit c of byte b = column 8 b + c)."""
    import torch
    by = bits.view(torch.uint8).reshape(G, -1).to(torch.int32)
    sh = torch.arange(8, device=bits.device, dtype=torch.int32)
    return ((by[:, :, None] >> sh[None, None, :]) & 1).reshape(G, -1).bool()


def leader_prune(bits, G):
    """agdiff_leader_prune on a packed bit-matrix (int64 [G, pitch / 8] on the GPU): (keep, leader, count, n_kept) int32.
    More than AGDIFF_PRUNE_MAX_CONFS conformers: AgdiffLimitError."""
    import torch
    dev = bits.device
    keep, leader, count = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(3))
    n_kept = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("agdiff_leader_prune", bits, G, keep, leader, count, n_kept)
    return keep, leader, count, n_kept


def _align(pos, idx, target):
    import torch
    G, n = pos.shape[0], pos.shape[1]
    out = torch.empty_like(pos)
    rmsd = torch.empty(G, dtype=torch.float32, device=pos.device)
    _lib.call("agdiff_align_conformers", pos, idx, target, G, n, int(idx.shape[0]), out, rmsd)
    return out, rmsd


def align_conformers(pos, atom_type, target, device="cuda"):
    """Superpose every conformer of pos [G, n, 3] (or [G*n, 3]) on target [n, 3] over the heavy atoms, atoms keeping their
    labels (rdkit AlignMolConformers): proper rotation + translation, applied to all atoms.  Returns (aligned [G, n, 3],
    rmsd [G]: the heavy-atom RMSD to the target after alignment) as float32 tensors on `device`."""
    import torch
    n = np.asarray(atom_type).reshape(-1).shape[0]
    heavy = heavy_atoms(atom_type)
    p = _lib.conformers(pos, n, device)
    t = _lib.conformers(target, n, device)
    if t.shape[0] != 1:
        raise ValueError("target must be one conformer [n, 3]")
    return _align(p, torch.from_numpy(heavy).to(device), t[0])


def _valid_mask(valid, G):
    """bool numpy [G] from a bool mask (numpy or tensor); anything else is a ValueError, before any launch"""
    v = as_host(valid)
    if v.dtype != np.bool_ or v.shape != (G,):
        raise ValueError("valid must be a bool mask with one entry per conformer: [%d] (got %s %s)" % (G, v.dtype, tuple(v.shape)))
    return v


def _usable_matrix(item, what, metric, device, valid, fix_handedness, fix_double_bonds, tfd_rings, check=None, threshold=None,
                   want_out=True, finite_only=True):
    """What prune_conformers, clusters.cluster_conformers, picks.pick_conformers and medoids.medoid_conformers do before their
    walk: the argument checks (all before any device work), the item's conformers, the `valid` mask, the fixes (the caller's tensor
    is never written), the compaction to the usable conformers on the device, and their RMSD (metric="rmsd") or TFD matrix.
        what         the caller's name, for the messages
        check        check(G, mask, why): the caller's own checks of conformer indices against the item's G conformers and the
                     bool mask [G] (None: nothing masked); called once before any device work with why = "that valid masks out",
                     and again, with why = "with a coordinate that is not finite", when such conformers were masked
        threshold    not None (the threshold walks): checked, and the matrix maker also packs `matrix <= threshold` into `bits`
        want_out     the float matrix `out` is made
        finite_only  a conformer with a coordinate that is not finite is masked like one that `valid` masks, which costs one
                     synchronising read; False (the threshold walks): it reaches the matrix, +inf from everything, and nothing
                     synchronises before the matrix launch
    Returns a namespace: total (the item's conformers), G (the usable ones), mask (bool numpy [total] or None), sel (int64 tensor
    [G], the usable conformers' indices, or None when all are), gen [G, n, 3], idx (the heavy atoms), out [G, G] and bits (int64
    [G, pitch / 8]) or None as asked for (both None when G == 0, with gen the uncompacted conformers), hand, ez_state (as
    prune_conformers returns them, or None).  _chosen, _own, _scatter and _attach turn a walk's answer into the caller's result."""
    import types
    import torch
    if metric not in ("rmsd", "tfd"):
        raise ValueError("metric must be 'rmsd' or 'tfd' (got %r)" % (metric,))
    if tfd_rings and metric != "tfd":
        raise ValueError("tfd_rings goes with metric='tfd'")
    thr = None if threshold is None else check_threshold(threshold, "RMSD")
    gen = _lib.conformers(item["pos_gen"], num_atoms(item))
    G = total = gen.shape[0]
    if G == 0:
        raise ValueError("%s: the item has no conformers" % what)
    if G > MAX_CONFS:
        raise _lib.AgdiffLimitError("%s: %d conformers, more than AGDIFF_PRUNE_MAX_CONFS = %d" % (what, G, MAX_CONFS))
    mask = None if valid is None else _valid_mask(valid, G)
    if check is not None:
        check(G, mask, "that valid masks out")
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
    gen = gen.to(device).contiguous()
    if finite_only:                                      # a coordinate that is not finite: masked before the matrix is made
        finite = torch.isfinite(gen).reshape(G, -1).all(dim=1).cpu().numpy()
        if not finite.all():
            mask = finite if mask is None else mask & finite
            if check is not None:
                check(G, mask, "with a coordinate that is not finite")
    res = types.SimpleNamespace(total=total, G=G, mask=mask, sel=None, gen=gen, idx=None, out=None, bits=None, hand=hand,
                                ez_state=ez_state)
    if mask is not None:                                 # compacted on the device; the kernels see the usable ones only
        res.sel = torch.nonzero(torch.from_numpy(mask).to(gen.device), as_tuple=False).reshape(-1)
        res.G = int(res.sel.shape[0])
        if res.G == 0:
            return res
        gen = gen[res.sel].contiguous()
    if metric == "tfd":
        from .torsions import _self_tfd
        # (the keyword is passed only when set: without the switch _self_tfd gets, argument for argument, the call it got before)
        res.gen, res.out, res.bits = _self_tfd(dict(item, pos_gen=gen), device, threshold=thr, want_out=want_out,
                                               **({"rings": True} if tfd_rings else {}))
        res.idx = torch.from_numpy(selection_of({"atom_type": item["atom_type"]})[1]).to(device)
    else:
        res.gen, res.idx, res.out, res.bits = _self_rmsd(dict(item, pos_gen=gen), device, threshold=thr, want_out=want_out)
    return res


def _chosen(m, chosen, align):
    """The conformers `chosen` (indices among the usable ones of the namespace m, in the caller's order) [K, n, 3]; with `align`
    superposed on the first of them over the heavy atoms, and that one put back bit for bit.  None chosen: nothing is launched."""
    pos = m.gen[chosen.long()]
    if align and pos.shape[0] > 0:
        first = pos[0].clone()
        pos, _ = _align(pos.contiguous(), m.idx, first)
        pos[0] = first
    return pos


def _own(m, chosen):
    """indices among the usable conformers as int32 indices into the item's own conformers"""
    import torch
    return (chosen if m.sel is None else m.sel[chosen.long()]).to(torch.int32)


def _scatter(m, x, fill):
    """a tensor with one entry per usable conformer as one with an entry per conformer of the item [total], `fill` (-1, NaN) for
    the masked ones; x itself when nothing was masked"""
    import torch
    if m.sel is None:
        return x
    full = torch.full((m.total,), fill, dtype=x.dtype, device=x.device)
    full[m.sel] = x
    return full


def _attach(m, res):
    """res with `hand` and `ez_state` when the fixes ran"""
    if m.hand is not None:
        res["hand"] = m.hand
    if m.ez_state is not None:
        res["ez_state"] = m.ez_state
    return res


def prune_conformers(item, threshold, align=True, device="cuda", fix_handedness=False, metric="rmsd", fix_double_bonds=False,
                     valid=None):
    """RDKit's pruneRmsThresh rule over the item's generated conformers, in their order: a conformer is kept iff its best RMSD
    to every conformer kept before it is above `threshold`; a dropped one belongs to the first kept conformer within the
    threshold.  metric="tfd": the same leader walk with the torsion fingerprint deviation (agdiff_amd.torsions; in [0, 1], the item
    must carry its bonds) in the RMSD's place; alignment and the handedness fix work as for the RMSD.
    Returns a dict of tensors on `device`:
        kept   int32 [K]  indices of the kept conformers, ascending
        leader int32 [G]  for every conformer the kept conformer it belongs to (itself when kept)
        count  int32 [K]  size of each kept conformer's cluster (itself included)
        pos    [K, n, 3]  the kept conformers; with align=True superposed on the first of them over the heavy atoms (that one
                          is returned as it is, bit for bit)
    fix_handedness=True (the item carries `stereo` and its bonds): the conformers that are the mirror image of the tagged molecule are
    inverted through their centroid first (agdiff_amd.stereo.fix_handedness), so that the prune does not spend the kept set on two
    families that can never superpose; the dict also gets
        hand   int32 [G]  the verdict before the fix: -1 was mirrored, 0 matches neither hand and is left as it is, +1 was right
    and `pos` holds the mirrored coordinates.
    fix_double_bonds=True (the item carries `ez_quads`, `ez` and its bonds): after the handedness fix, the tagged double bonds of the
    wrong E/Z parity are turned over (agdiff_amd.ezbonds.fix_double_bonds), so that the kept set is not spent on the wrong isomer;
    the dict also gets
        ez_state int8 [G, D]  each bond's state before the fix: +1 right, -1 wrong, 0 undecided or untagged
    and `pos` holds the flipped coordinates.
    valid (bool [G], e.g. agdiff_amd.validity.check_geometry(item)["valid"]): the walk runs over the valid conformers only, in their
    order -- a broken conformer is far from everything, so without the mask the rule keeps every one of them.  `kept` still indexes
    the item's conformers, `leader` is -1 for an invalid one, and with no valid conformer `kept` is empty and nothing is aligned.
    At most AGDIFF_PRUNE_MAX_CONFS conformers."""
    import torch
    m = _usable_matrix(item, "prune_conformers", metric, device, valid, fix_handedness, fix_double_bonds, False,
                       threshold=threshold, want_out=False, finite_only=False)
    if m.G == 0:
        none = torch.empty(0, dtype=torch.int32, device=m.gen.device)
        return _attach(m, {"kept": none, "leader": _scatter(m, none, -1), "count": none.clone(), "pos": m.gen[:0]})
    keep, leader, count, _ = leader_prune(m.bits, m.G)
    kept = torch.nonzero(keep, as_tuple=False).reshape(-1)
    return _attach(m, {"kept": _own(m, kept), "leader": _scatter(m, _own(m, leader), -1), "count": count[kept],
                       "pos": _chosen(m, kept, align)})


def _add_shared_flags(ap):
    """the flags that python -m agdiff_amd.ensemble, .clusters, .picks and .medoids share"""
    ap.add_argument("--samples", required=True)
    ap.add_argument("--testset", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--align", action="store_true", help="superpose the conformers that are written on the first of them")
    ap.add_argument("--fix-handedness", action="store_true", help="invert the mirror-image conformers first (needs stereo_<i> in --testset)")
    ap.add_argument("--fix-double-bonds", action="store_true",
                    help="turn over the double bonds of the wrong E/Z parity first, after --fix-handedness (needs ez_quads_<i> and ez_<i> "
                         "in --testset: python -m agdiff_amd.ezbonds); also writes ez_state_<i> [G, D].  --drop-invalid and --drop-bent "
                         "judge the conformers as sampled, before the flip, which can bring the two sides of a bond into contact: the "
                         "driver's order (flip, repair, check) is the one to use when that matters")
    ap.add_argument("--drop-invalid", action="store_true",
                    help="leave the conformers with a bond out of bounds or a steric clash (agdiff_amd.validity) out; also writes "
                         "valid_<i> [G]")
    ap.add_argument("--drop-bent", action="store_true",
                    help="leave the conformers with an aromatic ring or a double bond out of plane (agdiff_amd.planarity) out; also "
                         "writes flat_<i> [G]")


def _add_tfd_flags(ap):
    """--tfd and --tfd-rings of python -m agdiff_amd.picks, .medoids, .pam and .silhouette (.clusters' --tfd takes a threshold)"""
    ap.add_argument("--tfd", action="store_true", help="the torsion fingerprint deviation (agdiff_amd.torsions) in the RMSD's place")
    ap.add_argument("--tfd-rings", action="store_true",
                    help="with --tfd: the rings are terms of the TFD too (agdiff_amd.rings): chair and boat are far apart")


def _check_tfd_flags(ap, args):
    """the parser's check of those two flags once they are parsed"""
    if args.tfd_rings and not args.tfd:
        ap.error("--tfd-rings goes with --tfd")


def _checked_items(items, args, out):
    """The per-molecule block of those four command lines over the (mol, item) pairs of a module's sampled_items: the test set's
    `stereo` / `ez_quads` + `ez` go into the item when the fixes are asked for (a test set without them: ValueError), --drop-invalid
    and --drop-bent judge the conformers and write `valid_<i>` / `flat_<i>` int8 [G] into `out`.  Yields (mol, item, valid), valid
    the AND of the two masks or None."""
    for mol, item in items:
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
            valid = check_geometry(item, device=args.device)["valid"]       # (mirroring keeps every distance: before or after the fix)
            out["valid_%d" % i] = valid.cpu().numpy().astype(np.int8)
        if args.drop_bent:
            flat = check_planarity(item, device=args.device)["flat"]       # (mirroring keeps every plane too)
            out["flat_%d" % i] = flat.cpu().numpy().astype(np.int8)
            valid = flat if valid is None else valid & flat
        yield mol, item, valid


def _write_tail(out, mol, res):
    """`name_<i>` and, when the fixes ran, `hand_<i>` and `ez_state_<i>` int8 of a molecule's result, into `out`"""
    i = mol["index"]
    out["name_%d" % i] = np.str_(mol["name"])
    for key in ("hand", "ez_state"):
        if key in res:
            out["%s_%d" % (key, i)] = res[key].cpu().numpy().astype(np.int8)


def main(argv=None):
    """python -m agdiff_amd.ensemble --samples samples_all.npz --testset test.npz --prune-rms 0.5 [--align] --out pruned.npz
    Prunes a finished job's output (agdiff_amd.driver: `pos_gen_<i>`).  The bonds come from the test set, so the molecules'
    symmetry is honoured.  Writes per molecule `pos_<i>` [K, n, 3], `kept_<i>` [K], `cluster_<i>` [G], `count_<i>` [K]
    (+ `name_<i>`).  Exactly one of --prune-rms / --prune-tfd T (the torsion fingerprint deviation, in [0, 1]).  --fix-handedness: the mirror images are inverted before the matrix (the test set must carry `stereo_<i>`:
    python -m agdiff_amd.stereo); also writes `hand_<i>` [G], the verdict before the fix.  --fix-double-bonds: then the double bonds of
    the wrong E/Z parity are turned over (the test set must carry `ez_quads_<i>` / `ez_<i>`: python -m agdiff_amd.ezbonds); also
    writes `ez_state_<i>` [G, D], each bond's state before the fix.  --drop-invalid: the conformers that fail
    agdiff_amd.validity.check_geometry (table bounds, default clash ratio) take no part in the walk: `cluster_<i>` is -1 for them;
    also writes `valid_<i>` int8 [G].  --drop-bent: the same for the conformers that fail agdiff_amd.planarity.check_planarity (an
    aromatic ring or a double bond out of plane, default threshold); also writes `flat_<i>` int8 [G]."""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    _add_shared_flags(ap)
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--prune-rms", type=float, default=None, help="RMSD threshold in Angstrom (heavy atoms)")
    how.add_argument("--prune-tfd", type=float, default=None,
                     help="torsion fingerprint deviation threshold in [0, 1] (agdiff_amd.torsions) instead of an RMSD")
    args = ap.parse_args(argv)
    metric, threshold = ("rmsd", args.prune_rms) if args.prune_tfd is None else ("tfd", args.prune_tfd)
    check_threshold(threshold, "RMSD")
    out, total, left = {}, 0, 0
    for mol, item, valid in _checked_items(sampled_items(args.testset, args.samples), args, out):
        i = mol["index"]
        res = prune_conformers(item, threshold, align=args.align, device=args.device, fix_handedness=args.fix_handedness,
                               metric=metric, valid=valid, fix_double_bonds=args.fix_double_bonds)
        out["pos_%d" % i] = res["pos"].cpu().numpy()
        out["kept_%d" % i] = res["kept"].cpu().numpy()
        out["cluster_%d" % i] = res["leader"].cpu().numpy()
        out["count_%d" % i] = res["count"].cpu().numpy()
        _write_tail(out, mol, res)
        total += int(res["leader"].shape[0])
        left += int(res["kept"].shape[0])
    np.savez_compressed(args.out, **out)
    if metric == "tfd":
        print("pruned %d conformers to %d at TFD %.3f" % (total, left, threshold))
    else:
        print("pruned %d conformers to %d at %.3f A" % (total, left, args.prune_rms))
    return out


if __name__ == "__main__":
    main()
