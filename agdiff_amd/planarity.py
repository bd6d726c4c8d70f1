"""Planarity of sampled conformers: bent aromatic rings, pyramidal sp2 centres, twisted double bonds.

agdiff_amd.validity judges a conformer by distances: bond lengths, 1-3 distances when references are given, contacts more than three
bonds apart.  A benzene ring folded into a boat, a carbonyl carbon left pyramidal and a C=C whose ends are twisted against each other
keep all of those legal, agdiff_relax_bounds alone knows no planes and can produce them (agdiff_relax_planar, below, holds both),
and the leader prune then keeps such a conformer as a cluster of its own because it is far from everything.  This module names the groups of atoms that must lie in one plane from the
bond types, and one kernel (csrc/eval.hip: agdiff_planar_groups; there is no CPU fallback) measures each group of each conformer:

  dev         the largest distance of a member from the group's best plane in Angstrom -- centroid c, y_k = x_k - c,
              A = (1 / m) sum y_k y_k^T, unit normal = the eigenvector of A's smallest eigenvalue, dev = (float32) max_k |normal . y_k|,
              all in float64 from the float32 coordinates; +inf when a member coordinate is not finite
  per conformer  flat_dev = max dev, flat_group = the lowest group attaining it (-1 without groups), n_bent = #{dev > thresh}
  flat        n_bent == 0; a molecule without groups is flat

The groups are THIS PROJECT'S rules, read from the bond types alone (planar_groups has them in full): the 5- and 6-membered cycles
of aromatic bonds (type 12), and every double bond (type 2) with the neighbours of its two ends.  There is no aromaticity perception
-- a ring written kekulised, as alternating single and double bonds, is seen through its double bonds only --, amide nitrogens are
not in any group unless a double bond puts them there, and conjugation is not followed.  check_planarity(groups=...) takes a
caller's own groups instead.

thresh = 0.25 Angstrom is this project's default; it is the figure the PoseBusters suite is recalled to use for its two flatness
tests (aromatic rings, double bonds).  Like validity.py's bounds it has not been run over GEOM's reference conformers: no
false-positive rate is claimed.  The check marks, and the prune can leave the marked ones out.

A bent conformer can also be flattened instead of dropped: agdiff_relax_planar (relax_planar, repair_planarity, --repair) is
agdiff_relax_bounds with the planes of these groups as one more constraint type, in the same launch -- every member further than
flat_to = 0.10 Angstrom from its group's best plane is moved towards it while the bond lengths and contacts are held (a projection
onto a plane shortens bonds, so the flattening includes the distance repair), and a conformer that is valid and flat comes back
bit for bit.  Like the distance repair it is a projection from the topology alone, NOT MMFF: no energies, no torsion terms, no
electrostatics.  It does not choose E or Z: a double bond twisted past 90 degrees flattens into the other isomer, because nothing
here knows which one the molecule is -- unless --fix-double-bonds (agdiff_amd.ezbonds) ran first, which puts every tagged bridge
double bond on the right side of 90 degrees.

    python -m agdiff_amd.planarity --samples out/samples_all.npz --testset test.npz --out planarity.npz [--thresh 0.25] [--per-group]
                                   [--repair flattened.npz [--flat-to 0.10] [--pad 0.02] [--omega 1.0] [--max-iter 200]]
"""
import numpy as np

from . import _lib
from .molecule import as_host, bonded_neighbours, bonds_of, field, num_atoms, sampled_items

MAX_ATOMS = _lib.DEFINES["AGDIFF_PLANAR_MAX_ATOMS"]
MAX_GROUPS = _lib.DEFINES["AGDIFF_FLATTEN_MAX_GROUPS"]            # of relax_planar; the check itself has no limit
AROMATIC, DOUBLE = 12, 2                  # bond types
KIND_RING, KIND_DOUBLE = 0, 1


def _aromatic_rings(adj):
    """sorted atom tuples of every simple cycle of 5 or 6 atoms in the subgraph of aromatic bonds; each cycle is walked from its
    lowest atom through higher ones only, and two cycles over the same atoms are one group"""
    aro = [sorted(j for j, ty in nb.items() if ty == AROMATIC) for nb in adj]
    rings = set()
    for s in range(len(adj)):
        stack = [(s, (s,))]
        while stack:
            at, path = stack.pop()
            for j in aro[at]:
                if j == s and len(path) in (5, 6):
                    rings.add(tuple(sorted(path)))
                elif j > s and j not in path and len(path) < 6:
                    stack.append((j, path + (j,)))
    return sorted(rings)


def planar_groups(item):
    """(grp_ptr int32 [P + 1], grp_idx int32 [grp_ptr[P]], grp_kind int8 [P]): the groups of atoms of the item (atom_type [n] atomic
    numbers and its bonds; types 1 .. 21 are bonds, the 2- and 3-hop entries are ignored) that must lie in one plane, as a CSR with
    every group's atoms ascending.

      kind 0, aromatic ring   every simple cycle of 5 or 6 atoms in the subgraph of bonds of type 12; the members are the ring atoms.
                              Naphthalene gives its two 6-rings and not the 10-atom envelope, an indole-like system one 5-ring and
                              one 6-ring.
      kind 1, double bond     for every bond of type 2 between u < v: {u, v} and the bonded neighbours of both, kept when both ends
                              have at most 3 bonded neighbours (sulfones and phosphates are out), every end with more than one
                              neighbour is C or N (a sulfoxide S is out, a terminal O or S is fine) and the group has at least 4
                              atoms (a C=O without its carbon's other neighbours gives nothing).  Alkenes (6 atoms), carbonyls,
                              imines and nitro groups (4 atoms), allenes (one group per double bond).

    Rings first and then double bonds, each in the order of their sorted atom tuples: the group index is deterministic.  No group has
    more than AGDIFF_PLANAR_MAX_ATOMS = 8 atoms.

    These are this project's rules, from the bond types alone.  There is NO aromaticity perception on kekulised input: a ring drawn as
    alternating bonds of type 1 and 2 is seen through its double bonds only (benzene: three 6-atom groups, no ring group).  There are
    NO amide nitrogens: the N of an amide and its substituents are in no group unless a double bond starts at it.  There is NO
    conjugation: a diene is two separate groups."""
    n = num_atoms(item)
    z = np.asarray(field(item, "atom_type")).reshape(-1)
    adj = bonded_neighbours(n, *bonds_of(item))
    groups = [(g, KIND_RING) for g in _aromatic_rings(adj)]
    doubles = []
    for u in range(n):
        for v, ty in adj[u].items():
            if ty != DOUBLE or v < u:
                continue
            if any(len(adj[e]) > 3 or (len(adj[e]) > 1 and int(z[e]) not in (6, 7)) for e in (u, v)):
                continue
            members = tuple(sorted({u, v} | set(adj[u]) | set(adj[v])))
            if len(members) >= 4:
                doubles.append(members)
    groups += [(g, KIND_DOUBLE) for g in sorted(doubles)]
    assert all(len(g) <= MAX_ATOMS for g, _ in groups)
    grp_ptr = np.zeros(len(groups) + 1, dtype=np.int32)
    grp_ptr[1:] = np.cumsum([len(g) for g, _ in groups])
    grp_idx = np.array([a for g, _ in groups for a in g], dtype=np.int32)
    return grp_ptr, grp_idx, np.array([k for _, k in groups], dtype=np.int8)


def check_groups(n, grp_ptr, grp_idx):
    """(grp_ptr int32 [P + 1], grp_idx int32) as writable contiguous copies, checked on the host: grp_ptr starts at 0, ascends and ends
    at len(grp_idx), every group has 3 .. AGDIFF_PLANAR_MAX_ATOMS members, every member lies in [0, n).  Anything else: ValueError."""
    ptr, idx = as_host(grp_ptr), as_host(grp_idx)
    if ptr.ndim != 1 or idx.ndim != 1 or ptr.dtype.kind not in "iu" or (idx.size and idx.dtype.kind not in "iu"):
        raise ValueError("grp_ptr and grp_idx must be one-dimensional integer arrays")
    ptr, idx = ptr.astype(np.int64), idx.astype(np.int64)
    if ptr.shape[0] < 1 or ptr[0] != 0 or ptr[-1] != idx.shape[0]:
        raise ValueError("grp_ptr must be [P + 1], start at 0 and end at len(grp_idx) = %d" % idx.shape[0])
    size = np.diff(ptr)
    if (size < 3).any() or (size > MAX_ATOMS).any():
        raise ValueError("grp_ptr must ascend by 3 .. %d atoms per group (AGDIFF_PLANAR_MAX_ATOMS)" % MAX_ATOMS)
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError("grp_idx names atoms outside [0, %d)" % n)
    return ptr.astype(np.int32), idx.astype(np.int32)


def _threshold(thresh):
    th = float(thresh)
    if not (th >= 0.0 and np.isfinite(th)):
        raise ValueError("the planarity threshold must be finite and >= 0 (got %r)" % (thresh,))
    return th


def planar_deviation(pos, grp_ptr, grp_idx, thresh=0.25, want_dev=False):
    """agdiff_planar_groups on pos [G, n, 3] (float32, contiguous, on the GPU): (worst float32 [G], worst_group int32 [G], n_bent
    int32 [G], dev float32 [G, P] or None) as tensors on the device.  The tables (numpy or tensors) are checked here, on the host
    (check_groups): the kernel trusts grp_ptr."""
    import torch
    _lib.require_device_conformers(pos)
    G, n = int(pos.shape[0]), int(pos.shape[1])
    if n == 0:
        raise ValueError("conformers without atoms")
    th = _threshold(thresh)
    ptr, idx = check_groups(n, grp_ptr, grp_idx)
    P = ptr.shape[0] - 1
    dev = pos.device
    worst = torch.empty(G, dtype=torch.float32, device=dev)
    worst_group, n_bent = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(2))
    table = torch.empty((G, P), dtype=torch.float32, device=dev) if want_dev else None
    if G:
        pt, it = ((torch.from_numpy(x).to(dev) if P else None) for x in (ptr, idx))
        _lib.call("agdiff_planar_groups", pos, pt, it, G, n, P, th, table if (table is not None and table.numel()) else None, worst,
                  worst_group, n_bent)
    return worst, worst_group, n_bent, table


def _groups_of(item, groups):
    """(grp_ptr, grp_idx, grp_kind) of an item: planar_groups(item), or the caller's own (grp_ptr, grp_idx[, grp_kind]) checked"""
    if groups is None:
        return planar_groups(item)
    if len(groups) not in (2, 3):
        raise ValueError("groups must be (grp_ptr, grp_idx) or (grp_ptr, grp_idx, grp_kind)")
    ptr, idx = check_groups(num_atoms(item), groups[0], groups[1])
    kind = np.full(ptr.shape[0] - 1, -1, dtype=np.int8) if len(groups) == 2 else as_host(groups[2], np.int8).reshape(-1)
    if kind.shape[0] != ptr.shape[0] - 1:
        raise ValueError("%d groups but %d kinds" % (ptr.shape[0] - 1, kind.shape[0]))
    return ptr, idx, kind


def check_planarity(item, thresh=0.25, groups=None, device="cuda", want_dev=False):
    """The planarity check over the item's generated conformers (atom_type [n], pos_gen, and its bonds: edge_index + edge_type or
    bond_index + bond_type).  groups: None (planar_groups(item)) or the caller's own (grp_ptr, grp_idx) -- optionally with a third
    entry, one kind per group; without it the kinds come back as -1.  thresh in Angstrom.  Returns a dict:
        flat       bool [G]       n_bent == 0 (a molecule without groups is flat)
        flat_dev   float32 [G]    the largest distance of an atom from its group's best plane (+inf: a coordinate that is not finite)
        flat_group int32 [G]      the group with that distance, -1 when there are no groups
        n_bent     int32 [G]      groups with dev > thresh
        groups     (grp_ptr, grp_idx, grp_kind) numpy, on the host
        dev        float32 [G, P] with want_dev: every group's distance
    The four per-conformer entries and dev are tensors on `device`."""
    th = _threshold(thresh)
    n = num_atoms(item)
    ptr, idx, kind = _groups_of(item, groups)
    pos = _lib.conformers(item["pos_gen"], n, device)
    worst, worst_group, n_bent, dev = planar_deviation(pos, ptr, idx, th, want_dev=want_dev)
    res = {"flat": n_bent == 0, "flat_dev": worst, "flat_group": worst_group, "n_bent": n_bent, "groups": (ptr, idx, kind)}
    if want_dev:
        res["dev"] = dev
    return res


def membership_csr(n, grp_ptr, grp_idx):
    """(mb_ptr int32 [n + 1], mb_grp int32 [len(grp_idx)]): the groups of (grp_ptr, grp_idx) by atom -- row i holds the groups that
    contain atom i, ascending (a group that names an atom twice appears twice in its row), q_i = mb_ptr[i + 1] - mb_ptr[i].  The
    second table of agdiff_relax_planar; the groups go through check_groups first."""
    n = int(n)
    ptr, idx = check_groups(n, grp_ptr, grp_idx)
    grp = np.repeat(np.arange(ptr.shape[0] - 1, dtype=np.int64), np.diff(ptr))
    order = np.argsort(idx, kind="stable")              # (by atom; stable: the groups of an atom stay ascending)
    mb_ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(mb_ptr, idx.astype(np.int64) + 1, 1)
    return np.cumsum(mb_ptr).astype(np.int32), grp[order].astype(np.int32)


def _flatten_params(thresh, flat_to, pad):
    """(thresh, flat_to) as floats; ValueError unless both are finite and >= 0 and flat_to + pad <= thresh as the C ABI carries them"""
    th = _threshold(thresh)
    ft = float(flat_to)
    if not (ft >= 0.0 and np.isfinite(ft)):
        raise ValueError("flat_to must be finite and >= 0 (got %r)" % (flat_to,))
    if float(np.float32(ft)) + float(np.float32(pad)) > float(np.float32(th)):
        raise ValueError("need flat_to + pad <= thresh, so that a repaired group passes the check (got %r + %r > %r)" % (flat_to, pad, thresh))
    return th, ft


def relax_planar(pos, grp_ptr, grp_idx, pairs, lo, hi, radius, ex_ptr, ex_idx, thresh=0.25, flat_to=0.10, clash=0.60, pad=0.02, omega=1.0,
                 max_iter=200):
    """agdiff_relax_planar on pos [G, n, 3] (float32, contiguous, on the GPU): validity.relax_bounds with the planes of the groups
    (grp_ptr, grp_idx) as one more constraint type, in one launch.  Every conformer that fails pair_bounds, clash_scan or
    planar_deviation at `thresh` has its atoms moved by small steps until every bounded distance and every contact is inside
    relax_bounds' targets and every member of every group is within flat_to of its group's best plane (to within half a pad), or
    max_iter updates are spent.  Not MMFF: no energies, no torsions, no electrostatics; E or Z is not chosen -- a double bond
    twisted past 90 degrees flattens into the other isomer, unless ezbonds.fix_double_bonds (--fix-double-bonds) ran first
    (include/agdiff_hip.h has the rule).  Returns what
    relax_bounds returns: (pos_out, status int32 [G]: 0 valid and flat as it came and unchanged bit for bit, 1 repaired, 2 not within
    max_iter updates, 3 not finite and unchanged; iters; resid; moved).  All tables are checked here, on the host (check_groups,
    validity.relax_tables; flat_to + pad <= thresh): ValueError before any launch.  More than AGDIFF_RELAX_MAX_ATOMS atoms or
    AGDIFF_FLATTEN_MAX_GROUPS groups: AgdiffLimitError.  Without groups the results are relax_bounds'."""
    import torch
    from .validity import relax_tables
    _lib.require_device_conformers(pos)
    G, n = int(pos.shape[0]), int(pos.shape[1])
    bd_ptr, bd_idx, bd_lo, bd_hi, rad, ptr, idx, K = relax_tables(n, pairs, lo, hi, radius, ex_ptr, ex_idx, clash, pad, omega)
    th, ft = _flatten_params(thresh, flat_to, pad)
    g_ptr, g_idx = check_groups(n, grp_ptr, grp_idx)
    mb_ptr, mb_grp = membership_csr(n, g_ptr, g_idx)
    P = g_ptr.shape[0] - 1
    dev = pos.device
    pos_out = torch.empty_like(pos)
    status, iters = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(2))
    resid, moved = (torch.empty(G, dtype=torch.float32, device=dev) for _ in range(2))
    if G:
        up = lambda x: torch.from_numpy(x).to(dev) if x.size else None
        grp = [up(x) if P else None for x in (g_ptr, g_idx, mb_ptr, mb_grp)]
        _lib.call("agdiff_relax_planar", pos, torch.from_numpy(bd_ptr).to(dev), up(bd_idx), up(bd_lo), up(bd_hi), up(rad), up(ptr), up(idx),
                  *grp, G, n, K, P, float(clash), float(pad), float(omega), int(max_iter), th, ft, pos_out, status, iters, resid, moved)
    return pos_out, status, iters, resid, moved


def repair_planarity(item, groups=None, bounds="table", thresh=0.25, flat_to=0.10, clash=0.60, pad=0.02, omega=1.0, max_iter=200,
                     device="cuda", **table_kw):
    """relax_planar over the item's generated conformers: the groups check_planarity judges (planar_groups(item), or the caller's
    `groups`) and the tables validity.check_geometry builds from the item (the same `bounds`, `clash` and keywords).  The conformers
    either check calls broken are flattened and moved into their bounds, the others come back bit for bit.  Not MMFF.  Returns the
    dict validity.repair_geometry returns: pos float32 [G, n, 3], status int32 [G] (0 valid and flat as sampled, 1 repaired, 2 not
    repaired within max_iter updates, 3 not finite), iters int32 [G], resid float32 [G], moved float32 [G], tensors on `device`."""
    from .validity import _tables
    ptr, idx, _ = _groups_of(item, groups)
    pairs, lo, hi, radius, ex_ptr, ex_idx = _tables(item, bounds, table_kw)
    pos = _lib.conformers(item["pos_gen"], num_atoms(item), device)
    out = relax_planar(pos, ptr, idx, pairs, lo, hi, radius, ex_ptr, ex_idx, thresh=thresh, flat_to=flat_to, clash=clash, pad=pad,
                       omega=omega, max_iter=max_iter)
    return dict(zip(("pos", "status", "iters", "resid", "moved"), out))


def main(argv=None):
    """python -m agdiff_amd.planarity --samples samples_all.npz --testset test.npz --out planarity.npz [--thresh 0.25] [--per-group]
    Checks every molecule of a finished job (agdiff_amd.driver: `pos_gen_<i>`; the bonds come from the test set).  Writes per molecule
    `flat_<i>` int8 [G], `flat_dev_<i>` float32 [G], `flat_group_<i>` int32 [G], `n_bent_<i>` int32 [G] (+ `name_<i>`); with
    --per-group also `planar_dev_<i>` float32 [G, P] and the groups `planar_ptr_<i>`, `planar_idx_<i>`, `planar_kind_<i>` (0 an
    aromatic ring, 1 a double bond with its neighbours).
    --repair FLATTENED.npz: every molecule's conformers first go through repair_planarity (the table bounds, --thresh; --flat-to, --pad,
    --omega, --max-iter); FLATTENED.npz is a copy of the samples file with every `pos_gen_<i>` repaired plus `repair_status_<i>` int8 [G]
    and `repair_moved_<i>` float32 [G], and --out holds the verdicts on the repaired conformers.  Not MMFF: a projection onto the planes
    and the distance bounds."""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", required=True)
    ap.add_argument("--testset", required=True)
    ap.add_argument("--thresh", type=float, default=0.25,
                    help="distance from the best plane in Angstrom above which a group is bent (this project's default)")
    ap.add_argument("--per-group", action="store_true", help="also write every group's distance and the groups themselves")
    ap.add_argument("--out", required=True)
    ap.add_argument("--repair", default=None, metavar="FLATTENED.npz",
                    help="flatten the bent conformers and move the invalid ones into their bounds first (repair_planarity; not MMFF) and "
                         "write the samples file with the repaired pos_gen_<i>, repair_status_<i> and repair_moved_<i> here; --out then "
                         "judges the repaired ones")
    ap.add_argument("--flat-to", type=float, default=0.10,
                    help="--repair: the distance from its plane a repaired atom is aimed at (Angstrom); --flat-to + --pad <= --thresh")
    ap.add_argument("--pad", type=float, default=0.02, help="--repair: how far inside its limits a repaired distance is aimed (Angstrom)")
    ap.add_argument("--omega", type=float, default=1.0, help="--repair: the step's relaxation factor, in (0, 2)")
    ap.add_argument("--max-iter", type=int, default=200, help="--repair: most updates per conformer")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if not (args.thresh >= 0.0 and np.isfinite(args.thresh)):
        ap.error("--thresh must be finite and >= 0")
    if args.repair:
        if not (args.pad > 0.0 and np.isfinite(args.pad)) or not 0.0 < args.omega < 2.0 or args.max_iter < 1:
            ap.error("--pad must be finite and > 0, --omega in (0, 2) and --max-iter >= 1")
        if not (args.flat_to >= 0.0 and np.isfinite(args.flat_to)) or np.float32(args.flat_to) + np.float32(args.pad) > np.float32(args.thresh):
            ap.error("--flat-to must be finite and >= 0, and --flat-to + --pad <= --thresh")
    out, mols, confs, bent, by_ring, by_double = {}, 0, 0, 0, 0, 0
    repaired, fixed, stuck = None, 0, 0
    if args.repair:
        with np.load(args.samples, allow_pickle=False) as zs:
            repaired = {k: zs[k] for k in zs.files}
    for mol, item in sampled_items(args.testset, args.samples):
        i = mol["index"]
        if repaired is not None:
            rep = repair_planarity(item, thresh=args.thresh, flat_to=args.flat_to, pad=args.pad, omega=args.omega, max_iter=args.max_iter,
                                   device=args.device)
            status = rep["status"].cpu().numpy()
            item["pos_gen"] = rep["pos"].cpu().numpy().reshape(np.shape(repaired["pos_gen_%d" % i]))
            repaired["pos_gen_%d" % i] = item["pos_gen"]
            repaired["repair_status_%d" % i] = status.astype(np.int8)
            repaired["repair_moved_%d" % i] = rep["moved"].cpu().numpy()
            fixed += int((status == 1).sum())
            stuck += int((status == 2).sum())
        res = check_planarity(item, thresh=args.thresh, device=args.device, want_dev=True)
        ptr, idx, kind = res["groups"]
        dev = res["dev"].cpu().numpy()
        out["flat_%d" % i] = res["flat"].cpu().numpy().astype(np.int8)
        for k in ("flat_dev", "flat_group", "n_bent"):
            out["%s_%d" % (k, i)] = res[k].cpu().numpy()
        out["name_%d" % i] = np.str_(mol["name"])
        if args.per_group:
            out["planar_dev_%d" % i], out["planar_ptr_%d" % i], out["planar_idx_%d" % i], out["planar_kind_%d" % i] = dev, ptr, idx, kind
        over = dev > np.float32(args.thresh)             # (the kernel's comparison: fp32 against fp32; NaN is not over)
        mols += 1
        confs += over.shape[0]
        bent += int(over.any(1).sum())
        by_ring += int(over[:, kind == KIND_RING].any(1).sum())
        by_double += int(over[:, kind == KIND_DOUBLE].any(1).sum())
    np.savez_compressed(args.out, **out)
    if repaired is not None:
        np.savez_compressed(args.repair, **repaired)
        print("%d conformers were repaired, %d were not within %d updates; the verdicts are on the repaired conformers"
              % (fixed, stuck, args.max_iter))
    print("%d molecules, %d conformers, %d bent (%d with an aromatic ring out of plane, %d with a double bond out of plane)"
          % (mols, confs, bent, by_ring, by_double))
    return out


if __name__ == "__main__":
    main()
