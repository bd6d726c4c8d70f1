"""Geometry validity of sampled conformers.

Every later stage asks of a conformer's geometry only that it is finite.  A diffusion sampler also produces conformers that are
finite and wrong -- a bond stretched to 2.5 A after a clip_local retry, two ring systems pushed through each other, a hydrogen on top
of a carbon five bonds away -- and the leader prune keeps exactly those, because a broken conformer is far from everything kept before
it.  The reference pipeline catches them with rdkit's sanitisation and its optional MMFF step; this project has neither, but it holds
what a topology-only check needs.  Two checks on the GPU (csrc/eval.hip; there is no CPU fallback):
    agdiff_pair_bounds   the distances of named atom pairs against [lo, hi]: bond lengths, and through the 1-3 distances bond angles
    agdiff_clash_scan    every pair i < j that is NOT 1, 2 or 3 bonds apart against a fraction of the sum of two radii

  d           |p_i - p_j|, every coordinate converted to float64 before the first subtraction
  violation   v = max(lo - d, d - hi, 0) in Angstrom on d rounded to float32; +inf when d is not finite or the pair names an atom
              outside the molecule.  Per conformer: worst = max v, the lowest pair attaining it, n_bad = #{v > 0}
  exclusions  every entry of type > 0 of the item's extended edge list (types 1 .. 21 bonds, 23 two-hop, 24 three-hop), as a
              symmetric CSR with ascending rows
  ratio       (float32)(d / (r_i + r_j)) over the pairs not excluded, 0 when d is not finite.  Per conformer: the smallest ratio
              (+inf when there is no pair), the lowest (i, j) attaining it, n_clash = #{ratio < clash}
  valid       n_bad == 0 and n_clash == 0

The defaults are this project's choices, not rdkit's: covalent radii of Cordero et al. 2008 for the table bounds (a bond is within
[0.72, 1.20] x (rc_i + rc_j): 0.72 admits C#N at 0.79 of the sum and C=O at 0.85, 1.20 every common single bond, all <= 1.02),
Bondi's van der Waals radii for the clash scan at clash = 0.60 of their sum (O...H 1.63 A, C...C 2.04 A, H...H 1.44 A -- below an
intramolecular hydrogen bond, so hydrogen bonds are not flagged).  Nobody has run them over GEOM's reference conformers: no
false-positive rate is claimed.

A conformer that fails can also be repaired instead of dropped: agdiff_relax_bounds (relax_bounds, repair_geometry, --repair) moves
its atoms by small steps until every bounded distance and every contact is back inside the limits the two checks test, and leaves a
valid conformer untouched bit for bit.  That is a projection onto distance bounds from the topology alone, NOT MMFF: no energies, no
torsion terms, no electrostatics; agdiff_amd.evaluation's use_force_field=True still raises.

    python -m agdiff_amd.validity --samples out/samples_all.npz --testset test.npz [--refs refs.npz] [--clash 0.6] --out validity.npz
                                  [--repair repaired.npz [--pad 0.02] [--omega 1.0] [--max-iter 200]]
"""
import numpy as np

from . import _lib
from .molecule import as_host, bonds_of, field, num_atoms, sampled_items

CLASH_SLICE = _lib.DEFINES["AGDIFF_CLASH_SLICE"]

COVALENT_RADII = {1: 0.31, 5: 0.84, 6: 0.76, 7: 0.71, 8: 0.66, 9: 0.57, 14: 1.11, 15: 1.07, 16: 1.05, 17: 1.02, 35: 1.20, 53: 1.39}
COVALENT_DEFAULT = 1.50
VDW_RADII = {1: 1.20, 5: 1.92, 6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 14: 2.10, 15: 1.80, 16: 1.80, 17: 1.75, 35: 1.85, 53: 1.98}
VDW_DEFAULT = 2.00


def covalent_radii(atom_type):
    """float64 [n]: Cordero 2008 by atomic number, COVALENT_DEFAULT for an element not in the table."""
    return np.array([COVALENT_RADII.get(int(a), COVALENT_DEFAULT) for a in np.asarray(atom_type).reshape(-1)], dtype=np.float64)


def vdw_radii(atom_type):
    """float32 [n]: Bondi by atomic number, VDW_DEFAULT for an element not in the table."""
    return np.array([VDW_RADII.get(int(a), VDW_DEFAULT) for a in np.asarray(atom_type).reshape(-1)], dtype=np.float32)


def _edges(n, edge_index, edge_type):
    """(i, j, type) int64 of the entries of type > 0, i != j, range-checked"""
    ei = np.asarray(edge_index).reshape(2, -1).astype(np.int64)
    et = np.asarray(edge_type).reshape(-1).astype(np.int64)
    if ei.shape[1] != et.shape[0]:
        raise ValueError("%d edges but %d edge types" % (ei.shape[1], et.shape[0]))
    sel = (et > 0) & (ei[0] != ei[1])
    i, j, t = ei[0][sel], ei[1][sel], et[sel]
    if i.size and (min(i.min(), j.min()) < 0 or max(i.max(), j.max()) >= n):
        raise ValueError("the edge list names atoms outside the molecule's %d atoms" % n)
    return i, j, t


def exclusions(n, edge_index, edge_type):
    """(ex_ptr int32 [n + 1], ex_idx int32): the pairs a clash scan leaves out, from EVERY entry of type > 0 of an extended edge list
    (1, 2 or 3 bonds apart when the list is extended to order 3, as the driver's test sets are) -- symmetrised, each row ascending,
    without duplicates or self entries."""
    n = int(n)
    i, j, _ = _edges(n, edge_index, edge_type)
    key = np.unique(np.concatenate([i * n + j, j * n + i]))
    rows, cols = key // max(n, 1), key % max(n, 1)
    ex_ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ex_ptr, rows + 1, 1)
    return np.cumsum(ex_ptr).astype(np.int32), cols.astype(np.int32)


def _check_exclusions(n, ex_ptr, ex_idx):
    ptr = np.asarray(ex_ptr)
    idx = np.asarray(ex_idx)
    if ptr.dtype != np.int32 or idx.dtype != np.int32 or ptr.ndim != 1 or idx.ndim != 1:
        raise ValueError("ex_ptr and ex_idx must be one-dimensional int32 arrays")
    if ptr.shape[0] != n + 1 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or ptr[-1] != idx.shape[0]:
        raise ValueError("ex_ptr must be [n + 1] = [%d], start at 0, not decrease and end at len(ex_idx)" % (n + 1))
    if idx.size == 0:
        return
    if idx.min() < 0 or idx.max() >= n:
        raise ValueError("ex_idx names atoms outside [0, %d)" % n)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    same_row = rows[1:] == rows[:-1]
    if (np.diff(idx.astype(np.int64))[same_row] <= 0).any():
        raise ValueError("every row of ex_idx must be strictly ascending (unsorted or repeated entry)")
    if (rows == idx).any():
        raise ValueError("ex_idx holds a self entry")
    if not np.array_equal(rows * n + idx, np.sort(idx.astype(np.int64) * n + rows)):
        raise ValueError("the exclusions are not symmetric")


def _bond_pairs(item, types):
    """sorted unique (i, j), i < j, of the item's edge entries whose type passes `types`; the item must carry bonds"""
    n = num_atoms(item)
    i, j, t = _edges(n, *bonds_of(item))
    sel = types(t)
    a, b = np.minimum(i[sel], j[sel]), np.maximum(i[sel], j[sel])
    key = np.unique(a * n + b)
    return np.stack([key // max(n, 1), key % max(n, 1)], axis=1).astype(np.int32).reshape(-1, 2)


def bounds_from_table(item, bond_lo=0.72, bond_hi=1.20):
    """(pairs int32 [K, 2], lo float32 [K], hi float32 [K]): one pair per bond of type 1 .. 21, i < j, in (i, j) order, bounded by
    bond_lo and bond_hi x the sum of the two covalent radii."""
    if not 0.0 <= float(bond_lo) <= float(bond_hi):
        raise ValueError("need 0 <= bond_lo <= bond_hi (got %r, %r)" % (bond_lo, bond_hi))
    pairs = _bond_pairs(item, lambda t: (t >= 1) & (t <= 21))
    rc = covalent_radii(item["atom_type"])
    s = rc[pairs[:, 0]] + rc[pairs[:, 1]]
    return pairs, (float(bond_lo) * s).astype(np.float32), (float(bond_hi) * s).astype(np.float32)


def bounds_from_references(item, slack=0.05):
    """(pairs, lo, hi) from the item's reference conformers `pos_ref` [R, n, 3]: the bonds and the two-hop entries (types 1 .. 21 and
    23; the 1-3 distances bound the bond angles), lo = (1 - slack) x the smallest and hi = (1 + slack) x the largest distance over
    the references.  Host work in float64."""
    if not 0.0 <= float(slack) < 1.0:
        raise ValueError("slack must be in [0, 1) (got %r)" % (slack,))
    if field(item, "pos_ref") is None:
        raise ValueError("the item carries no reference conformers (pos_ref)")
    n = num_atoms(item)
    ref = as_host(field(item, "pos_ref"), np.float64).reshape(-1, n, 3)
    if ref.shape[0] == 0 or not np.isfinite(ref).all():
        raise ValueError("pos_ref must hold at least one conformer and be finite")
    pairs = _bond_pairs(item, lambda t: ((t >= 1) & (t <= 21)) | (t == 23))
    d = np.sqrt(((ref[:, pairs[:, 0]] - ref[:, pairs[:, 1]]) ** 2).sum(-1))
    return pairs, ((1.0 - float(slack)) * d.min(0)).astype(np.float32), ((1.0 + float(slack)) * d.max(0)).astype(np.float32)


def pair_bounds(pos, pairs, lo, hi, want_dist=False):
    """agdiff_pair_bounds on pos [G, n, 3] (float32, contiguous, on the GPU): (worst float32 [G], worst_pair int32 [G], n_bad int32
    [G], dist float32 [G, K] or None).  pairs int32 [K, 2], lo / hi [K] (numpy or tensors; no NaN, lo <= hi).  A pair naming an atom
    outside [0, n) is allowed: its violation is +inf and nothing is read."""
    import torch
    _lib.require_device_conformers(pos)
    G, n = int(pos.shape[0]), int(pos.shape[1])
    if n == 0:
        raise ValueError("conformers without atoms")
    pr = as_host(pairs, np.int32).reshape(-1, 2)                        # (copies: the caller's arrays may be read-only)
    K = pr.shape[0]
    lo_, hi_ = (as_host(x, np.float32).reshape(-1) for x in (lo, hi))
    if lo_.shape[0] != K or hi_.shape[0] != K:
        raise ValueError("%d pairs but %d lower and %d upper bounds" % (K, lo_.shape[0], hi_.shape[0]))
    if K and not (lo_ <= hi_).all():
        raise ValueError("every pair needs lo <= hi (and neither may be NaN)")
    dev = pos.device
    worst = torch.empty(G, dtype=torch.float32, device=dev)
    worst_pair, n_bad = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(2))
    dist = torch.empty((G, K), dtype=torch.float32, device=dev) if want_dist else None
    if G:
        pt, lt, ht = ((torch.from_numpy(x).to(dev) if K else None) for x in (pr, lo_, hi_))
        _lib.call("agdiff_pair_bounds", pos, pt, lt, ht, G, n, K, dist if (dist is not None and dist.numel()) else None, worst,
                  worst_pair, n_bad)
    return worst, worst_pair, n_bad, dist


def clash_scan(pos, radius, ex_ptr, ex_idx, thresh, want_scratch=False):
    """agdiff_clash_scan on pos [G, n, 3] (float32, contiguous, on the GPU): (min_ratio float32 [G], min_pair int32 [G, 2], n_clash
    int32 [G]) (+ the call's scratch, int32 [G, S, 4], with want_scratch).  radius [n] finite and > 0; ex_ptr int32 [n + 1] / ex_idx
    int32 (numpy: `exclusions`) are checked here, on the host, for range, ascending rows and symmetry -- the kernel does not.  More than
    AGDIFF_MAX_ATOMS_LARGE atoms: AgdiffLimitError."""
    import torch
    _lib.require_device_conformers(pos)
    G, n = int(pos.shape[0]), int(pos.shape[1])
    if n == 0:
        raise ValueError("conformers without atoms")
    th = float(thresh)
    if not (th >= 0.0 and np.isfinite(th)):
        raise ValueError("the clash threshold must be finite and >= 0 (got %r)" % (thresh,))
    rad = as_host(radius, np.float32).reshape(-1)
    if rad.shape[0] != n or not (np.isfinite(rad).all() and (rad > 0).all()):
        raise ValueError("radius must hold %d finite numbers > 0" % n)
    ptr, idx = as_host(ex_ptr), as_host(ex_idx)
    _check_exclusions(n, ptr, idx)
    dev = pos.device
    S = (n + CLASH_SLICE - 1) // CLASH_SLICE
    scratch = torch.empty((G, S, 4), dtype=torch.int32, device=dev)
    min_ratio = torch.empty(G, dtype=torch.float32, device=dev)
    min_pair = torch.empty((G, 2), dtype=torch.int32, device=dev)
    n_clash = torch.empty(G, dtype=torch.int32, device=dev)
    rt, pt = torch.from_numpy(rad).to(dev), torch.from_numpy(np.array(ptr)).to(dev)
    it = torch.from_numpy(np.array(idx)).to(dev) if idx.size else None
    if G:
        _lib.call("agdiff_clash_scan", pos, rt, pt, it, G, n, th, scratch, min_ratio, min_pair, n_clash)
    return (min_ratio, min_pair, n_clash, scratch) if want_scratch else (min_ratio, min_pair, n_clash)


def bounds_csr(n, pairs, lo, hi):
    """(bd_ptr int32 [n + 1], bd_idx int32 [2K], bd_lo float32 [2K], bd_hi float32 [2K]): the tables of agdiff_relax_bounds -- every
    bounded pair once in the row of each of its two atoms (partner, lo, hi), within a row in the order of the pair list (a pair listed
    twice appears twice).  ValueError: a pair that names an atom outside [0, n) or one atom twice (there is nothing to move), lo > hi
    or a NaN bound."""
    n = int(n)
    pr = as_host(pairs, np.int32).reshape(-1, 2)
    K = pr.shape[0]
    lo_, hi_ = (as_host(x, np.float32).reshape(-1) for x in (lo, hi))
    if lo_.shape[0] != K or hi_.shape[0] != K:
        raise ValueError("%d pairs but %d lower and %d upper bounds" % (K, lo_.shape[0], hi_.shape[0]))
    if K and not (lo_ <= hi_).all():
        raise ValueError("every pair needs lo <= hi (and neither may be NaN)")
    if K and (pr.min() < 0 or pr.max() >= n):
        raise ValueError("a bounded pair names an atom outside the molecule's %d atoms" % n)
    if K and (pr[:, 0] == pr[:, 1]).any():
        raise ValueError("a bounded pair names one atom twice")
    rows = pr.reshape(-1).astype(np.int64)                              # a_0 b_0 a_1 b_1 ...: a stable sort keeps the list's order
    order = np.argsort(rows, kind="stable")
    bd_ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(bd_ptr, rows + 1, 1)
    return (np.cumsum(bd_ptr).astype(np.int32), pr[:, ::-1].reshape(-1)[order].astype(np.int32), np.repeat(lo_, 2)[order],
            np.repeat(hi_, 2)[order])


def relax_tables(n, pairs, lo, hi, radius, ex_ptr, ex_idx, clash=0.60, pad=0.02, omega=1.0):
    """Everything relax_bounds checks and builds on the host, before any launch: (bd_ptr, bd_idx, bd_lo, bd_hi, radius float32 [n],
    ex_ptr, ex_idx, K).  ValueError for what bounds_csr, clash_scan's radius and exclusion checks refuse, and for a clash that is not
    finite and >= 0, a pad that is not finite and > 0 or an omega outside (0, 2)."""
    n = int(n)
    if n <= 0:
        raise ValueError("conformers without atoms")
    if not (float(clash) >= 0.0 and np.isfinite(float(clash))):
        raise ValueError("the clash threshold must be finite and >= 0 (got %r)" % (clash,))
    if not (np.float32(pad) > 0.0 and np.isfinite(np.float32(pad))):
        raise ValueError("pad must be finite and > 0 (got %r)" % (pad,))
    if not 0.0 < np.float32(omega) < 2.0:
        raise ValueError("omega must lie in (0, 2) (got %r)" % (omega,))
    bd = bounds_csr(n, pairs, lo, hi)
    rad = as_host(radius, np.float32).reshape(-1)
    if rad.shape[0] != n or not (np.isfinite(rad).all() and (rad > 0).all()):
        raise ValueError("radius must hold %d finite numbers > 0" % n)
    ptr, idx = as_host(ex_ptr), as_host(ex_idx)
    _check_exclusions(n, ptr, idx)
    return bd + (rad, np.array(ptr), np.array(idx), bd[1].shape[0] // 2)


def relax_bounds(pos, pairs, lo, hi, radius, ex_ptr, ex_idx, clash=0.60, pad=0.02, omega=1.0, max_iter=200):
    """agdiff_relax_bounds on pos [G, n, 3] (float32, contiguous, on the GPU): every conformer that fails pair_bounds(pairs, lo, hi)
    or clash_scan(radius, exclusions, clash) has its atoms moved by small steps until every bounded distance is inside
    [lo + p, hi - p], p = min(pad, (hi - lo) / 2), and every pair not excluded at least clash x (r_i + r_j) + pad apart (to within
    half a pad), or max_iter updates are spent; omega in (0, 2) scales the step.  Not MMFF: no energies, no torsions, no
    electrostatics (include/agdiff_hip.h has the rule).  Returns (pos_out float32 [G, n, 3], status int32 [G]:
    0 valid as it came and unchanged bit for bit, 1 repaired, 2 not within max_iter updates, 3 not finite and unchanged;
    iters int32 [G]; resid float32 [G], what the stop rule last saw in Angstrom; moved float32 [G], the RMS displacement of the
    atoms).  The tables are checked here, on the host (relax_tables); more than AGDIFF_RELAX_MAX_ATOMS atoms: AgdiffLimitError."""
    import torch
    _lib.require_device_conformers(pos)
    G, n = int(pos.shape[0]), int(pos.shape[1])
    bd_ptr, bd_idx, bd_lo, bd_hi, rad, ptr, idx, K = relax_tables(n, pairs, lo, hi, radius, ex_ptr, ex_idx, clash, pad, omega)
    dev = pos.device
    pos_out = torch.empty_like(pos)
    status, iters = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(2))
    resid, moved = (torch.empty(G, dtype=torch.float32, device=dev) for _ in range(2))
    if G:
        up = lambda x: torch.from_numpy(x).to(dev) if x.size else None
        _lib.call("agdiff_relax_bounds", pos, torch.from_numpy(bd_ptr).to(dev), up(bd_idx), up(bd_lo), up(bd_hi), up(rad), up(ptr), up(idx),
                  G, n, K, float(clash), float(pad), float(omega), int(max_iter), pos_out, status, iters, resid, moved)
    return pos_out, status, iters, resid, moved


def _tables(item, bounds, table_kw):
    """(pairs, lo, hi, radius, ex_ptr, ex_idx) of an item: host work, and every ValueError an item can cause, before any launch"""
    n = num_atoms(item)
    b_idx, b_typ = bonds_of(item)                     # (an item without bonds: ValueError)
    if isinstance(bounds, str):
        if bounds == "table":
            pairs, lo, hi = bounds_from_table(item, **table_kw)
        elif bounds == "references":
            pairs, lo, hi = bounds_from_references(item, **table_kw)
        else:
            raise ValueError("bounds must be 'table', 'references' or (pairs, lo, hi) (got %r)" % (bounds,))
    else:
        if table_kw:
            raise ValueError("keyword arguments %s go with bounds='table' or 'references'" % sorted(table_kw))
        pairs, lo, hi = bounds
    return (pairs, lo, hi, vdw_radii(item["atom_type"])) + exclusions(n, b_idx, b_typ)


def check_geometry(item, bounds="table", clash=0.60, device="cuda", **table_kw):
    """Both checks over the item's generated conformers (atom_type [n], pos_gen, and its bonds: edge_index + edge_type extended to
    order 3, or bond_index + bond_type).  bounds: "table" (bounds_from_table; bond_lo / bond_hi as keywords), "references"
    (bounds_from_references, the item carries pos_ref; slack as a keyword) or (pairs, lo, hi).  clash: the fraction of the van der
    Waals sum below which a pair not excluded clashes.  Returns a dict of tensors on `device`:
        valid      bool [G]       n_bad == 0 and n_clash == 0
        bond_dev   float32 [G]    the worst violation of a bound in Angstrom (+inf: a distance that is not finite)
        bond_pair  int32 [G, 2]   the atoms of the pair with that violation, -1 when there are no bounded pairs
        n_bad      int32 [G]      violated pairs
        clash      float32 [G]    the smallest d / (rvdw_i + rvdw_j) over the pairs more than three bonds apart (+inf: none)
        clash_pair int32 [G, 2]   the atoms of that pair, -1 when there is none
        n_clash    int32 [G]      pairs below `clash`"""
    import torch
    pairs, lo, hi, radius, ex_ptr, ex_idx = _tables(item, bounds, table_kw)
    pos = _lib.conformers(item["pos_gen"], num_atoms(item), device)
    worst, worst_pair, n_bad, _ = pair_bounds(pos, pairs, lo, hi)
    min_ratio, min_pair, n_clash = clash_scan(pos, radius, ex_ptr, ex_idx, clash)
    pt = torch.from_numpy(as_host(pairs, np.int32).reshape(-1, 2)).to(pos.device)
    pt = torch.cat([pt, torch.full((1, 2), -1, dtype=torch.int32, device=pos.device)])      # (row -1 = K: no pair)
    return {"valid": (n_bad == 0) & (n_clash == 0), "bond_dev": worst, "bond_pair": pt[worst_pair.long()], "n_bad": n_bad,
            "clash": min_ratio, "clash_pair": min_pair, "n_clash": n_clash}


def repair_geometry(item, bounds="table", clash=0.60, pad=0.02, omega=1.0, max_iter=200, device="cuda", **table_kw):
    """relax_bounds over the item's generated conformers with the tables check_geometry builds from the item (the same `bounds`,
    `clash` and keywords): the conformers check_geometry calls invalid are moved into their bounds, the valid ones come back bit for
    bit.  Not MMFF (no energies, torsions or electrostatics; evaluation.py's use_force_field=True still raises).  The defaults come
    from a CPU prototype of the rule on hand-built molecules; none was tuned on a GPU.  Returns a dict of tensors on `device`:
        pos     float32 [G, n, 3]   the repaired conformers
        status  int32 [G]           0 valid as sampled, 1 repaired, 2 not repaired within max_iter updates, 3 not finite
        iters   int32 [G]           updates applied
        resid   float32 [G]         the largest distance still wanted by the stop rule, in Angstrom
        moved   float32 [G]         the root mean square displacement of the atoms"""
    pairs, lo, hi, radius, ex_ptr, ex_idx = _tables(item, bounds, table_kw)
    pos = _lib.conformers(item["pos_gen"], num_atoms(item), device)
    out = relax_bounds(pos, pairs, lo, hi, radius, ex_ptr, ex_idx, clash=clash, pad=pad, omega=omega, max_iter=max_iter)
    return dict(zip(("pos", "status", "iters", "resid", "moved"), out))


def main(argv=None):
    """python -m agdiff_amd.validity --samples samples_all.npz --testset test.npz [--refs refs.npz] [--clash 0.6] --out validity.npz
    Checks every molecule of a finished job (agdiff_amd.driver: `pos_gen_<i>`; the bonds come from the test set, extended to order 3).
    Writes per molecule `valid_<i>` int8 [G], `bond_dev_<i>` float32 [G], `bond_pair_<i>` int32 [G, 2], `n_bad_<i>` int32 [G],
    `clash_<i>` float32 [G], `clash_pair_<i>` int32 [G, 2], `n_clash_<i>` int32 [G] (+ `name_<i>`).  --refs (`pos_ref_<i>` [R, n, 3]):
    the bounds come from the molecule's reference conformers (bounds_from_references) instead of the covalent-radius table.
    --repair REPAIRED.npz: every molecule's conformers first go through repair_geometry (the same bounds and --clash; --pad, --omega,
    --max-iter); REPAIRED.npz is a copy of the samples file with every `pos_gen_<i>` repaired plus `repair_status_<i>` int8 [G] and
    `repair_moved_<i>` float32 [G], and --out holds the verdicts on the repaired conformers.  Not MMFF: a projection onto the bounds."""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", required=True)
    ap.add_argument("--testset", required=True)
    ap.add_argument("--refs", default=None, help="bounds from these reference conformers instead of the covalent-radius table")
    ap.add_argument("--clash", type=float, default=0.60, help="fraction of the van der Waals sum below which a pair clashes")
    ap.add_argument("--out", required=True)
    ap.add_argument("--repair", default=None, metavar="REPAIRED.npz",
                    help="move the invalid conformers into their bounds first (repair_geometry; not MMFF) and write the samples file "
                         "with the repaired pos_gen_<i>, repair_status_<i> and repair_moved_<i> here; --out then judges the repaired ones")
    ap.add_argument("--pad", type=float, default=0.02, help="--repair: how far inside its limits a repaired distance is aimed (Angstrom)")
    ap.add_argument("--omega", type=float, default=1.0, help="--repair: the step's relaxation factor, in (0, 2)")
    ap.add_argument("--max-iter", type=int, default=200, help="--repair: most updates per conformer")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if not (args.clash >= 0.0 and np.isfinite(args.clash)):
        ap.error("--clash must be finite and >= 0")
    if not (args.pad > 0.0 and np.isfinite(args.pad)) or not 0.0 < args.omega < 2.0 or args.max_iter < 1:
        ap.error("--pad must be finite and > 0, --omega in (0, 2) and --max-iter >= 1")
    zr = np.load(args.refs, allow_pickle=False) if args.refs else None
    out, mols, confs, invalid, by_bond, by_clash = {}, 0, 0, 0, 0, 0
    repaired, fixed, stuck = None, 0, 0
    if args.repair:
        with np.load(args.samples, allow_pickle=False) as zs:
            repaired = {k: zs[k] for k in zs.files}
    for mol, item in sampled_items(args.testset, args.samples):
        i = mol["index"]
        if zr is not None:
            if "pos_ref_%d" % i not in zr.files:
                raise ValueError("--refs: %s has no pos_ref_%d" % (args.refs, i))
            item["pos_ref"] = zr["pos_ref_%d" % i]
        how = "references" if zr is not None else "table"
        if repaired is not None:
            rep = repair_geometry(item, bounds=how, clash=args.clash, pad=args.pad, omega=args.omega, max_iter=args.max_iter,
                                  device=args.device)
            status = rep["status"].cpu().numpy()
            item["pos_gen"] = rep["pos"].cpu().numpy().reshape(np.shape(repaired["pos_gen_%d" % i]))
            repaired["pos_gen_%d" % i] = item["pos_gen"]
            repaired["repair_status_%d" % i] = status.astype(np.int8)
            repaired["repair_moved_%d" % i] = rep["moved"].cpu().numpy()
            fixed += int((status == 1).sum())
            stuck += int((status == 2).sum())
        res = check_geometry(item, bounds=how, clash=args.clash, device=args.device)
        for k, v in res.items():
            out["%s_%d" % (k, i)] = v.cpu().numpy().astype(np.int8) if k == "valid" else v.cpu().numpy()
        out["name_%d" % i] = np.str_(mol["name"])
        bad, hit = res["n_bad"].cpu().numpy() > 0, res["n_clash"].cpu().numpy() > 0
        mols += 1
        confs += bad.shape[0]
        invalid += int((bad | hit).sum())
        by_bond += int(bad.sum())
        by_clash += int(hit.sum())
    np.savez_compressed(args.out, **out)
    if repaired is not None:
        np.savez_compressed(args.repair, **repaired)
        print("%d conformers were repaired, %d were not within %d updates; the verdicts are on the repaired conformers"
              % (fixed, stuck, args.max_iter))
    print("%d molecules, %d conformers, %d invalid (%d with a distance out of bounds, %d with a clash)"
          % (mols, confs, invalid, by_bond, by_clash))
    return out


if __name__ == "__main__":
    main()
