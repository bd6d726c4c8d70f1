"""Conformers under torsion restraints: circular windows on dihedral angles, applied while the sampler runs.

A torsion scan (one ensemble per grid value of a rotatable bond), a fixed phi / psi pair, an amide held trans, a biaryl twist held
to a docking pose.  A distance window (restraints.py) cannot say any of these: a 1-4 distance fixes |theta| at best, never its
sign, and the sampler draws either sign.  A restraint is a quad (a, u, v, b) over a bridge bond u - v with a window
target +- tol in radians, theta as torsions.py defines it; after a step's update one side of every violated bond is turned rigidly
about the bond, the fraction `weight` of the way onto the violated edge of the window (csrc/eval.hip: agdiff_restrain_torsions,
fp64, one wave per graph of a packed batch; there is no CPU fallback), and the network relaxes the molecule around it in the steps
that follow.  A rigid turn about a bridge changes no bond length, no angle and no other bond's dihedral, so restraints on distinct
bonds are independent and weight 1 satisfies all of them at once.  A restraint is soft all the same: the steps between two
launches move the angle again, and `tors_viol` says what is left.  DESIGN.md 4.19.

    bridge_quads           the bonds of a molecule that can carry a restraint, as quads
    torsion_sides          the atoms one restraint turns: the smaller side of its bridge, or the side without a frozen atom
    restraint_arguments    the checks of epsnet.LangevinRun's keywords torsion_quads / _target / _tol / _sides / _weight / _start_sigma
    restrain_torsions      one stand-alone launch on a packed batch
    add_torsion_restraints / load_torsion_restraints   the test set's `tors_quads_<i>`, `tors_target_<i>`, `tors_tol_<i>`
    pack_torsion_restraints   batch-level quads and the shared side table of a driver.pack_batch result
    scan_grid              the [K, 1] target table of a torsion scan: conformer c takes row c mod K
    sample_restrained      one molecule x num_samples conformers, with the reference driver's retry rule
    python -m agdiff_amd.torsion_restraints   a sampling job under the test set's restraints, or --report on a finished one

Inside a run the restraints are constraints.TorsionRestraints, the second entry of constraints.ORDER; the launcher's prologue, the
sampling routine and the job's skeleton are shared with restraints.py and live in constraints.py too.

The CHEMISTRY IS UNVERIFIED: nobody has run this on a trained checkpoint.  No angle restraints, no ring bonds (a ring bond cannot
be turned rigidly), no symmetry-equivalent atom mappings, no --dist-mode shard; packed multi-molecule jobs through driver.run_job
are a follow-up.
"""
import math

import numpy as np

from . import _lib, constraints
from .ezbonds import _side
from .molecule import as_host, bonded_neighbours

_PI32 = float(np.float32(np.pi))             # (fp32's pi lies above pi: a target or tolerance given as np.float32(np.pi) is legal)


def torsion_sides(n, bond_index, bond_type, quads, frozen=None):
    """(quads int32 [T, 4], side_ptr int32 [T + 1], side_idx int32) for the restraints `quads` (a, u, v, b) of ONE molecule of n
    atoms: row t lists, ascending, the atoms on one side of the cut u - v, that side's end atom included -- the atoms
    agdiff_restrain_torsions turns.  ezbonds.flip_sides' rule: the smaller side, v's on a tie; with frozen (bool [n]: atoms that
    must not move, a held core's mask) the side without a frozen atom instead, and an empty row -- measure, do not turn -- for a bond
    with a frozen atom on both sides.  A row always lists the v, b end of its quad: a quad whose chosen side is u's comes back
    reversed, (b, v, u, a), which has the same dihedral.  ValueError: an atom outside [0, n), u - v no bond, a not bonded to u or b
    not bonded to v, a == v or b == u, a ring bond (it cannot be turned rigidly), two restraints on one bond."""
    n = int(n)
    q = as_host(quads)
    if q.size and (q.ndim != 2 or q.shape[1] != 4):
        raise ValueError("torsion quads must have shape [T, 4], got %s" % (tuple(q.shape),))
    q = np.array(q, dtype=np.int32).reshape(-1, 4)
    if q.size and (q.min() < 0 or q.max() >= n):
        raise ValueError("torsion quads name atoms outside [0, %d)" % n)
    fz = None
    if frozen is not None:
        fz = as_host(frozen).reshape(-1) != 0
        if fz.shape[0] != n:
            raise ValueError("frozen has %d entries for %d atoms" % (fz.shape[0], n))
    adj = bonded_neighbours(n, bond_index, bond_type)
    nbrs = [sorted(a) for a in adj]
    out, ptr, idx, seen = [], [0], [], set()
    for a, u, v, b in q.tolist():
        if v not in adj[u]:
            raise ValueError("torsion quad (%d, %d, %d, %d): (%d, %d) is no bond of the molecule" % (a, u, v, b, u, v))
        if a == v or a not in adj[u]:
            raise ValueError("torsion quad (%d, %d, %d, %d): atom %d is no other bonded neighbour of atom %d" % (a, u, v, b, a, u))
        if b == u or b not in adj[v]:
            raise ValueError("torsion quad (%d, %d, %d, %d): atom %d is no other bonded neighbour of atom %d" % (a, u, v, b, b, v))
        if (min(u, v), max(u, v)) in seen:
            raise ValueError("two torsion restraints on the bond (%d, %d)" % (u, v))
        seen.add((min(u, v), max(u, v)))
        side_v = _side(nbrs, v, u, v)
        if u in side_v:
            raise ValueError("torsion quad (%d, %d, %d, %d): (%d, %d) is a ring bond, which cannot be turned rigidly" % (a, u, v, b, u, v))
        side_u = _side(nbrs, u, u, v)
        held_u = fz is not None and bool(fz[side_u].any())
        held_v = fz is not None and bool(fz[side_v].any())
        if held_u and held_v:
            row, quad = [], (a, u, v, b)
        elif held_v or (not held_u and len(side_u) < len(side_v)):
            row, quad = side_u, (b, v, u, a)
        else:
            row, quad = side_v, (a, u, v, b)
        out.append(quad)
        idx.extend(row)
        ptr.append(len(idx))
    return np.asarray(out, dtype=np.int32).reshape(-1, 4), np.asarray(ptr, dtype=np.int32), np.asarray(idx, dtype=np.int32)


def bridge_quads(n, bond_index, bond_type):
    """int32 [B, 4]: one quad (a, u, v, b) for every bond of the molecule that can carry a torsion restraint -- a bridge u - v,
    u < v, with another bonded neighbour on both ends (a and b the lowest-index ones) --, sorted by (u, v)."""
    from .molecule import bridges
    nbrs = [sorted(a) for a in bonded_neighbours(int(n), bond_index, bond_type)]
    out = []
    for u, v in sorted(bridges(nbrs)):
        a, b = [k for k in nbrs[u] if k != v], [k for k in nbrs[v] if k != u]
        if a and b:
            out.append((a[0], u, v, b[0]))
    return np.asarray(out, dtype=np.int32).reshape(-1, 4)


def _quad_arrays(quads, target, tol):
    """(quads int32 [T, 4], target float32 [T], tol float32 [T]) on the host; ValueError for a quad list that is not [T, 4], for
    targets or tolerances of another length, a NaN, a target outside [-pi, pi] or a tolerance outside [0, pi]."""
    q = as_host(quads)
    if q.size and (q.ndim != 2 or q.shape[1] != 4):
        raise ValueError("torsion quads must have shape [T, 4], got %s" % (tuple(q.shape),))
    if q.size and not np.issubdtype(q.dtype, np.integer):
        raise ValueError("torsion quads must be atom indices (an integer array), got %s" % q.dtype)
    q = np.array(q, dtype=np.int32).reshape(-1, 4)
    if target is None or tol is None:
        raise ValueError("torsion quads need their targets and tolerances in radians (tol = pi: always satisfied)")
    tg, tl = (as_host(x, np.float32).reshape(-1) for x in (target, tol))
    if tg.shape[0] != q.shape[0] or tl.shape[0] != q.shape[0]:
        raise ValueError("%d torsion quads but %d targets and %d tolerances" % (q.shape[0], tg.shape[0], tl.shape[0]))
    if q.shape[0] and not (np.abs(tg) <= _PI32).all():
        raise ValueError("every torsion target must lie in [-pi, pi] radians")
    if q.shape[0] and not ((tl >= 0.0) & (tl <= _PI32)).all():
        raise ValueError("every torsion tolerance must lie in [0, pi] radians")
    return q, tg, tl


def _settings(weight, start_sigma):
    return constraints.weight_and_start(weight, start_sigma,
                                        "the torsion weight must lie in (0, 1] (got %r): 1 puts a violated angle onto the edge of its window",
                                        "the torsion start sigma must be a number (inf: restrain from the first step)")


def _side_table(T, sides):
    """(side_row int32 [T], side_ptr int32 [S + 1], side_idx int32) checked: rows in [-1, S), a CSR that starts at 0, does not
    decrease and ends at len(side_idx), offsets >= 0."""
    if not isinstance(sides, (tuple, list)) or len(sides) != 3:
        raise ValueError("torsion_sides must be (side_row [T], side_ptr [S + 1], side_idx) as pack_torsion_restraints returns them")
    row, ptr, idx = (as_host(x, np.int32).reshape(-1) for x in sides)
    S = ptr.shape[0] - 1
    if row.shape[0] != T:
        raise ValueError("%d torsion quads but %d side rows" % (T, row.shape[0]))
    if S < 0 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or ptr[-1] != idx.shape[0]:
        raise ValueError("side_ptr must start at 0, not decrease and end at len(side_idx) = %d" % idx.shape[0])
    if row.size and (row.min() < -1 or row.max() >= S):
        raise ValueError("side rows must lie in [-1, %d)" % S)
    if idx.size and idx.min() < 0:
        raise ValueError("side_idx holds offsets from the graph's first atom: none may be negative")
    return row, ptr, idx


def batch_sides(N, bond_index, bond_type, batch, quads, frozen=None):
    """(quads int32 [T, 4] oriented, (side_row, side_ptr, side_idx)) for batch-level quads of a packed batch with sorted graph ids
    `batch` [N] and batch-level bonds: torsion_sides ONCE PER DISTINCT TOPOLOGY -- graphs with the same atoms count, bond list,
    restraints and frozen mask (the conformers of a molecule) share their rows of the table."""
    b = as_host(batch).reshape(-1).astype(np.int64)
    q = as_host(quads, np.int32).reshape(-1, 4)
    G = int(b[-1]) + 1 if b.size else 0
    first = np.searchsorted(b, np.arange(G + 1))
    bi = as_host(bond_index).reshape(2, -1).astype(np.int64)
    bt = as_host(bond_type).reshape(-1).astype(np.int64)
    if bi.size and (bi.min() < 0 or bi.max() >= N):
        raise ValueError("bond_index names atoms outside the batch's %d atoms" % N)
    order = np.argsort(b[bi[0]], kind="stable")
    bi, bt = bi[:, order], bt[order]
    bptr = np.searchsorted(b[bi[0]], np.arange(G + 1))
    fz = None if frozen is None else (as_host(frozen).reshape(-1) != 0)
    if fz is not None and fz.shape[0] != N:
        raise ValueError("the frozen mask has %d entries, the batch %d atoms" % (fz.shape[0], N))
    graph_of = b[q[:, 1]]
    tptr = np.searchsorted(graph_of, np.arange(G + 1))
    out_q, side_row = np.empty_like(q), np.full(q.shape[0], -1, dtype=np.int32)
    known, ptr, idx = {}, [0], []
    for g in np.unique(graph_of).tolist():
        a0, n = int(first[g]), int(first[g + 1] - first[g])
        lb, lt = bi[:, bptr[g]:bptr[g + 1]] - a0, bt[bptr[g]:bptr[g + 1]]
        lq = q[tptr[g]:tptr[g + 1]] - a0
        lf = None if fz is None else fz[a0:a0 + n]
        key = (n, lb.tobytes(), lt.tobytes(), lq.astype(np.int64).tobytes(), b"" if lf is None else lf.tobytes())
        if key not in known:
            oq, sp, si = torsion_sides(n, lb, lt, lq, frozen=lf)
            rows = np.full(oq.shape[0], -1, dtype=np.int32)
            for t in range(oq.shape[0]):
                if sp[t + 1] > sp[t]:
                    rows[t] = len(ptr) - 1
                    idx.extend(si[sp[t]:sp[t + 1]].tolist())
                    ptr.append(len(idx))
            known[key] = (oq, rows)
        oq, rows = known[key]
        out_q[tptr[g]:tptr[g + 1]] = oq + a0
        side_row[tptr[g]:tptr[g + 1]] = rows
    return out_q, (side_row, np.asarray(ptr, dtype=np.int32), np.asarray(idx, dtype=np.int32))


def restraint_arguments(N, quads, target, tol, batch, sides=None, weight=1.0, start_sigma=float("inf"), bond_index=None, bond_type=None,
                        frozen=None, num_graphs=None):
    """(tr_ptr int32 [G + 1], quads int32 [T, 4], centre float32 [T], half float32 [T], sides, weight, start sigma) on the host for a
    batch of N atoms with sorted graph ids `batch` [N], or None when no quads are given (None or an empty list).  quads [T, 4] hold
    batch-level atoms (a, u, v, b), listed graph by graph.  sides: (side_row [T], side_ptr [S + 1], side_idx) for quads that are
    oriented already (pack_torsion_restraints); without them the table comes from batch_sides when the batch's bonds are given
    (frozen: atoms that must not move), and is None -- checked, not launchable -- without bonds.  ValueError: targets without
    quads, a wrong shape, an atom outside the batch, a quad across two graphs, quads not in graph order, a NaN, a target outside
    [-pi, pi], a tolerance outside [0, pi], a weight outside (0, 1], a start sigma that is NaN, and what torsion_sides refuses.
    Needs no GPU."""
    settings = _settings(weight, start_sigma)
    if quads is None:
        if target is not None or tol is not None or sides is not None:
            raise ValueError("torsion targets, tolerances and sides need torsion quads [T, 4]")
        return None
    N = int(N)
    q, tg, tl = _quad_arrays(quads, target, tol)
    if q.shape[0] == 0:
        return None
    if q.min() < 0 or q.max() >= N:
        raise ValueError("torsion quads name atoms outside the batch's %d atoms" % N)
    if batch is None:
        raise ValueError("torsion restraints need the batch's graph ids: the four atoms of a quad lie in one graph")
    b = as_host(batch).reshape(-1).astype(np.int64)
    if b.shape[0] != N:
        raise ValueError("batch has %d entries, the batch %d atoms" % (b.shape[0], N))
    gq = b[q]
    if (gq != gq[:, :1]).any():
        raise ValueError("a torsion quad names atoms of two different graphs")
    if (np.diff(gq[:, 0]) < 0).any():
        raise ValueError("torsion restraints must be listed graph by graph (in the order of the batch)")
    G = max(int(b[-1]) + 1, int(num_graphs or 0))
    tr_ptr = np.searchsorted(gq[:, 0], np.arange(G + 1)).astype(np.int32)
    if sides is not None:
        table = _side_table(q.shape[0], sides)
    elif bond_index is not None and bond_type is not None:
        q, table = batch_sides(N, bond_index, bond_type, b, q, frozen=frozen)
    else:
        table = None
    return (tr_ptr, q, tg, tl, table) + settings


SAMPLER_KEYWORDS = constraints.TorsionRestraints.KEYWORDS


def sampler_arguments(N, batch, torsion_quads=None, torsion_target=None, torsion_tol=None, torsion_sides=None, torsion_weight=1.0,
                      torsion_start_sigma=float("inf"), bond_index=None, bond_type=None, frozen=None, num_graphs=None):
    """restraint_arguments for epsnet.LangevinRun's keywords."""
    return restraint_arguments(N, torsion_quads, torsion_target, torsion_tol, batch, torsion_sides, torsion_weight, torsion_start_sigma,
                               bond_index=bond_index, bond_type=bond_type, frozen=frozen, num_graphs=num_graphs)


def restrain_torsions(pos, quads, target, tol, batch, sides, weight=1.0, turn=True, skip=None, copy_out=None, device="cuda"):
    """One agdiff_restrain_torsions launch on the packed batch `pos` [N, 3]: (pos, angle, viol).  A contiguous float32 tensor on the
    GPU is changed IN PLACE and returned; anything else is copied to `device` first.  `quads` [T, 4] batch-level atoms (a, u, v, b),
    graph by graph, with their windows `target` +- `tol` [T] in radians; `sides` = (side_row [T], side_ptr, side_idx) as
    pack_torsion_restraints / batch_sides return them WITH the quads (a row turns the v, b end), or None to only measure; `batch`
    [N] sorted graph ids; skip [G] (!= 0 leaves the graph alone) and copy_out (a contiguous float32 GPU tensor [N, 3] that
    receives every stored value) are optional.  turn=False moves nothing and only measures.  angle float32 [T] on the device: each
    dihedral as found when its turn came (NaN: degenerate, or its graph was left alone); viol float32 [G]: each graph's largest
    excess in radians BEFORE the call, 0 without restraints, NaN for a graph that was left alone."""
    import torch
    pos, gp, G, N, skip = constraints.launch_prologue(pos, batch, skip, copy_out, device)
    dev_ = pos.device
    args = restraint_arguments(N, quads, target if quads is not None else None, tol if quads is not None else None, batch,
                               sides if quads is not None else None, weight, num_graphs=G)
    D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev_)
    viol = torch.empty(G, dtype=torch.float32, device=dev_)
    if args is None:
        _lib.call("agdiff_restrain_torsions", pos, gp, torch.zeros(G + 1, dtype=torch.int32, device=dev_), None, None, None, None, None, None,
                  skip, G, N, 0, 0, 1.0, 0, copy_out, None, viol)
        return pos, torch.empty(0, dtype=torch.float32, device=dev_), viol
    tr_ptr, q, tg, tl, table, w, _ = args
    T = int(q.shape[0])
    if table is None:
        table = (np.full(T, -1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32))
    row, sp, si = table
    angle = torch.empty(T, dtype=torch.float32, device=dev_)
    _lib.call("agdiff_restrain_torsions", pos, gp, D(tr_ptr), D(q), D(tg), D(tl), D(row), D(sp), D(si) if si.size else None, skip, G, N, T,
              int(sp.shape[0]) - 1, w, 1 if turn else 0, copy_out, angle, viol)
    return pos, angle, viol


# ---- the test set's fields -------------------------------------------------------------------------------------------------
def _molecule_restraints(n, bond_index, bond_type, quads, target, tol, what):
    """One molecule's restraints checked against its n atoms and its bonds (molecule-level indices): (quads int32 [T, 4] as given,
    target float32 [K, T] -- a [T] list is one row --, tol float32 [T])."""
    try:
        q = as_host(quads)
        if q.ndim != 2 or q.shape[1] != 4:
            raise ValueError("torsion quads must have shape [T, 4], got %s" % (tuple(q.shape),))
        if target is None or tol is None:
            raise ValueError("torsion quads need their targets and tolerances in radians")
        tg = as_host(target, np.float32)
        tg = tg[None, :] if tg.ndim == 1 else tg
        if tg.ndim != 2 or tg.shape[0] < 1 or tg.shape[1] != q.shape[0]:
            raise ValueError("torsion targets must have shape [T] or [K, T] for %d quads, got %s" % (q.shape[0], tuple(tg.shape)))
        for row in tg:
            q, _, tl = _quad_arrays(q, row, tol)
        if q.size and (q.min() < 0 or q.max() >= n):
            raise ValueError("torsion quads name atoms outside [0, %d)" % n)
        torsion_sides(n, bond_index, bond_type, q)
    except ValueError as e:
        raise ValueError("%s: %s" % (what, e))
    return q, tg, tl


def add_torsion_restraints(testset_in, testset_out, restraints):
    """Copy the test set `testset_in` (driver.save_testset's .npz) to `testset_out` with `tors_quads_<i>` int32 [T, 4] (molecule-level
    atoms (a, u, v, b)), `tors_target_<i>` float32 [T] or [K, T] and `tors_tol_<i>` float32 [T], in radians, for every molecule
    index i of `restraints` = {i: (quads, target, tol)}; with a [K, T] table conformer c takes row c mod K (scan_grid).  Fields a
    molecule already had are replaced, every other field is kept.  ValueError for an index outside the test set and for what
    restraint_arguments and torsion_sides refuse."""
    z = np.load(testset_in, allow_pickle=False)
    out = {k: z[k] for k in z.files}
    count = int(z["count"])
    for i, (quads, target, tol) in restraints.items():
        i = int(i)
        if not 0 <= i < count:
            raise ValueError("torsion restraints for molecule %d, the test set has %d molecules" % (i, count))
        n = int(np.asarray(z["atom_type_%d" % i]).reshape(-1).shape[0])
        q, tg, tl = _molecule_restraints(n, z["edge_index_%d" % i], z["edge_type_%d" % i], quads, target, tol, "molecule %d" % i)
        out["tors_quads_%d" % i], out["tors_tol_%d" % i] = q, tl
        out["tors_target_%d" % i] = tg if as_host(target).ndim == 2 else tg[0]
    np.savez_compressed(testset_out, **out)


def load_torsion_restraints(testset):
    """{i: (quads int32 [T, 4], target float32 [T] or [K, T], tol float32 [T])} for the molecules of the test set that carry torsion
    restraints."""
    z = np.load(testset, allow_pickle=False)
    out = {}
    for i in range(int(z["count"])):
        keys = ["tors_%s_%d" % (k, i) for k in ("quads", "target", "tol")]
        if all(k in z.files for k in keys):
            n = int(np.asarray(z["atom_type_%d" % i]).reshape(-1).shape[0])
            q, _, tl = _molecule_restraints(n, z["edge_index_%d" % i], z["edge_type_%d" % i], *(z[k] for k in keys), what="molecule %d" % i)
            out[i] = (q, np.asarray(z[keys[1]], dtype=np.float32), tl)
    return out


def scan_grid(start, stop, step):
    """The target table of a torsion scan over ONE restraint: float32 [K, 1] with the angles start, start + step, ... below stop
    (radians), each wrapped into (-pi, pi].  Given as a molecule's `tors_target`, conformer c is restrained to row c mod K: one job
    samples the whole scan."""
    start, stop, step = float(start), float(stop), float(step)
    if not (step > 0.0 and stop > start and math.isfinite(stop - start)):
        raise ValueError("scan_grid needs start < stop and a step > 0")
    k = int(math.ceil((stop - start) / step - 1e-9))
    v = start + step * np.arange(k, dtype=np.float64)
    v = np.pi - np.mod(np.pi - v, 2.0 * np.pi)                      # (-pi, pi]
    return v.astype(np.float32).reshape(-1, 1)


def pack_torsion_restraints(packed, per_molecule, frozen=None):
    """Batch-level (quads int32 [T, 4], target float32 [T], tol float32 [T], sides) for a driver.pack_batch result: `per_molecule`
    holds, for every molecule of the batch in order, None or its (quads, target [T] or [K, T], tol) with molecule-level indices.
    Each list once per conformer, conformer by conformer, shifted by the spans; conformer c takes target row c mod K.  sides =
    (side_row, side_ptr, side_idx): torsion_sides once per MOLECULE, its rows shared by all of the molecule's conformers, the quads
    oriented to match.  frozen [N]: atoms that must not move (default: the batch's `core_select`, when it carries a core)."""
    spans = packed["spans"]
    if len(per_molecule) != len(spans):
        raise ValueError("%d torsion restraint lists for a batch of %d molecules" % (len(per_molecule), len(spans)))
    if frozen is None and packed.get("core_select") is not None:
        frozen = packed["core_select"]
    fz = None if frozen is None else as_host(frozen).reshape(-1) != 0
    bi, bt = np.asarray(packed["bond_index"]).reshape(2, -1), np.asarray(packed["bond_type"]).reshape(-1)
    qs, tgs, tls, rows = [np.zeros((0, 4), dtype=np.int32)], [np.zeros(0, dtype=np.float32)], [np.zeros(0, dtype=np.float32)], []
    ptr, idx = [0], []
    for k, (r, (off, n, g)) in enumerate(zip(per_molecule, spans)):
        if r is None or np.asarray(r[0]).size == 0:
            continue
        own = (bi[0] >= off) & (bi[0] < off + n)                     # the first conformer's bonds
        q, tg, tl = _molecule_restraints(n, bi[:, own] - off, bt[own], *r, what="molecule %d of the batch" % k)
        oq, sp, si = torsion_sides(n, bi[:, own] - off, bt[own], q, frozen=None if fz is None else fz[off:off + n])
        row = np.full(oq.shape[0], -1, dtype=np.int32)
        for t in range(oq.shape[0]):
            if sp[t + 1] > sp[t]:
                row[t] = len(ptr) - 1
                idx.extend(si[sp[t]:sp[t + 1]].tolist())
                ptr.append(len(idx))
        shift = off + n * np.arange(g, dtype=np.int64)
        qs.append((oq[None, :, :].astype(np.int64) + shift[:, None, None]).reshape(-1, 4).astype(np.int32))
        tgs.append(tg[np.arange(g) % tg.shape[0]].reshape(-1))
        tls.append(np.tile(tl, g))
        rows.append(np.tile(row, g))
    sides = (np.concatenate(rows) if rows else np.zeros(0, dtype=np.int32), np.asarray(ptr, dtype=np.int32), np.asarray(idx, dtype=np.int32))
    return np.concatenate(qs), np.concatenate(tgs), np.concatenate(tls), sides


def _of_molecule(mol):
    """(quads, target, tol) a molecule dict carries as tors_quads / tors_target / tors_tol, or None."""
    if mol.get("tors_quads") is None or np.asarray(mol["tors_quads"]).size == 0:
        return None
    return mol["tors_quads"], mol.get("tors_target"), mol.get("tors_tol")


def measure(mol, pos_gen, restraints, device="cuda"):
    """(viol float32 [G], angle float32 [G, T]) (numpy) of one molecule's conformers pos_gen [G, n, 3] under its (quads, target, tol):
    the launch that only measures, over the quads as pack_torsion_restraints orients them.  Zeros and a [G, 0] table without
    restraints; NaN for a conformer with a quad coordinate that is not finite."""
    from . import driver
    pos = np.asarray(pos_gen, dtype=np.float32)
    G, n = pos.shape[0], pos.shape[1]
    if restraints is None or G == 0:
        return np.zeros(G, dtype=np.float32), np.zeros((G, 0), dtype=np.float32)
    packed = driver.pack_batch([mol], lambda _num_refs: G)
    q, tg, tl, sides = pack_torsion_restraints(packed, [restraints])
    _, angle, viol = restrain_torsions(pos.reshape(G * n, 3), q, tg, tl, packed["batch"], sides, turn=False, device=device)
    return viol.cpu().numpy(), angle.cpu().numpy().reshape(G, -1)


# ---- sampling ------------------------------------------------------------------------------------------------------------------
def sample_restrained(model, mol, num_samples, sampler_kwargs, device, weight=1.0, start_sigma=float("inf"), counter_seed=None,
                      max_retry=2, log=print, restraint_weight=1.0, restraint_start_sigma=float("inf"), restraint_sweeps=1):
    """`num_samples` conformers of ONE molecule in one batch (the reference driver's own granularity), under the torsion restraints
    the molecule dict carries as tors_quads / tors_target / tors_tol (molecule-level indices; without them it is sampled
    unrestrained): (pos_gen float32 [G, n, 3] numpy, viol float32 [G], angle float32 [G, T], ok).  A molecule that also carries
    restr_pairs / restr_lo / restr_hi (restraints.py) is sampled under both, the distance restraints with restraint_weight /
    _start_sigma / _sweeps.  Packs with driver.pack_batch and samples with driver.run_part; the retry rule is scripts/test.py's, as
    driver.sample_passes applies it: the packing, the checks and the sampling are constraints.sample_restrained's.  viol: each
    conformer's largest excess in radians at the end of the run, angle its final dihedrals (zeros and [G, 0] without restraints); ok
    False: every attempt failed, all three NaN.  Holds no core."""
    G = int(num_samples)
    res = constraints.sample_restrained(model, mol, G, sampler_kwargs, device, torsions=dict(weight=weight, start_sigma=start_sigma),
                                        pairs=dict(weight=restraint_weight, start_sigma=restraint_start_sigma, sweeps=restraint_sweeps),
                                        counter_seed=counter_seed, max_retry=max_retry, log=log)
    if "torsion_viol" not in res:
        return res["pos"], constraints.no_violation(G, res["ok"]), np.zeros((G, 0), dtype=np.float32), res["ok"]
    return res["pos"], res["torsion_viol"], res["torsion_angle"], res["ok"]


def build_parser():
    return constraints.job_parser(main.__doc__, "test set with tors_quads_<i> / tors_target_<i> / tors_tol_<i> (add_torsion_restraints)",
                                  "the fraction of the way a violated angle is turned onto the edge of its window per step, in (0, 1]")


def main(argv=None):
    """python -m agdiff_amd.torsion_restraints --ckpt ckpt.pt --testset test.npz --out out/ [--num-confs 2x --n-steps 5000
        --w-global 1.0 --global-start-sigma 0.5 --clip 1000 --weight 1.0 --start-sigma inf --seed 2021 --noise default|counter
        --precision ... --start-idx --end-idx --trust-ckpt]
    samples every molecule of the range, ONE molecule per batch, under the torsion restraints the test set carries for it (and under
    its distance restraints `restr_*_<i>`, at their defaults, when it has those too; a molecule without torsion restraints is sampled
    without, so the output is a complete job), and writes out/samples_all.npz: `pos_gen_<i>` [G, n, 3], `name_<i>`, `tors_viol_<i>`
    float32 [G], each conformer's largest excess in radians on the saved positions, and `tors_angle_<i>` float32 [G, T], its final
    dihedrals (zeros and a [G, 0] table for a molecule without torsion restraints).  The post-sampling modules run on that file
    unchanged.
    python -m agdiff_amd.torsion_restraints --report --samples samples_all.npz --testset test.npz --out viol.npz
    measures a finished job: `tors_viol_<i>` and `tors_angle_<i>` for every molecule of the samples."""
    args = build_parser().parse_args(argv)
    from . import driver, restraints
    own = load_torsion_restraints(args.testset)
    pairs = {} if args.report else restraints.load_restraints(args.testset)
    mols = {m["index"]: m for m in driver.load_testset(args.testset)} if args.report else {}

    def attach(m):
        if m["index"] in own:
            m["tors_quads"], m["tors_target"], m["tors_tol"] = own[m["index"]]
        if m["index"] in pairs:
            m["restr_pairs"], m["restr_lo"], m["restr_hi"] = pairs[m["index"]]

    def sample(model, m, G, kw, device, counter_seed):
        pos, viol, angle, ok = sample_restrained(model, m, G, kw, device, weight=args.weight, start_sigma=args.start_sigma,
                                                 counter_seed=counter_seed)
        return dict(pos_gen=pos, tors_viol=viol, tors_angle=angle), ok

    def report(i, pos_gen):
        viol, angle = measure(mols[i], pos_gen, own.get(i), device=args.device)
        return dict(tors_viol=viol, tors_angle=angle)

    return constraints.restrained_job(args, own, lambda: _settings(args.weight, args.start_sigma), attach, sample, report,
                                      ("tors_viol", "torsion restraints",
                                       "largest excess left %.5f rad, median of the molecules' largest %.5f rad"))


if __name__ == "__main__":
    main()
