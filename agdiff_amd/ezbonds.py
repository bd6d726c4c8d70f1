"""E/Z of the double bonds of sampled conformers.

The score network sees atom types, bond types (single, double, triple, aromatic) and distances: nothing in its input says whether
a C=C, C=N or N=N double bond is E or Z.  The two isomers are different compounds, and the sampler is free to draw either.  This
module is the double-bond half of what stereo.py does for tetrahedral centres: it finds the stereogenic double bonds of a
molecular graph, takes their target parity from reference conformers (or from the user), and on the GPU (csrc/eval.hip; there is
no CPU fallback) judges every conformer's bonds and turns the wrong ones over:
    agdiff_torsion_angles      the dihedrals the check is read from (double_bond_verdict)
    agdiff_flip_double_bonds   state per bond, and a 180 degree rotation of one side of every wrong bond, in place

A stereogenic double bond is a bond of type 2 between atoms i < j, neither end carrying a second double bond or a triple bond (no
cumulenes), each end with one or two other bonded neighbours (hydrogens count) that differ in their 1-WL colour when there are
two, and the bond a bridge of the bond graph or in rings of 8 or more atoms only.  Its quad is (a, i, j, d), a and d the
lowest-index other neighbours of i and j.  The parity of a bond in a conformer is read from the dihedral phi of its quad as
agdiff_torsion_angles defines it (0: a and d eclipsed, pi: opposite): +1 trans (|phi| > 90 degrees, a and d on opposite sides,
cos phi < 0), -1 cis, 0 when a normal of the dihedral is zero or a coordinate is not finite.  A plain definition that any
toolkit's E/Z tags can be converted to; there is no CIP priority logic and there are no E/Z letters here.  `ez_quads` int32
[D, 4] and `ez` int8 [D] hold an item's bonds and their target parity (0: not tagged).

Not handled: ring double bonds are judged but never flipped (and those in rings of 7 or fewer atoms are forced cis and not
reported); amide and other partial double bonds (type 1); atropisomers.  How often a trained checkpoint draws the wrong isomer has
not been measured.

    python -m agdiff_amd.ezbonds --testset test.npz --refs refs.npz --out test_ez.npz
"""
import numpy as np

from . import _lib
from .molecule import as_host, bonded_neighbours, bonds_of, bridges, field, num_atoms, refine_colours


def _ring_size(nbrs, i, j):
    """Atoms of the smallest ring through the bond i - j: breadth-first from i to j without that bond.  None: a bridge."""
    dist = {i: 0}
    frontier = [i]
    while frontier:
        nxt = []
        for u in frontier:
            for v in nbrs[u]:
                if (u == i and v == j) or v in dist:
                    continue
                dist[v] = dist[u] + 1
                if v == j:
                    return dist[v] + 1
                nxt.append(v)
        frontier = nxt
    return None


def stereo_double_bonds(atom_type, bond_index, bond_type):
    """(quads int32 [D, 4], in_ring bool [D]): the stereogenic double bonds (module docstring) as (a, i, j, d), i < j, sorted by
    (i, j); in_ring marks those in a ring of 8 or more atoms, which can be judged but not flipped.  The colours are those of
    stereo.tetrahedral_centres (1-WL over ALL atoms); the 2- / 3-hop entries of the bond list (type >= 22) take no part."""
    at = np.asarray(atom_type).reshape(-1).astype(np.int64)
    n = at.shape[0]
    adj = bonded_neighbours(n, bond_index, bond_type)
    colour = refine_colours(at, adj)
    nbrs = [sorted(a) for a in adj]
    cut = bridges(nbrs)
    quads, in_ring = [], []
    for i in range(n):
        for j in nbrs[i]:
            if j < i or adj[i][j] != 2:
                continue
            ends = []
            for x, y in ((i, j), (j, i)):
                others = [k for k in nbrs[x] if k != y]
                if any(adj[x][k] in (2, 3) for k in others) or len(others) not in (1, 2):
                    break
                if len(others) == 2 and colour[others[0]] == colour[others[1]]:
                    break
                ends.append(others[0])
            if len(ends) != 2:
                continue
            ring = None if (i, j) in cut else _ring_size(nbrs, i, j)
            if ring is not None and ring < 8:
                continue
            quads.append((ends[0], i, j, ends[1]))
            in_ring.append(ring is not None)
    return np.asarray(quads, dtype=np.int32).reshape(-1, 4), np.asarray(in_ring, dtype=np.bool_)


def cos_dihedral(pos, quads):
    """float64 [K, D]: cos phi of every quad (a, i, j, d) in every conformer of pos [K, n, 3] (numpy), phi the dihedral as
    agdiff_torsion_angles defines it; NaN when a normal is zero or a coordinate is not finite."""
    p = np.asarray(pos, dtype=np.float64)
    p = p.reshape(-1, p.shape[-2], 3)
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    b1, b2, b3 = p[:, q[:, 1]] - p[:, q[:, 0]], p[:, q[:, 2]] - p[:, q[:, 1]], p[:, q[:, 3]] - p[:, q[:, 2]]
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.einsum("kci,kci->kc", n1, n2) / np.sqrt(np.einsum("kci,kci->kc", n1, n1) * np.einsum("kci,kci->kc", n2, n2))


def parities_from_conformers(pos, quads):
    """(target int8 [D], disagree int32 [D]) from reference conformers pos [K, n, 3], on numpy: the majority parity of each bond
    over the K conformers (+1 trans, -1 cis) -- 0 on a tie or when no conformer decides -- and the number of conformers on the
    minority side, exactly as stereo.parities_from_conformers does for the signed volumes."""
    c = cos_dihedral(pos, quads)
    ok = np.isfinite(c)
    plus = ((c < 0) & ok).sum(0)
    minus = ((c > 0) & ok).sum(0)
    return np.sign(plus - minus).astype(np.int8), np.minimum(plus, minus).astype(np.int32)


def _side(nbrs, start, i, j):
    """The atoms reachable from `start` without crossing the bond i - j, ascending"""
    seen, stack = {start}, [start]
    while stack:
        u = stack.pop()
        for v in nbrs[u]:
            if (u == i and v == j) or (u == j and v == i) or v in seen:
                continue
            seen.add(v)
            stack.append(v)
    return sorted(seen)


def flip_sides(n, bond_index, bond_type, quads, frozen=None):
    """(side_ptr int32 [D + 1], side_idx int32): per bond of quads the atoms on ONE side of the cut i - j, that side's end atom
    included, ascending -- the atoms agdiff_flip_double_bonds turns.  The smaller side, j's on a tie; with frozen (bool [n]: atoms
    that must not move, --hold-core's core mask) the side without a frozen atom instead.  An empty row -- judge, do not flip --
    for a ring bond and for a bond with a frozen atom on both sides."""
    n = int(n)
    q = as_host(quads, np.int32).reshape(-1, 4)
    if q.size and (q.min() < 0 or q.max() >= n):
        raise ValueError("quads name atoms outside [0, %d)" % n)
    fz = None
    if frozen is not None:
        fz = as_host(frozen).reshape(-1) != 0
        if fz.shape[0] != n:
            raise ValueError("frozen has %d entries for %d atoms" % (fz.shape[0], n))
    nbrs = [sorted(a) for a in bonded_neighbours(n, bond_index, bond_type)]
    ptr, idx = [0], []
    for _, i, j, _ in q.tolist():
        if j not in nbrs[i]:
            raise ValueError("quad bond (%d, %d) is no bond of the molecule" % (i, j))
        side_j = _side(nbrs, j, i, j)
        row = []
        if i not in side_j:                                  # (a bridge; else a ring bond: the cut does not separate)
            side_i = _side(nbrs, i, i, j)
            held_i = fz is not None and bool(fz[side_i].any())
            held_j = fz is not None and bool(fz[side_j].any())
            if held_i and held_j:
                row = []
            elif held_i or held_j:
                row = side_i if held_j else side_j
            else:
                row = side_j if len(side_j) <= len(side_i) else side_i
        idx.extend(row)
        ptr.append(len(idx))
    return np.asarray(ptr, dtype=np.int32), np.asarray(idx, dtype=np.int32)


def ez_table(item):
    """(quads int32 [D, 4], target int8 [D]) of an item's `ez_quads` and `ez` tags, checked against its atoms and bonds: every
    index in [0, n), (i, j) a bond of type 2, a bonded to i and d bonded to j, a != j and d != i."""
    quads, ez = field(item, "ez_quads"), field(item, "ez")
    if quads is None or ez is None:
        raise ValueError("the item carries no `ez_quads` / `ez` tags (int32 [D, 4] quads (a, i, j, d) of the stereogenic double bonds "
                         "and int8 [D] target parity, +1 trans, -1 cis, 0 untagged; python -m agdiff_amd.ezbonds adds them to a test "
                         "set from reference conformers)")
    n = num_atoms(item)
    q = as_host(quads)
    if q.ndim != 2 or q.shape[1] != 4:
        if q.size:
            raise ValueError("ez_quads must be int32 [D, 4] (got shape %s)" % (tuple(q.shape),))
        q = q.reshape(0, 4)
    q = q.astype(np.int32)
    t = as_host(ez).reshape(-1)
    if t.shape[0] != q.shape[0]:
        raise ValueError("ez has %d entries for %d quads" % (t.shape[0], q.shape[0]))
    if q.size and (q.min() < 0 or q.max() >= n):
        raise ValueError("ez_quads name atoms outside [0, %d)" % n)
    adj = bonded_neighbours(n, *bonds_of(item))
    for a, i, j, d in q.tolist():
        if adj[i].get(j) != 2:
            raise ValueError("ez tag on (%d, %d), which is no double bond (type 2) of the molecule" % (i, j))
        if a == j or a not in adj[i]:
            raise ValueError("ez quad (%d, %d, %d, %d): atom %d is no other bonded neighbour of atom %d" % (a, i, j, d, a, i))
        if d == i or d not in adj[j]:
            raise ValueError("ez quad (%d, %d, %d, %d): atom %d is no other bonded neighbour of atom %d" % (a, i, j, d, d, j))
    return q, np.sign(t.astype(np.int64)).astype(np.int8)


def _checked_tables(n, quads, target):
    q = as_host(quads, np.int32).reshape(-1, 4)
    t = as_host(target, np.int8).reshape(-1)
    if t.shape[0] != q.shape[0]:
        raise ValueError("%d quads but %d targets" % (q.shape[0], t.shape[0]))
    if q.size and (q.min() < 0 or q.max() >= n):
        raise ValueError("quads name atoms outside [0, %d)" % n)
    return q, t


def double_bond_verdict(pos, quads, target):
    """The check: state int8 [G, D] on the device for pos [G, n, 3] (float32, contiguous, on the GPU): +1 the bond has its target
    parity, -1 the other one, 0 undecided (a degenerate or non-finite quad, or exactly 90 degrees) or untagged (target 0).  Read
    from the dihedrals of agdiff_torsion_angles: |theta| > pi / 2 is trans, a NaN gives 0."""
    import torch
    from .torsions import torsion_angles
    _lib.require_device_conformers(pos)
    q, t = _checked_tables(int(pos.shape[1]), quads, target)
    theta = torsion_angles(pos, q).abs()
    half = torch.tensor(np.pi / 2, dtype=torch.float64, device=pos.device)
    parity = (theta.double() > half).to(torch.int8) - (theta.double() < half).to(torch.int8)     # (NaN: 0 - 0)
    want = torch.from_numpy(np.sign(t.astype(np.int64)).astype(np.int8)).to(pos.device)
    return parity * want[None, :]


def flip_double_bonds(pos, quads, target, side_ptr, side_idx, want_flipped=False):
    """agdiff_flip_double_bonds on pos [G, n, 3] (float32, contiguous, on the GPU), in place: every bond of quads int32 [D, 4]
    with the wrong parity against target int8 [D] and a row in the CSR table (side_ptr int32 [D + 1], side_idx int32; flip_sides)
    has that row's atoms turned by 180 degrees about the bond.  Returns state int8 [G, D] as it was BEFORE the flip (+1 right, -1
    wrong, 0 undecided or untagged); want_flipped=True: (state, flipped int32 [G], the number of flips applied to each conformer).
    Indices and the CSR table are checked here, on the host, before any launch."""
    import torch
    _lib.require_device_conformers(pos)
    G, n = int(pos.shape[0]), int(pos.shape[1])
    dev = pos.device
    q, t = _checked_tables(n, quads, target)
    D = q.shape[0]
    sp = as_host(side_ptr, np.int32).reshape(-1)
    si = as_host(side_idx, np.int32).reshape(-1)
    if sp.shape[0] != D + 1 or sp[0] != 0 or (np.diff(sp) < 0).any() or sp[-1] != si.shape[0]:
        raise ValueError("side_ptr must be int32 [%d], start at 0, not decrease and end at len(side_idx) = %d" % (D + 1, si.shape[0]))
    if si.size and (si.min() < 0 or si.max() >= n):
        raise ValueError("side_idx names atoms outside [0, %d)" % n)
    state = torch.zeros((G, D), dtype=torch.int8, device=dev)
    flipped = torch.zeros(G, dtype=torch.int32, device=dev)
    if G and D:
        _lib.call("agdiff_flip_double_bonds", pos, torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(sp).to(dev),
                  torch.from_numpy(si).to(dev) if si.size else None, G, n, D, state, flipped)
    return (state, flipped) if want_flipped else state


def fix_double_bonds(item, pos, frozen=None):
    """Flips, in place, the wrong tagged double bonds of pos [G, n, 3] (contiguous float32 tensor on the GPU) of `item` (atom_type,
    bonds, ez_quads, ez) and returns state int8 [G, D] as it was BEFORE the flip.  frozen (bool [n]): atoms that must not move; a
    bond with one on both sides is judged only, like a ring bond."""
    _lib.require_device_conformers(pos)
    n = num_atoms(item)
    if pos.shape[1] != n:
        raise ValueError("pos has %d atoms per conformer, the item %d" % (pos.shape[1], n))
    quads, target = ez_table(item)
    side_ptr, side_idx = flip_sides(n, *bonds_of(item), quads, frozen=frozen)
    return flip_double_bonds(pos, quads, target, side_ptr, side_idx)


def wrong_share(item, device="cuda"):
    """The share of the item's generated conformers (pos_gen) with at least one tagged double bond of the wrong parity; host tables
    and the check only, nothing is moved.  NaN without a tagged bond."""
    quads, target = ez_table(item)
    if not (target != 0).any():
        return float("nan")
    pos = _lib.conformers(item["pos_gen"], num_atoms(item), device)
    if pos.shape[0] == 0:
        return float("nan")
    return float((double_bond_verdict(pos, quads, target) < 0).any(dim=1).double().mean())


def main(argv=None):
    """python -m agdiff_amd.ezbonds --testset test.npz --refs refs.npz --out test_ez.npz
    Copies the test set and adds `ez_quads_<i>` int32 [D, 4], the quads (a, i, j, d) of the molecule's stereogenic double bonds, and
    `ez_<i>` int8 [D]: the majority parity of the molecule's reference conformers (`pos_ref_<i>` [R, n, 3] of refs.npz; +1 trans, -1
    cis, 0 on a tie).  Host work only."""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--testset", required=True)
    ap.add_argument("--refs", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    zt, zr = np.load(args.testset, allow_pickle=False), np.load(args.refs, allow_pickle=False)
    out = {k: zt[k] for k in zt.files}
    for i in range(int(zt["count"])):
        at = zt["atom_type_%d" % i]
        n = at.shape[0]
        name = str(zt["name_%d" % i]) if "name_%d" % i in zt.files else "mol%d" % i
        if "pos_ref_%d" % i not in zr.files:
            print("%s: no pos_ref_%d in %s; not tagged" % (name, i, args.refs))
            continue
        quads, in_ring = stereo_double_bonds(at, zt["edge_index_%d" % i], zt["edge_type_%d" % i])
        target, disagree = parities_from_conformers(np.asarray(zr["pos_ref_%d" % i]).reshape(-1, n, 3), quads)
        out["ez_quads_%d" % i] = quads
        out["ez_%d" % i] = target
        print("%s: %d stereogenic double bonds (%d in a ring), %d with disagreeing references (%d tagged)"
              % (name, quads.shape[0], int(in_ring.sum()), int((disagree > 0).sum()), int((target != 0).sum())))
    with open(args.out, "wb") as f:
        np.savez_compressed(f, **out)
    return out


if __name__ == "__main__":
    main()
