"""Torsion fingerprint deviation -- the second standard metric between conformers, next to the heavy-atom RMSD.

A conformer is defined by its torsion angles.  RMSD grows with the molecule, mixes ring breathing and bond-angle noise with rotamer
changes and does not say which bond turned; the TFD (rdkit Chem.TorsionFingerprints) is the mean circular difference of the
rotatable bonds' dihedrals, lies in [0, 1] whatever the molecule's size, and one threshold (0.2, say) serves a whole test set.
rdkit is not a dependency and the reference never computes a TFD, so the quantity is defined here in plain terms:

  bonds       the item's bond list entries of type 1 .. 21 (molecule.bonded_neighbours), hydrogens dropped
  rotatable   a heavy - heavy bond (u, v), u < v, of type 1 that is a bridge of the heavy-atom graph (in no ring), with at least two
              heavy neighbours at both ends, neither end carrying a type-3 (triple) bond; ordered by (u, v); T of them
  columns     for every rotatable bond every heavy neighbour a of u (a != v) and b of v (b != u): the quad (a, u, v, b); ordered by
              bond, a, b; Q of them.  A bond's canonical column is the one with the smallest a and b.
  dihedral    theta = atan2(|b2| b1 . n2, n1 . n2), b1 = p_u - p_a, b2 = p_v - p_u, b3 = p_b - p_v, n1 = b1 x b2, n2 = b2 x b3
  tmap        int32 [P, T]: row 0 the canonical columns; row p, for each bond, the column that holds the image of the bond's
              canonical quad under heavy-atom automorphism p (read in either direction: theta(a, u, v, b) = theta(b, v, u, a));
              duplicate rows removed
  TFD(x, y)   min_p min(S_p(x -> y), S_p(y -> x)),  S_p(x -> y) = sum_t w_t delta(x[tmap[0][t]], y[tmap[p][t]]) / (pi sum_t w_t),
              delta the circular difference (pi when an angle is NaN).  Both directions: the canonical choice of neighbours is not
              carried along by the automorphisms, and one direction alone is not symmetric in (x, y).  T = 0: 0.
  mirror      a reflection negates every dihedral: the TFD to y's mirror image is the same with y's angles negated.

rdkit's distance-from-centre weighting is not built; `weights` [T] takes any weighting a caller wants.

Ring terms are opt-in (rings=True; agdiff_amd.rings has the rings and their values): without them every ring bond is left out and
chair and twist-boat cyclohexane have TFD 0.  With them
  values      a conformer's table is its Q dihedral columns followed by its Rg ring columns tau_r (the ring torsion value of
              Schulz-Gasch et al. 2012: the mean |dihedral| around the ring, in [0, pi])
  terms       the T rotatable bonds followed by the Rg rings, each with a scale s_t -- pi for a bond, pi exp(-0.025 (N - 14)^2)
              for a ring of N atoms, as published -- and a flag even_t, 1 for a ring: a reflection negates a dihedral and leaves tau
  tmap        ring r goes to column Q + (the ring with the image atom set under automorphism p)
  TFD(x, y)   as above with S_p(x -> y) = sum_t w_t min(1, delta_t / s_t) / sum_t w_t, delta_t = s_t when a value is NaN.  The cap
              keeps the range [0, 1]: a chair (tau = 60 degrees) against a flat ring would otherwise score 1.65 on that term.
              rdkit is believed not to cap, and agreement with rdkit is NOT claimed.  The mirror value negates y only where
              even_t = 0.
tau cannot tell a chair from its ring-flipped chair; only the sign of the Cremer-Pople q_3 (agdiff_amd.rings) can.

Angles and matrices are computed on the GPU (csrc/eval.hip: agdiff_torsion_angles, agdiff_tfd_matrix; with ring terms
agdiff_ring_coords, agdiff_tfd_matrix_terms); there is no CPU fallback.

    python -m agdiff_amd.torsions --samples out/samples_all.npz --testset test.npz --out torsions.npz
"""
import numpy as np

from . import _lib
from .ensemble import bits_pitch
from .evaluation import selection_of
from .molecule import as_host, bonded_neighbours, bonds_of, bridges, check_threshold, num_atoms, sampled_items

MAX_COLUMNS = _lib.DEFINES["AGDIFF_TFD_MAX_COLUMNS"]


def _heavy_graph(atom_type, bond_index, bond_type):
    """(heavy bool [n], adj: per atom {neighbour: type} over ALL bonded atoms, hadj: per atom the sorted heavy neighbours)"""
    at = np.asarray(atom_type).reshape(-1).astype(np.int64)
    n = at.shape[0]
    adj = bonded_neighbours(n, bond_index, bond_type)
    heavy = at != 1
    hadj = [sorted(j for j in adj[i] if heavy[j]) if heavy[i] else [] for i in range(n)]
    return heavy, adj, hadj


_bridges = bridges            # (the search lives in molecule.py, which ezbonds.py shares; the name stays for its importers)


def _columns(atom_type, bond_index, bond_type):
    """(bonds [(u, v)], per bond its quads [(a, u, v, b)] in (a, b) order)"""
    heavy, adj, hadj = _heavy_graph(atom_type, bond_index, bond_type)
    bridges = _bridges(hadj)
    triple = [any(ty == 3 for ty in adj[i].values()) for i in range(len(adj))]
    bonds, quads = [], []
    for u, v in sorted(bridges):
        if adj[u][v] != 1 or len(hadj[u]) < 2 or len(hadj[v]) < 2 or triple[u] or triple[v]:
            continue
        bonds.append((u, v))
        quads.append([(a, u, v, b) for a in hadj[u] if a != v for b in hadj[v] if b != u])
    return bonds, quads


def rotatable_bonds(atom_type, bond_index, bond_type):
    """(bonds int32 [T, 2], canonical quads int32 [T, 4]): the rotatable bonds (u, v), u < v, in (u, v) order -- single, in no ring,
    at least two heavy neighbours at both ends, no triple bond at either end -- and for each the quad (a, u, v, b) with the smallest
    heavy neighbour a of u and b of v.  Hydrogens and the 2- / 3-hop entries (type >= 22) of the bond list take no part."""
    bonds, quads = _columns(atom_type, bond_index, bond_type)
    return (np.asarray(bonds, dtype=np.int32).reshape(-1, 2), np.asarray([q[0] for q in quads], dtype=np.int32).reshape(-1, 4))


def torsion_table(item, rings=False):
    """(quads int32 [Q, 4], tmap int32 [P', T]) of an item (atom_type + its bonds; optionally perms): every column of every rotatable
    bond, and the distinct rows of the column mappings under the molecule's heavy-atom automorphisms (the item's `perms`, or its
    bonds through evaluation.selection_of, exactly as for the RMSD), row 0 = the canonical columns.  T = 0: ([0, 4], [1, 0]).
    rings=True (or a list of rings of the caller's own, each the atoms in walking order, 4 .. AGDIFF_RING_MAX_ATOMS of them; True =
    rings.find_rings): (quads, tmap int32 [P', T + Rg], scale float32 [T + Rg], even int32 [T + Rg], ring_ptr, ring_idx) -- the
    rings are terms T .. T + Rg - 1, ring r in column Q + r of the value table and in the rows of tmap at Q + (the ring whose atom
    set is the image of r's); scale is pi for a bond and rings.ring_scales for a ring, even 0 for a bond and 1 for a ring."""
    at = np.asarray(item["atom_type"]).reshape(-1)
    bonds, per_bond = _columns(at, *bonds_of(item))
    T = len(bonds)
    cols = [q for qs in per_bond for q in qs]
    where = {q: k for k, q in enumerate(cols)}
    first = np.cumsum([0] + [len(qs) for qs in per_bond])[:T]
    ring_list = []
    if rings is not False:
        from .rings import find_rings, pack_rings, ring_scales
        ring_list = find_rings(at, *bonds_of(item)) if rings is True else [tuple(int(a) for a in r) for r in rings]
        ring_ptr, ring_idx = pack_rings(ring_list)
    which = {frozenset(r): k for k, r in enumerate(ring_list)}
    rows = [tuple(int(f) for f in first) + tuple(len(cols) + k for k in range(len(ring_list)))]
    _, heavy, pa = selection_of(item)
    if pa is not None and (T or ring_list):
        order = {int(h): k for k, h in enumerate(heavy)}
        for p in pa:
            image = lambda i: int(heavy[p[order[i]]])
            row = []
            for qs in per_bond:
                a, u, v, b = (image(i) for i in qs[0])
                k = where.get((a, u, v, b), where.get((b, v, u, a)))
                if k is None:
                    raise ValueError("perms holds a mapping that is no automorphism of the molecule's bonds: the image of torsion "
                                     "%s is no torsion" % (qs[0],))
                row.append(k)
            for r in ring_list:
                if any(i not in order for i in r):
                    raise ValueError("ring %r names an atom that is no heavy atom of the molecule" % (r,))
                k = which.get(frozenset(image(i) for i in r))
                if k is None:
                    raise ValueError("the image of ring %r under a mapping of the molecule onto itself is no ring of the table" % (r,))
                row.append(len(cols) + k)
            if tuple(row) not in rows:
                rows.append(tuple(row))
    quads = np.asarray(cols, dtype=np.int32).reshape(-1, 4)
    tmap = np.asarray(rows, dtype=np.int32).reshape(len(rows), T + len(ring_list))
    if rings is False:
        return quads, tmap
    scale = np.concatenate([np.full(T, np.pi, dtype=np.float32), ring_scales(ring_ptr)])
    even = np.concatenate([np.zeros(T, dtype=np.int32), np.ones(len(ring_list), dtype=np.int32)])
    return quads, tmap, scale, even, ring_ptr, ring_idx


def torsion_angles(pos, quads):
    """agdiff_torsion_angles on pos [G, n, 3] (float32, contiguous, on the GPU): float32 [G, Q], the dihedral of every quad
    (int32 [Q, 4], numpy or tensor) in radians in [-pi, pi]; NaN for a degenerate quad, a coordinate that is not finite or an atom
    index outside [0, n)."""
    import torch
    _lib.require_device_conformers(pos)
    G, n = int(pos.shape[0]), int(pos.shape[1])
    q = as_host(quads, np.int32).reshape(-1, 4)
    Q = q.shape[0]
    out = torch.empty((G, Q), dtype=torch.float32, device=pos.device)
    if G == 0 or Q == 0:
        return out
    _lib.call("agdiff_torsion_angles", pos, torch.from_numpy(q).to(pos.device), G, n, Q, out)
    return out


def tfd_from_angles(ang_x, ang_y, tmap, weights=None, threshold=None, want_out=True, want_mirror=False, rings=False):
    """agdiff_tfd_matrix on two angle tables of one molecule (float32 [R, Q] and [G, Q] on the GPU; the same tensor for a self
    matrix): (out [R, G] or None, mirror [R, G] or None, bits int64 [R, pitch / 8] or None -- the packed `out <= threshold` in the
    layout of ensemble.bits_pitch(G) / ensemble.unpack_bits).  tmap int32 [P, T] (numpy), weights [T] > 0 or None.  The entries of
    tmap are checked against Q here, on the host; more than AGDIFF_TFD_MAX_COLUMNS columns: AgdiffLimitError.
    rings = (scale [T], even [T]) as torsion_table(item, rings=True) returns them: agdiff_tfd_matrix_terms on value tables that carry
    the ring columns behind the dihedrals (value_table); Q, T and the column limit then count the ring columns and terms."""
    import torch
    for a in (ang_x, ang_y):
        _lib.require_device_table(a, "angle tables must be contiguous float32 tensors [conformers, Q] on one GPU")
    dev = ang_x.device
    if ang_y.device != dev:
        raise ValueError("angle tables must be contiguous float32 tensors [conformers, Q] on one GPU")
    R, Q, G = int(ang_x.shape[0]), int(ang_x.shape[1]), int(ang_y.shape[0])
    if int(ang_y.shape[1]) != Q:
        raise ValueError("angle tables of %d and %d columns" % (Q, ang_y.shape[1]))
    tm = np.ascontiguousarray(np.asarray(tmap), dtype=np.int32)
    if tm.ndim != 2 or tm.shape[0] < 1:
        raise ValueError("tmap must be int32 [P, T] with P >= 1")
    P, T = tm.shape
    if T and (tm.min() < 0 or tm.max() >= Q):
        raise ValueError("tmap names columns outside [0, %d)" % Q)
    wt = None
    if weights is not None:
        wn = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
        if wn.shape[0] != T or not (wn > 0).all() or not np.isfinite(wn).all():
            raise ValueError("weights must be %d finite numbers > 0" % T)
        wt = torch.from_numpy(wn).to(dev) if T else None
    if rings is not False:
        sc = np.ascontiguousarray(np.asarray(rings[0], dtype=np.float32).reshape(-1))
        ev = np.ascontiguousarray(np.asarray(rings[1]).reshape(-1) != 0, dtype=np.int32)
        if sc.shape[0] != T or ev.shape[0] != T or not (sc > 0).all() or not np.isfinite(sc).all():
            raise ValueError("rings must be (scale, even): %d finite scales > 0 and %d flags" % (T, T))
        if Q > MAX_COLUMNS:
            raise _lib.AgdiffLimitError("tfd_from_angles: %d value columns with the ring columns counted, more than "
                                        "AGDIFF_TFD_MAX_COLUMNS = %d" % (Q, MAX_COLUMNS))
    if not (want_out or want_mirror or threshold is not None):
        raise ValueError("nothing asked for: no matrix and no threshold")
    out = torch.empty((R, G), dtype=torch.float32, device=dev) if want_out else None
    mirror = torch.empty((R, G), dtype=torch.float32, device=dev) if want_mirror else None
    bits = None
    if threshold is not None:
        bits = torch.empty((R, bits_pitch(G) // 8), dtype=torch.int64, device=dev)
    if R == 0 or G == 0:
        return out, mirror, bits
    tt = torch.from_numpy(tm).to(dev) if T else None
    if rings is not False:
        _lib.call("agdiff_tfd_matrix_terms", ang_x if Q else None, ang_y if Q else None, tt, wt,
                  torch.from_numpy(sc).to(dev) if T else None, torch.from_numpy(ev).to(dev) if T else None, R, G, Q, T, P,
                  0.0 if threshold is None else check_threshold(threshold, "TFD"), out, mirror, bits)
        return out, mirror, bits
    _lib.call("agdiff_tfd_matrix", ang_x if Q else None, ang_y if Q else None, tt, wt, R, G, Q, T, P,
              0.0 if threshold is None else check_threshold(threshold, "TFD"), out, mirror, bits)
    return out, mirror, bits


def _angles_of(item, key, quads, device):
    pos = _lib.conformers(item[key], num_atoms(item), device)
    return pos, torsion_angles(pos, quads)


def value_table(pos, quads, ring_ptr, ring_idx):
    """float32 [G, Q + Rg]: the dihedral of every quad followed by the ring torsion value of every ring (rings.ring_torsion_values),
    the value table of the TFD with ring terms"""
    import torch
    from .rings import ring_torsion_values
    return torch.cat([torsion_angles(pos, quads), ring_torsion_values(pos, ring_ptr, ring_idx)], dim=1).contiguous()


def _values_of(item, key, table, device):
    """(pos on the device, its value table) for a torsion_table(item, rings=True)"""
    pos = _lib.conformers(item[key], num_atoms(item), device)
    return pos, value_table(pos, table[0], table[4], table[5])


def tfd_matrix(item, hands=False, weights=None, device="cuda", rings=False):
    """The TFD confusion matrix [references x generated] of an item (atom_type, bonds, pos_ref, pos_gen), float32 on `device`.
    hands=True: (proper, mirror) -- mirror is the TFD of every generated conformer's mirror image to the references.
    rings=True: with the molecule's rings as terms behind the rotatable bonds (the module's docstring; weights then [T + Rg])."""
    if rings is not False:
        table = torsion_table(item, rings=rings)
        _, ref = _values_of(item, "pos_ref", table, device)
        _, gen = _values_of(item, "pos_gen", table, device)
        out, mirror, _ = tfd_from_angles(ref, gen, table[1], weights=weights, want_mirror=hands, rings=table[2:4])
        return (out, mirror) if hands else out
    quads, tmap = torsion_table(item)
    _, ref = _angles_of(item, "pos_ref", quads, device)
    _, gen = _angles_of(item, "pos_gen", quads, device)
    out, mirror, _ = tfd_from_angles(ref, gen, tmap, weights=weights, want_mirror=hands)
    return (out, mirror) if hands else out


def _self_tfd(item, device, threshold=None, weights=None, want_out=True, rings=False):
    """(gen [G, n, 3] on the device, out [G, G] or None, bits or None)"""
    if rings is not False:
        table = torsion_table(item, rings=rings)
        gen, val = _values_of(item, "pos_gen", table, device)
        out, _, bits = tfd_from_angles(val, val, table[1], weights=weights, threshold=threshold, want_out=want_out, rings=table[2:4])
        return gen, out, bits
    quads, tmap = torsion_table(item)
    gen, ang = _angles_of(item, "pos_gen", quads, device)
    out, _, bits = tfd_from_angles(ang, ang, tmap, weights=weights, threshold=threshold, want_out=want_out)
    return gen, out, bits


def tfd_self(item, threshold=None, weights=None, device="cuda", rings=False):
    """(out [G, G], bits): the TFD between the item's generated conformers -- exactly symmetric -- and, with a threshold, the packed
    adjacency `out <= threshold` (int64 [G, pitch / 8]; ensemble.unpack_bits, ensemble.leader_prune), else None.  rings=True: with
    the molecule's rings as terms."""
    thr = None if threshold is None else check_threshold(threshold, "TFD")
    if rings is not False:   # (passed only when set: without it _self_tfd gets the arguments it got before)
        _, out, bits = _self_tfd(item, device, threshold=thr, weights=weights, rings=rings)
    else:
        _, out, bits = _self_tfd(item, device, threshold=thr, weights=weights)
    return out, bits


def main(argv=None):
    """python -m agdiff_amd.torsions --samples samples_all.npz --testset test.npz --out torsions.npz
    For every molecule of a finished job (agdiff_amd.driver: `pos_gen_<i>`; the bonds come from the test set) writes
    `torsion_quads_<i>` int32 [T, 4], the canonical quad (a, u, v, b) of each rotatable bond, and `torsion_<i>` float32 [G, T], their
    dihedrals in radians in every conformer (+ `name_<i>`): what a torsion histogram or a phi / psi plot is drawn from."""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", required=True)
    ap.add_argument("--testset", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    out, mols, total = {}, 0, 0
    for mol, item in sampled_items(args.testset, args.samples):
        i = mol["index"]
        _, quads = rotatable_bonds(mol["atom_type"], mol["edge_index"], mol["edge_type"])
        pos = _lib.conformers(item["pos_gen"], num_atoms(item), args.device)
        out["torsion_quads_%d" % i] = quads
        out["torsion_%d" % i] = torsion_angles(pos, quads).cpu().numpy()
        out["name_%d" % i] = np.str_(mol["name"])
        mols += 1
        total += quads.shape[0]
    np.savez_compressed(args.out, **out)
    print("%d molecules, %d rotatable bonds" % (mols, total))
    return out


if __name__ == "__main__":
    main()
