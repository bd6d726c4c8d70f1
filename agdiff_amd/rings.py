"""Ring conformations -- which shape a ring is in, and ring terms for the torsion fingerprint deviation.

torsions.rotatable_bonds takes bridges only, so the TFD does not see a ring: chair and twist-boat cyclohexane, the envelope and the
twist of a proline ring, every pucker of a sugar have TFD 0, and a molecule without a rotatable bond has only "one conformer".
This module finds the rings, describes each one's shape in every conformer on the GPU (csrc/eval.hip: agdiff_ring_coords; there is
no CPU fallback), and hands torsions.py what it needs to put the rings into the TFD (torsion_table(item, rings=True)).  rdkit is
not a dependency; the quantities are defined here and in include/agdiff_hip.h in plain terms:

  rings       the chordless simple cycles of 4 .. max_size (default 12) atoms of the heavy-atom graph of the item's bonds of type
              1 .. 21: no two atoms of the cycle that are not neighbours in it are bonded.  A chordless cycle is fixed by its atom
              set, so the set of rings is unique and every automorphism of the molecule carries it onto itself.  Naphthalene: the
              two six-rings, not the 10-perimeter; bicyclo[2.2.2]octane: three six-rings; norbornane: two five-rings and the
              six-ring; cubane: its 6 faces and 4 six-rings.  NOT the smallest set of smallest rings (SSSR), which is not unique.
              Three-rings have no conformation and are left out; rings of more than 12 atoms are not searched for (a caller may
              name one of up to AGDIFF_RING_MAX_ATOMS = 32 atoms by hand: pack_rings).
  walk        from the ring's lowest atom index towards that atom's lower-index ring neighbour; rings ordered by (size, atoms)
  tau         the ring torsion value of Schulz-Gasch et al., J. Chem. Inf. Model. 52, 1499 (2012): the mean |dihedral| over the N
              consecutive quads of the ring, in [0, pi].  Invariant under the start atom, the direction, rigid motion and
              reflection -- so it cannot tell a chair from its ring-flipped chair: only the sign of q_3 below can.
  pucker      the Cremer-Pople coordinates (J. Am. Chem. Soc. 97, 1354 (1975)): z_j = the atoms' heights over the ring's mean
              plane, (q_m, phi_m) for m = 2 .. floor((N - 1) / 2), the signed q_(N/2) for even N, total amplitude Q with
              sum q_m^2 = Q^2.  The amplitudes do not depend on the walk; the phases do, which is why the walk is pinned.
  scale       of a ring term in the TFD: pi exp(-0.025 (N - 14)^2), as published (36.34 degrees for a six-ring)
  class       of a six-ring, by theta = atan2(q_2, q_3) and phi_2 -- project defaults, not a standard: theta within 30 degrees of
              0 or 180: chair; within 30 degrees of 90: boat (phi_2 mod 60 nearer 0) or twist-boat (nearer 30); else
              half-chair/envelope

Not built: SSSR, rings of more than 12 atoms found automatically, rdkit's distance-from-centre weights, ring terms in the
torsion restraints.  Agreement with rdkit's TFD is not claimed (torsions.py says why).

    python -m agdiff_amd.rings --samples out/samples_all.npz --testset test.npz --out rings.npz
"""
import numpy as np

from . import _lib
from .molecule import as_host, bonded_neighbours, bonds_of, bridges, num_atoms, sampled_items

MAX_ATOMS = _lib.DEFINES["AGDIFF_RING_MAX_ATOMS"]
MIN_ATOMS = 4
CLASS_NAMES = ("", "chair", "boat", "twist-boat", "half-chair/envelope")      # ring_class codes 0 .. 4; 0 = no six-ring, or NaN


def find_rings(atom_type, bond_index, bond_type, max_size=12):
    """The rings of a molecule as a list of atom tuples: every chordless simple cycle of 4 .. max_size heavy atoms, each walked
    from its lowest atom towards that atom's lower ring neighbour, the list ordered by (size, atoms)."""
    at = np.asarray(atom_type).reshape(-1).astype(np.int64)
    n = at.shape[0]
    adj = bonded_neighbours(n, bond_index, bond_type)
    heavy = at != 1
    hadj = [sorted(j for j in adj[i] if heavy[j]) if heavy[i] else [] for i in range(n)]
    cut = bridges(hadj)                               # a bridge lies on no cycle
    nbrs = [set(j for j in hadj[i] if (min(i, j), max(i, j)) not in cut) for i in range(n)]
    max_size = min(int(max_size), MAX_ATOMS)
    found = []
    for s in range(n):                                # s = the lowest atom of the cycle; the path grows through atoms > s
        if len(nbrs[s]) < 2:
            continue
        stack = [(s, v) for v in sorted(nbrs[s], reverse=True) if v > s]
        while stack:
            path = stack.pop()
            for v in sorted(nbrs[path[-1]], reverse=True):
                if v <= s or v in path or any(v in nbrs[u] for u in path[1:-1]):
                    continue                          # (a bond to an inner atom of the path would be a chord)
                if v in nbrs[s]:                      # closes the cycle; going on from v would leave v - s as a chord
                    if len(path) + 1 >= MIN_ATOMS and path[1] < v:        # (each cycle once: the direction with the lower second atom)
                        found.append(path + (v,))
                elif len(path) + 1 < max_size:
                    stack.append(path + (v,))
    return sorted(found, key=lambda r: (len(r), r))


def pack_rings(rings):
    """(ring_ptr int32 [Rg + 1], ring_idx int32 [ring_ptr[Rg]]) of a list of rings, each a sequence of atom indices in walking
    order.  A ring of fewer than 4 or more than AGDIFF_RING_MAX_ATOMS atoms: AgdiffLimitError; an atom twice in a ring: ValueError."""
    rings = [tuple(int(a) for a in r) for r in rings]
    for r in rings:
        if not MIN_ATOMS <= len(r) <= MAX_ATOMS:
            raise _lib.AgdiffLimitError("a ring of %d atoms: agdiff_ring_coords takes %d .. AGDIFF_RING_MAX_ATOMS = %d"
                                        % (len(r), MIN_ATOMS, MAX_ATOMS))
        if len(set(r)) != len(r):
            raise ValueError("ring %r names an atom twice" % (r,))
    ptr = np.cumsum([0] + [len(r) for r in rings]).astype(np.int32)
    return ptr, np.asarray([a for r in rings for a in r], dtype=np.int32).reshape(-1)


def unpack_rings(ring_ptr, ring_idx):
    """the list of atom tuples of a ring table"""
    ptr, idx = as_host(ring_ptr).reshape(-1), as_host(ring_idx).reshape(-1)
    return [tuple(int(a) for a in idx[ptr[r]:ptr[r + 1]]) for r in range(ptr.shape[0] - 1)]


def ring_table(item, max_size=12):
    """(ring_ptr int32 [Rg + 1], ring_idx int32 [ring_ptr[Rg]]) of an item (atom_type + its bonds): find_rings, packed."""
    return pack_rings(find_rings(np.asarray(item["atom_type"]).reshape(-1), *bonds_of(item), max_size=max_size))


def ring_scales(ring_ptr):
    """float32 [Rg]: the scale of each ring's term in the TFD, pi exp(-0.025 (N - 14)^2) for a ring of N atoms, as published."""
    size = np.diff(as_host(ring_ptr).reshape(-1).astype(np.int64)).astype(np.float64)
    return (np.pi * np.exp(-0.025 * (size - 14.0) ** 2)).astype(np.float32)


def _checked_table(ring_ptr, ring_idx):
    ptr = as_host(ring_ptr, np.int32).reshape(-1)
    idx = as_host(ring_idx, np.int32).reshape(-1)
    if ptr.shape[0] < 1 or ptr[0] != 0 or idx.shape[0] != ptr[-1]:
        raise ValueError("ring_ptr must be int32 [Rg + 1] starting at 0 and ring_idx hold ring_ptr[Rg] atoms")
    return ptr, idx


def _ring_coords(pos, ring_ptr, ring_idx, shape_too):
    """the one launch of agdiff_ring_coords: (tau, amp or None, pucker or None); amp and pucker only with shape_too"""
    import torch
    _lib.require_device_conformers(pos)
    G, n = int(pos.shape[0]), int(pos.shape[1])
    ptr, idx = _checked_table(ring_ptr, ring_idx)
    Rg = ptr.shape[0] - 1
    K = int(ptr[-1]) - 3 * Rg if Rg else 0
    new = lambda cols: torch.empty((G, cols), dtype=torch.float32, device=pos.device)
    tau, amp, pucker = new(Rg), (new(Rg) if shape_too else None), (new(max(K, 0)) if shape_too else None)
    if G and Rg:
        _lib.call("agdiff_ring_coords", pos, torch.from_numpy(ptr).to(pos.device), torch.from_numpy(idx).to(pos.device), G, n, Rg,
                  tau, amp, pucker)
    return tau, amp, pucker


def ring_coordinates(pos, ring_ptr, ring_idx):
    """agdiff_ring_coords on pos [G, n, 3] (float32, contiguous, on the GPU) and a ring table (numpy or tensors): (tau float32
    [G, Rg] in radians, amp float32 [G, Rg] in the positions' unit, pucker float32 [G, K]), K = ring_ptr[Rg] - 3 Rg: ring r's
    N - 3 numbers q_2, phi_2, ..., q_M, phi_M[, q_(N/2)] start at column ring_ptr[r] - 3 r (pucker_columns).  NaN in all of a ring's
    numbers when it names an atom outside [0, n) or a coordinate is not finite; a ring of fewer than 4 or more than
    AGDIFF_RING_MAX_ATOMS atoms: AgdiffLimitError."""
    return _ring_coords(pos, ring_ptr, ring_idx, True)


def ring_torsion_values(pos, ring_ptr, ring_idx):
    """tau alone, float32 [G, Rg]: the ring columns of the TFD's value table"""
    return _ring_coords(pos, ring_ptr, ring_idx, False)[0]


def pucker_columns(ring_ptr):
    """int [Rg + 1]: ring r's puckering numbers are the columns [c[r], c[r + 1]) of `pucker`"""
    ptr = as_host(ring_ptr).reshape(-1).astype(np.int64)
    return ptr - 3 * np.arange(ptr.shape[0])


def six_ring_theta(q2, q3):
    """atan2(q_2, q_3) in degrees, in [0, 180]: 0 and 180 the two chairs, 90 the boat / twist-boat equator"""
    return np.degrees(np.arctan2(np.asarray(q2, dtype=np.float64), np.asarray(q3, dtype=np.float64)))


def six_ring_class(q2, phi2, q3):
    """int8 codes into CLASS_NAMES for six-rings with the Cremer-Pople coordinates (q_2, phi_2 in radians, q_3): 1 chair (theta
    within 30 degrees of 0 or 180), 2 boat / 3 twist-boat (theta within 30 degrees of 90; phi_2 mod 60 degrees nearer 0 / nearer
    30), 4 half-chair/envelope (the rest); 0 where a number is NaN.  The 30-degree bands are this project's defaults."""
    q2, phi2, q3 = (np.asarray(a, dtype=np.float64) for a in (q2, phi2, q3))
    theta = six_ring_theta(q2, q3)
    with np.errstate(invalid="ignore"):
        d = np.degrees(phi2) % 60.0
        equator = np.where(np.minimum(d, 60.0 - d) <= np.abs(d - 30.0), 2, 3)
        code = np.where(np.minimum(theta, 180.0 - theta) <= 30.0, 1, np.where(np.abs(theta - 90.0) <= 30.0, equator, 4))
    return np.where(np.isnan(theta) | np.isnan(phi2), 0, code).astype(np.int8)


def ring_classes(ring_ptr, pucker):
    """int8 [G, Rg]: six_ring_class of every six-ring of a `pucker` table (numpy [G, K]); 0 for the rings of another size"""
    ptr = as_host(ring_ptr).reshape(-1).astype(np.int64)
    pk = as_host(pucker)
    col = pucker_columns(ptr)
    out = np.zeros((pk.shape[0], ptr.shape[0] - 1), dtype=np.int8)
    for r in np.nonzero(np.diff(ptr) == 6)[0]:
        out[:, r] = six_ring_class(pk[:, col[r]], pk[:, col[r] + 1], pk[:, col[r] + 2])
    return out


def main(argv=None):
    """python -m agdiff_amd.rings --samples samples_all.npz --testset test.npz --out rings.npz
    For every molecule of a finished job (agdiff_amd.driver: `pos_gen_<i>`; the bonds come from the test set) writes its rings
    `ring_ptr_<i>`, `ring_idx_<i>` and, per conformer, `ring_tau_<i>` float32 [G, Rg] (radians), `ring_amp_<i>` float32 [G, Rg],
    `ring_pucker_<i>` float32 [G, K] (ring r's q_2, phi_2, ... at column ring_ptr[r] - 3 r) and `ring_class_<i>` int8 [G, Rg]
    (1 chair, 2 boat, 3 twist-boat, 4 half-chair/envelope; 0 for the rings that are no six-rings) (+ `name_<i>`)."""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", required=True)
    ap.add_argument("--testset", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--max-size", type=int, default=12, help="the largest ring searched for (default 12)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    out, mols, total, six, chairs = {}, 0, 0, 0, 0
    for mol, item in sampled_items(args.testset, args.samples):
        i = mol["index"]
        ptr, idx = ring_table(item, max_size=args.max_size)
        pos = _lib.conformers(item["pos_gen"], num_atoms(item), args.device)
        tau, amp, pucker = (t.cpu().numpy() for t in ring_coordinates(pos, ptr, idx))
        cls = ring_classes(ptr, pucker)
        out["ring_ptr_%d" % i], out["ring_idx_%d" % i] = ptr, idx
        out["ring_tau_%d" % i], out["ring_amp_%d" % i], out["ring_pucker_%d" % i], out["ring_class_%d" % i] = tau, amp, pucker, cls
        out["name_%d" % i] = np.str_(mol["name"])
        mols += 1
        total += ptr.shape[0] - 1
        six += int((cls != 0).sum())
        chairs += int((cls == 1).sum())
    np.savez_compressed(args.out, **out)
    print("%d molecules, %d rings; %d six-ring conformations classified, %d of them chairs" % (mols, total, six, chairs))
    return out


if __name__ == "__main__":
    main()
