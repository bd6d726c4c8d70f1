"""Handedness of sampled conformers.

The score network sees atom types, bonds and interatomic distances only, eq_transform turns its output into an O(3)-equivariant
field, and the initial positions and the noise are isotropic: the sampler draws a molecule and its mirror image with equal
probability.  For a molecule with stereocentres the mirror image is another compound.  This module finds the tetrahedral
centres of a molecular graph, takes their target parity from reference conformers (or from the user), and on the GPU
(csrc/eval.hip; there is no CPU fallback) reads every conformer's parities and inverts the wrong-handed ones:
    agdiff_chiral_verdict     signed volumes of the centres and one verdict per conformer (+1 right, -1 mirror image, 0 neither)
    agdiff_mirror_conformers  inversion through the centroid, in place

The parity of a centre is the sign of (p_b - p_a) . ((p_c - p_a) x (p_d - p_a)) over its four bonded neighbours a < b < c < d
(atom indices).  `stereo` int8 [n] holds the target parity at the centre atoms and 0 elsewhere -- a plain definition that can be
filled in from any toolkit's chirality tags.

    python -m agdiff_amd.stereo --testset test.npz --refs refs.npz --out test_stereo.npz
"""
import numpy as np

from . import _lib
from .molecule import as_host, bonded_neighbours, bonds_of, field, num_atoms, refine_colours


def tetrahedral_centres(atom_type, bond_index, bond_type):
    """(centre int32 [C], quads int32 [C, 4]): the atoms with exactly four bonded neighbours of four pairwise different colours,
    ascending, and each one's neighbours in ascending atom index.  The colours come from colour refinement (1-WL) over ALL atoms,
    hydrogens included: atomic number first, then rounds of (own colour, sorted multiset of (neighbour colour, bond type)) to a
    fixed point.  1-WL never separates equivalent atoms, so every centre reported is a true one; it may miss centres whose
    substituents differ only beyond what 1-WL sees, which fixing the global hand does not need."""
    at = np.asarray(atom_type).reshape(-1).astype(np.int64)
    n = at.shape[0]
    adj = bonded_neighbours(n, bond_index, bond_type)
    colour = refine_colours(at, adj)
    centre, quads = [], []
    for i in range(n):
        nb = sorted(adj[i])
        if len(nb) == 4 and len(set(colour[j] for j in nb)) == 4:
            centre.append(i)
            quads.append(nb)
    return np.asarray(centre, dtype=np.int32), np.asarray(quads, dtype=np.int32).reshape(-1, 4)


def signed_volumes(pos, quads):
    """float64 [K, C]: (p_b - p_a) . ((p_c - p_a) x (p_d - p_a)) of every quad in every conformer of pos [K, n, 3] (numpy)."""
    p = np.asarray(pos, dtype=np.float64)
    p = p.reshape(-1, p.shape[-2], 3)
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    a = p[:, q[:, 0]]
    u, v, w = p[:, q[:, 1]] - a, p[:, q[:, 2]] - a, p[:, q[:, 3]] - a
    return np.einsum("kci,kci->kc", u, np.cross(v, w))


def parities_from_conformers(pos, quads):
    """(target int8 [C], disagree int32 [C]) from reference conformers pos [K, n, 3], on numpy: the majority sign of each quad's
    signed volume over the K conformers -- 0 on a tie or when every volume is zero or not finite -- and the number of conformers
    on the minority side (min of the + and - counts)."""
    vol = signed_volumes(pos, quads)
    ok = np.isfinite(vol)
    plus = ((vol > 0) & ok).sum(0)
    minus = ((vol < 0) & ok).sum(0)
    return np.sign(plus - minus).astype(np.int8), np.minimum(plus, minus).astype(np.int32)


def stereo_quads(item):
    """(quads int32 [C, 4], target int8 [C]) of an item's `stereo` tags: one row per atom with stereo != 0, which must have
    exactly four bonded neighbours."""
    stereo = field(item, "stereo")
    if stereo is None:
        raise ValueError("the item carries no `stereo` tags (int8 [n]: target parity at the stereocentres, 0 elsewhere; "
                         "python -m agdiff_amd.stereo adds them to a test set from reference conformers)")
    n = num_atoms(item)
    st = np.asarray(stereo).reshape(-1)
    if st.shape[0] != n:
        raise ValueError("stereo has %d entries for %d atoms" % (st.shape[0], n))
    adj = bonded_neighbours(n, *bonds_of(item))
    quads, target = [], []
    for i in np.nonzero(st)[0]:
        nb = sorted(adj[int(i)])
        if len(nb) != 4:
            raise ValueError("stereo tag on atom %d, which has %d bonded neighbours: only four-neighbour centres are handled"
                             % (i, len(nb)))
        quads.append(nb)
        target.append(1 if st[i] > 0 else -1)
    return np.asarray(quads, dtype=np.int32).reshape(-1, 4), np.asarray(target, dtype=np.int8)


def chiral_verdict(pos, quads, target, want_vol=True):
    """agdiff_chiral_verdict on pos [G, n, 3] (float32, contiguous, on the GPU): (verdict int32 [G], vol float32 [G, C] or None).
    quads int32 [C, 4] / target int8 [C]: numpy or tensors.  Atom indices are checked here, on the host."""
    import torch
    G, n = int(pos.shape[0]), int(pos.shape[1])
    dev = pos.device
    q = as_host(quads, np.int32).reshape(-1, 4)
    t = as_host(target, np.int8).reshape(-1)
    C = q.shape[0]
    if t.shape[0] != C:
        raise ValueError("%d quads but %d targets" % (C, t.shape[0]))
    if C and (q.min() < 0 or q.max() >= n):
        raise ValueError("quads name atoms outside [0, %d)" % n)
    qt = torch.from_numpy(q).to(dev) if C else None
    tt = torch.from_numpy(t).to(dev) if C else None
    verdict = torch.empty(G, dtype=torch.int32, device=dev)
    vol = torch.empty((G, C), dtype=torch.float32, device=dev) if want_vol else None
    _lib.call("agdiff_chiral_verdict", pos, qt, tt, G, n, C, vol if (vol is not None and vol.numel()) else None, verdict)
    return verdict, vol


def mirror_conformers(pos, flags):
    """agdiff_mirror_conformers: inverts, in place, every conformer g of pos [G, n, 3] (float32, contiguous, on the GPU) with
    flags[g] != 0 through the centroid of all its atoms.  Returns pos."""
    import torch
    _lib.require_device_conformers(pos)
    f = flags.to(device=pos.device, dtype=torch.int32).contiguous()
    if f.shape != (pos.shape[0],):
        raise ValueError("flags must have one entry per conformer")
    _lib.call("agdiff_mirror_conformers", pos, f, int(pos.shape[0]), int(pos.shape[1]))
    return pos


def handedness(item, pos, device="cuda"):
    """(verdict int32 [G], vol float32 [G, C]) on the device for the conformers pos [G, n, 3] (or [G*n, 3]; numpy or tensor) of
    `item` (atom_type, bonds, stereo): + 1 every tagged centre has its target parity, - 1 every one is inverted (the conformer
    is the mirror image), 0 the centres disagree or one is flat -- a diastereomer, which reflection cannot fix."""
    quads, target = stereo_quads(item)
    return chiral_verdict(_lib.conformers(pos, num_atoms(item), device), quads, target)


def fix_handedness(item, pos):
    """Mirrors, in place, the conformers of pos [G, n, 3] (contiguous float32 tensor on the GPU) whose verdict is - 1 and returns
    the verdict (int32 [G]) as it was BEFORE mirroring: - 1 was mirrored, 0 is left as sampled, + 1 was right."""
    _lib.require_device_conformers(pos)
    n = num_atoms(item)
    if pos.shape[1] != n:
        raise ValueError("pos has %d atoms per conformer, the item %d" % (pos.shape[1], n))
    quads, target = stereo_quads(item)
    verdict, _ = chiral_verdict(pos, quads, target, want_vol=False)
    mirror_conformers(pos, (verdict < 0))
    return verdict


def main(argv=None):
    """python -m agdiff_amd.stereo --testset test.npz --refs refs.npz --out test_stereo.npz
    Copies the test set and adds `stereo_<i>` int8 [n]: at every tetrahedral centre the majority parity of the molecule's
    reference conformers (`pos_ref_<i>` [R, n, 3] of refs.npz), 0 elsewhere.  Host work only."""
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
        centre, quads = tetrahedral_centres(at, zt["edge_index_%d" % i], zt["edge_type_%d" % i])
        target, disagree = parities_from_conformers(np.asarray(zr["pos_ref_%d" % i]).reshape(-1, n, 3), quads)
        stereo = np.zeros(n, dtype=np.int8)
        stereo[centre] = target
        out["stereo_%d" % i] = stereo
        print("%s: %d tetrahedral centres, %d with disagreeing references (%d tagged)"
              % (name, centre.size, int((disagree > 0).sum()), int((target != 0).sum())))
    with open(args.out, "wb") as f:
        np.savez_compressed(f, **out)
    return out


if __name__ == "__main__":
    main()
