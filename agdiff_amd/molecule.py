"""What the modules that run after the sampler (evaluation, ensemble, stereo, ezbonds, torsions, validity, planarity, trajectory, distances) share on
the host: how an item's fields, atoms and bonds are read, the bonded-neighbour graph, colour refinement, the bridge search, and the item loops of
their command lines.  numpy only; the device-side counterparts (`call`, `conformers`, ...) are in _lib.py.

An item is a plain dict (or any object with the same attributes): atom_type [n] atomic numbers, its bonds as bond_index [2, e] +
bond_type [e] or edge_index + edge_type (types 1 .. 21 are bonds; the 2- / 3-hop entries of utils/transforms.py:12-71 have type
>= 22), and whatever the module at hand reads besides (pos_gen, pos_ref, perms, stereo, smiles).
"""
import numpy as np


def field(item, key):
    """item[key] of a dict, item.key of an object; None when absent."""
    return item.get(key) if isinstance(item, dict) else getattr(item, key, None)


def num_atoms(item):
    at = field(item, "atom_type")
    if at is None:
        raise KeyError("atom_type")
    return np.asarray(at).reshape(-1).shape[0]


def heavy_atoms(atom_type):
    """int32 [m]: the indices of the atoms that are not hydrogens (type 1), ascending; a molecule without one is a ValueError."""
    heavy = np.nonzero(np.asarray(atom_type).reshape(-1) != 1)[0].astype(np.int32)
    if heavy.size == 0:
        raise ValueError("molecule without heavy atoms")
    return heavy


def bonds_of(item, required=True):
    """(index [2, e], type [e]) of the item's bonds: bond_index + bond_type, else edge_index + edge_type.  Neither: a ValueError,
    or (None, None) with required=False."""
    b_idx = field(item, "bond_index") if field(item, "bond_index") is not None else field(item, "edge_index")
    b_typ = field(item, "bond_type") if field(item, "bond_type") is not None else field(item, "edge_type")
    if b_idx is None or b_typ is None:
        if required:
            raise ValueError("the item carries no bonds (bond_index + bond_type, or edge_index + edge_type)")
        return None, None
    return b_idx, b_typ


def bonded_neighbours(n, bond_index, bond_type):
    """Per atom: {neighbour: bond type} over the bonds of type 1 .. 21 of a directed or undirected bond list (the 2- / 3-hop
    entries have type >= 22 and are ignored), symmetric, without self loops.  A bond naming an atom outside [0, n): ValueError."""
    bi = np.asarray(bond_index).reshape(2, -1).astype(np.int64)
    bt = np.asarray(bond_type).reshape(-1).astype(np.int64)
    adj = [dict() for _ in range(n)]
    for (u, v), ty in zip(bi.T, bt):
        if ty <= 0 or ty >= 22 or u == v:
            continue
        if not (0 <= u < n and 0 <= v < n):
            raise ValueError("bond (%d, %d) outside the molecule's %d atoms" % (u, v, n))
        adj[int(u)][int(v)] = int(ty)
        adj[int(v)][int(u)] = int(ty)
    return adj


def refine_colours(colour, adj):
    """Colour refinement (1-WL) to a fixed point: rounds of (own colour, sorted multiset of (neighbour colour, bond type)) over
    the graph `adj` (per atom {neighbour: type}), from the initial colours `colour` (atomic numbers).  Returns a list of ints,
    after the first round numbered densely in the order of the sorted signatures.  1-WL never separates equivalent atoms."""
    colour = [int(c) for c in colour]
    for _ in range(len(colour)):
        sig = [(colour[i], tuple(sorted((colour[j], ty) for j, ty in adj[i].items()))) for i in range(len(colour))]
        ids = {s: k for k, s in enumerate(sorted(set(sig)))}
        new = [ids[s] for s in sig]
        stable = len(set(new)) == len(set(colour))
        colour = new
        if stable:
            break
    return colour


def bridges(nbrs):
    """The bridges (u, v), u < v, of an undirected graph given as sorted neighbour lists: depth-first search with low-links,
    iterative (a molecule may have thousands of atoms)."""
    n = len(nbrs)
    order, low, out, clock = [-1] * n, [0] * n, set(), 0
    for root in range(n):
        if order[root] >= 0:
            continue
        order[root] = low[root] = clock
        clock += 1
        stack = [(root, -1, 0)]
        while stack:
            i, parent, k = stack.pop()
            if k < len(nbrs[i]):
                stack.append((i, parent, k + 1))
                j = nbrs[i][k]
                if j == parent:
                    continue
                if order[j] < 0:
                    order[j] = low[j] = clock
                    clock += 1
                    stack.append((j, i, 0))
                else:
                    low[i] = min(low[i], order[j])
            elif parent >= 0:
                low[parent] = min(low[parent], low[i])
                if low[i] > order[parent]:
                    out.add((min(i, parent), max(i, parent)))
    return out


def as_host(x, dtype=None):
    """numpy from a tensor (on any device) or an array-like.  With a dtype: always a writable, C-contiguous copy of that dtype
    (the caller's array may be read-only, and what is handed to torch.from_numpy must not be)."""
    if hasattr(x, "detach"):         # a torch tensor; torch itself is not needed here
        x = x.detach().cpu().numpy()
    return np.asarray(x) if dtype is None else np.array(x, dtype=dtype, order="C")


def check_threshold(value, what):
    """float(value) of a prune threshold of the metric `what` ("RMSD", "TFD"); negative or NaN: ValueError."""
    t = float(value)
    if not t >= 0.0:
        raise ValueError("the %s threshold must be >= 0 (got %r)" % (what, value))
    return t


def sampled_items(testset_path, samples_path):
    """(mol, item) for every molecule of a test set (driver.load_testset) that has a `pos_gen_<i>` in a finished job's samples
    file: item = atom_type, pos_gen and the test set's bonds (edge_index, edge_type); mol carries name, index and the rest."""
    from .driver import load_testset
    zs = np.load(samples_path)
    for mol in load_testset(testset_path):
        if "pos_gen_%d" % mol["index"] in zs.files:
            yield mol, {"atom_type": mol["atom_type"], "pos_gen": zs["pos_gen_%d" % mol["index"]], "edge_index": mol["edge_index"],
                        "edge_type": mol["edge_type"]}


def reference_items(refs_path, samples_path):
    """(i, item) for every `pos_ref_<i>` of a references file, i as the string the key carries: item = pos_ref, atom_type, and when
    the files hold them smiles, perms, bond_index, bond_type, edge_index, edge_type (refs) and pos_gen (samples)."""
    zs, zr = np.load(samples_path), np.load(refs_path)
    for key in zr.files:
        if not key.startswith("pos_ref_"):
            continue
        i = key[len("pos_ref_"):]
        item = {"pos_ref": zr[key], "atom_type": zr["atom_type_" + i]}
        if "smiles_" + i in zr.files:
            item["smiles"] = str(zr["smiles_" + i])
        for k in ("perms", "bond_index", "bond_type", "edge_index", "edge_type"):
            if "%s_%s" % (k, i) in zr.files:
                item[k] = zr["%s_%s" % (k, i)]
        if "pos_gen_" + i in zs.files:
            item["pos_gen"] = zs["pos_gen_" + i]
        yield i, item
