"""COV / MAT evaluation of generated conformers -- the step after the sampling path, mirroring
the reference's utils/evaluation/covmat.py:16-165 (get_rmsd_confusion_matrix, evaluate_conf, CovMatEvaluator,
print_covmat_results) without rdkit / PyG / easydict.

The RMSD confusion matrix [references x generated] is computed on the GPU (agdiff_rmsd_matrix, csrc/eval.hip:
Kabsch / Horn RMSD with proper rotations, minimum over atom mappings); so are its row / column minima.
There is no CPU fallback.

Data items are plain dicts (the reference uses PyG Data objects with an rdkit molecule):
    pos_ref [R*n, 3] or [R, n, 3], pos_gen [G*n, 3] or [G, n, 3], atom_type [n] (atomic numbers; hydrogens = 1 are
    removed like utils/chem.py:133-137 does with RemoveHs), smiles (optional; "." marks a disconnected molecule),
    bond_index [2, e] + bond_type [e] (or edge_index / edge_type; 2-/3-hop entries are ignored): the molecule's bonds, from
    which the heavy-atom self-matches GetBestRMS minimises over are enumerated here (heavy_atom_automorphisms) -- or
    perms [P, m]: those matches given directly.  With neither only the identity mapping is tried and symmetric molecules
    get an UPPER BOUND of GetBestRMS (COV a lower bound, MAT an upper bound).
Force-field relaxation (use_force_field=True -> rdkit MMFF) is not available.
"""
import numpy as np

from . import _lib
from .config import Config
from .molecule import bonded_neighbours, bonds_of, field, heavy_atoms, num_atoms, reference_items, refine_colours


def heavy_atom_automorphisms(atom_type, bond_index, bond_type, max_perms=65536):
    """The atom mappings rdkit's GetBestRMS minimises over (utils/chem.py:133-137, covmat.py:16-35): every match of the
    hydrogen-free molecule onto itself, i.e. every automorphism of its heavy-atom graph that keeps atomic numbers and bond
    types (rdkit: `RemoveHs(mol).GetSubstructMatches(RemoveHs(mol), uniquify=False)`; a molecule used as a query matches
    atoms by atomic number and bonds by type, aromatic with aromatic).  Returns int32 [P, m] over the heavy atoms in
    ascending index order (row 0 is the identity): perms[p][k] = image of heavy atom k.
      atom_type  [n] atomic numbers (hydrogens = 1 are dropped)
      bond_index [2, e], bond_type [e]  directed or undirected bond list; entries with type >= 22 (the 2-/3-hop edges of
                 utils/transforms.py:12-71) and bonds to hydrogens are ignored
    Colour refinement (1-WL over atom type and typed neighbourhoods) partitions the atoms first; a backtracking search then
    maps atoms class by class, checking every bond to the atoms already placed.  Raises if the group has more than
    `max_perms` elements (rdkit's own cap, maxMatches, is 1e6)."""
    at = np.asarray(atom_type).reshape(-1).astype(np.int64)
    heavy = heavy_atoms(at)
    m = int(heavy.size)
    new_id = {int(h): k for k, h in enumerate(heavy)}
    full = bonded_neighbours(at.shape[0], bond_index, bond_type)
    adj = [{new_id[j]: ty for j, ty in full[h].items() if j in new_id} for h in heavy]     # the heavy-atom graph
    colour = refine_colours(at[heavy], adj)
    # visiting order: breadth first from the rarest colour class, so that every atom after the first of its component has
    # a placed neighbour to be checked against
    count = {c: colour.count(c) for c in set(colour)}
    order, seen = [], [False] * m
    for start in sorted(range(m), key=lambda i: (count[colour[i]], i)):
        if seen[start]:
            continue
        queue = [start]
        seen[start] = True
        while queue:
            i = queue.pop(0)
            order.append(i)
            for j in sorted(adj[i], key=lambda j: (count[colour[j]], j)):
                if not seen[j]:
                    seen[j] = True
                    queue.append(j)
    placed_nbrs = []                                  # for order[k]: its neighbours among order[:k]
    pos_in_order = {a: k for k, a in enumerate(order)}
    for k, i in enumerate(order):
        placed_nbrs.append([(j, ty) for j, ty in adj[i].items() if pos_in_order[j] < k])
    by_colour = {}
    for i in range(m):
        by_colour.setdefault(colour[i], []).append(i)
    perms, image, used = [], [-1] * m, [False] * m

    def place(k):
        if k == m:
            perms.append(list(image))
            if len(perms) > max_perms:
                raise ValueError("more than %d heavy-atom self-matches; pass a larger max_perms" % max_perms)
            return
        i = order[k]
        nb = placed_nbrs[k]
        if nb:          # candidates: the neighbours of an already placed neighbour's image
            j0, ty0 = nb[0]
            cands = [c for c, ty in adj[image[j0]].items() if ty == ty0]
        else:
            cands = by_colour[colour[i]]
        for c in sorted(cands):
            if used[c] or colour[c] != colour[i] or len(adj[c]) != len(adj[i]):
                continue
            if any(adj[c].get(image[j]) != ty for j, ty in nb):
                continue
            image[i], used[c] = c, True
            place(k + 1)
            image[i], used[c] = -1, False

    import sys
    lim = sys.getrecursionlimit()
    if lim < m + 100:
        sys.setrecursionlimit(m + 100)
    try:
        place(0)
    finally:
        sys.setrecursionlimit(lim)
    out = np.asarray(perms, dtype=np.int32).reshape(-1, m)
    ident = np.nonzero((out == np.arange(m)[None, :]).all(1))[0]
    if ident.size and ident[0] != 0:                  # identity first
        out[[0, ident[0]]] = out[[ident[0], 0]]
    return out


def selection_of(data):
    """What the RMSD of one item runs over (shared with agdiff_amd.ensemble): (atom_type [n], heavy-atom indices int32 [m],
    atom mappings int32 [P, m] or None).  The mappings are the item's `perms`, or -- when it carries its bonds (bond_index +
    bond_type, or edge_index + edge_type) -- the molecule's own symmetry as GetBestRMS finds it (heavy_atom_automorphisms);
    None = the identity only."""
    at = np.asarray(data["atom_type"]).reshape(-1)
    heavy = heavy_atoms(at)
    m = int(heavy.size)
    perms = field(data, "perms")
    if perms is None:       # the molecule's own symmetry, as GetBestRMS finds it, when the item carries its bonds
        b_idx, b_typ = bonds_of(data, required=False)
        if b_idx is not None:
            perms = heavy_atom_automorphisms(at, b_idx, b_typ)
    if perms is None:
        return at, heavy, None
    pa = np.ascontiguousarray(np.asarray(perms, dtype=np.int32).reshape(-1, m))
    if pa.min() < 0 or pa.max() >= m or not all(np.array_equal(np.sort(r), np.arange(m)) for r in pa):
        raise ValueError("perms must hold permutations of the %d heavy atoms" % m)
    return at, heavy, pa


def selection_on_device(data, device):
    """selection_of(data) as the RMSD entry points take it: (atom_type [n], heavy-atom index tensor int32 [m], P, mappings tensor
    int32 [P, m]) on `device`; (..., 0, None) = the identity only."""
    import torch
    at, heavy, pa = selection_of(data)
    idx = torch.from_numpy(heavy).to(device)
    if pa is None:
        return at, idx, 0, None
    return at, idx, pa.shape[0], torch.from_numpy(pa).to(device)


def get_rmsd_confusion_matrix(data, useFF=False, device="cuda", hands=False):
    """covmat.py:16-35.  Returns a float32 torch tensor [num_ref, num_gen] on `device`.
    hands=True: (proper, mirror) -- `proper` is that matrix bit for bit, `mirror` the same quantity for every generated conformer's
    mirror image (agdiff_rmsd_matrix_hands: one diagonalisation gives both).  The sampler draws either hand with equal
    probability; min(proper, mirror) is what the run would score were handedness free."""
    import torch
    if useFF:
        raise NotImplementedError("MMFF relaxation needs rdkit (covmat.py:27-29); not available here")
    n = num_atoms(data)
    ref = _lib.conformers(data["pos_ref"], n, device)
    gen = _lib.conformers(data["pos_gen"], n, device)
    _, idx, P, pt = selection_on_device(data, device)
    m = idx.shape[0]
    R, G = ref.shape[0], gen.shape[0]
    out = torch.empty((R, G), dtype=torch.float32, device=device)
    mirror = torch.empty((R, G), dtype=torch.float32, device=device) if hands else None
    scratch = torch.empty((R + G) * (3 * m + 1), dtype=torch.float32, device=device)
    _lib.call("agdiff_rmsd_matrix_hands" if hands else "agdiff_rmsd_matrix", ref, gen, idx, pt, R, G, n, m, P, scratch,
              *((out, mirror) if hands else (out,)))
    return (out, mirror) if hands else out


def get_tfd_confusion_matrix(data, hands=False, device="cuda", weights=None, rings=False):
    """The confusion matrix of get_rmsd_confusion_matrix with the torsion fingerprint deviation (agdiff_amd.torsions: the mean
    circular difference of the rotatable bonds' dihedrals, in [0, 1], minimised over the molecule's symmetry) in the RMSD's place:
    float32 [num_ref, num_gen] on `device`.  The item must carry its bonds.  hands=True: (proper, mirror), mirror being the TFD
    of every generated conformer's mirror image (a reflection negates every dihedral).  rings=True: with the molecule's rings as
    terms behind the rotatable bonds (agdiff_amd.rings; a reflection leaves a ring's value as it is)."""
    from .torsions import tfd_matrix
    if rings:                # (passed only when set: without it this is the call it was before)
        return tfd_matrix(data, hands=hands, weights=weights, device=device, rings=True)
    return tfd_matrix(data, hands=hands, weights=weights, device=device)


TFD_THRESHOLDS = np.arange(1, 61) / 100.0            # 0.01 .. 0.60: the TFD lies in [0, 1], 0.2 being the usual "same conformer"


def matrix_minima(confusion):
    """(rmsd_ref_min [R], rmsd_gen_min [G]) of a confusion matrix on the GPU (covmat.py:135-136)."""
    import torch
    c = confusion.contiguous()
    R, G = c.shape
    rmin = torch.empty(R, dtype=torch.float32, device=c.device)
    gmin = torch.empty(G, dtype=torch.float32, device=c.device)
    _lib.call("agdiff_matrix_minima", c, R, G, rmin, gmin)
    return rmin, gmin


def evaluate_conf(data, useFF=False, threshold=0.5):
    """covmat.py:38-41: (coverage at `threshold`, mean of the references' smallest RMSD)."""
    rmin, _ = matrix_minima(get_rmsd_confusion_matrix(data, useFF=useFF))
    rmin = rmin.cpu().numpy().astype(np.float64)
    return (rmin <= threshold).mean(), rmin.mean()


def scores_from_minima(ref_min, gen_min, thresholds):
    """covmat.py:137-153 for one molecule."""
    thresholds = np.asarray(thresholds).flatten()
    ref_min, gen_min = np.asarray(ref_min, dtype=np.float64), np.asarray(gen_min, dtype=np.float64)
    covr = (ref_min.reshape(-1, 1) <= thresholds.reshape(1, -1)).mean(0, keepdims=True)
    covp = (gen_min.reshape(-1, 1) <= thresholds.reshape(1, -1)).mean(0, keepdims=True)
    return covr, ref_min.mean(), covp, gen_min.mean()


def print_covmat_results(results, print_fn=print):
    """covmat.py:44-74 (a dict of columns instead of a pandas DataFrame; same numbers, same MAT lines)."""
    cols = {
        "COV-R_mean": np.mean(results.CoverageR, 0), "COV-R_median": np.median(results.CoverageR, 0),
        "COV-R_std": np.std(results.CoverageR, 0),
        "COV-P_mean": np.mean(results.CoverageP, 0), "COV-P_median": np.median(results.CoverageP, 0),
        "COV-P_std": np.std(results.CoverageP, 0),
    }
    head = "%9s " % "" + " ".join("%12s" % c for c in cols)
    rows = ["%9.2f " % t + " ".join("%12.6f" % cols[c][k] for c in cols) for k, t in enumerate(results.thresholds)]
    print_fn("\n" + "\n".join([head] + rows))
    print_fn("MAT-R_mean: %.4f | MAT-R_median: %.4f | MAT-R_std %.4f"
             % (np.mean(results.MatchingR), np.median(results.MatchingR), np.std(results.MatchingR)))
    print_fn("MAT-P_mean: %.4f | MAT-P_median: %.4f | MAT-P_std %.4f"
             % (np.mean(results.MatchingP), np.median(results.MatchingP), np.std(results.MatchingP)))
    return cols


class CovMatEvaluator(object):
    """covmat.py:77-165.  `num_workers` is accepted and ignored: the confusion matrices come from the GPU.
    either_hand=True: the results also carry `either_hand`, the same five fields computed from min(proper, mirror) -- every
    generated conformer scored as the better of itself and its mirror image (get_rmsd_confusion_matrix(hands=True)) -- and
    `mirror_nearest`, per molecule the fraction of generated conformers whose nearest reference is reached through the mirror
    image.  No stereo tags are needed: it shows what handedness costs a run.  `confusion_fn` must then return (proper, mirror).
    metric="tfd": the same reductions and table over get_tfd_confusion_matrix; the thresholds then default to 0.01 .. 0.60 in
    steps of 0.01 (for the RMSD, as in the reference, 0.05 .. 3.00 Angstrom in steps of 0.05).  tfd_rings=True: with the rings as
    terms of the TFD (get_tfd_confusion_matrix(rings=True))."""

    def __init__(self, num_workers=8, use_force_field=False, thresholds=None, ratio=2,
                 filter_disconnected=True, print_fn=print, confusion_fn=None, either_hand=False, metric="rmsd", tfd_rings=False):
        if use_force_field:
            raise NotImplementedError("MMFF relaxation needs rdkit; not available here")
        if metric not in ("rmsd", "tfd"):
            raise ValueError("metric must be 'rmsd' or 'tfd' (got %r)" % (metric,))
        if thresholds is None:
            thresholds = np.arange(0.05, 3.05, 0.05) if metric == "rmsd" else TFD_THRESHOLDS
        self.metric = metric
        if tfd_rings and metric != "tfd":
            raise ValueError("tfd_rings goes with metric='tfd'")
        self.tfd_rings = bool(tfd_rings)
        self._confusion = get_rmsd_confusion_matrix if metric == "rmsd" else get_tfd_confusion_matrix
        if self.tfd_rings:
            self._confusion = lambda data, hands=False: get_tfd_confusion_matrix(data, hands=hands, rings=True)
        self.num_workers = num_workers
        self.use_force_field = use_force_field
        self.thresholds = np.array(thresholds).flatten()
        self.ratio = ratio
        self.filter_disconnected = filter_disconnected
        self.print_fn = print_fn
        # hook for callers that already hold the matrices (and for CPU tests of the filtering / reductions)
        self.confusion_fn = confusion_fn
        self.either_hand = either_hand

    def __call__(self, packed_data_list, start_idx=0):
        filtered = []
        for data in packed_data_list:
            if "pos_gen" not in data or "pos_ref" not in data:
                continue
            if self.filter_disconnected and ("." in data.get("smiles", "")):
                continue
            n = num_atoms(data)
            ref = _lib.conformers(data["pos_ref"], n)
            gen = _lib.conformers(data["pos_gen"], n)
            num_gen = ref.shape[0] * self.ratio
            if gen.shape[0] < num_gen:
                continue
            filtered.append(dict(data, pos_ref=ref, pos_gen=gen[:num_gen]))
        filtered = filtered[start_idx:]
        self.print_fn("Filtered: %d / %d" % (len(filtered), len(packed_data_list)))
        covr_scores, matr_scores, covp_scores, matp_scores = [], [], [], []
        either, mirror_nearest = ([], [], [], []), []
        for data in filtered:
            if self.either_hand:
                if self.confusion_fn is not None:
                    cm, cmm = (np.asarray(c) for c in self.confusion_fn(data))
                    ref_min, gen_min, mir_min = cm.min(-1), cm.min(0), cmm.min(0)
                    both = np.minimum(cm, cmm)
                    e_ref_min, e_gen_min = both.min(-1), both.min(0)
                else:
                    import torch
                    proper, mirror = self._confusion(data, hands=True)
                    rmin, gmin = matrix_minima(proper)
                    _, mmin = matrix_minima(mirror)
                    ermin, egmin = matrix_minima(torch.minimum(proper, mirror))
                    ref_min, gen_min, mir_min = rmin.cpu().numpy(), gmin.cpu().numpy(), mmin.cpu().numpy()
                    e_ref_min, e_gen_min = ermin.cpu().numpy(), egmin.cpu().numpy()
                for acc, v in zip(either, scores_from_minima(e_ref_min, e_gen_min, self.thresholds)):
                    acc.append(v)
                mirror_nearest.append(float((mir_min < gen_min).mean()))
            elif self.confusion_fn is not None:
                cm = np.asarray(self.confusion_fn(data))
                ref_min, gen_min = cm.min(-1), cm.min(0)
            else:
                rmin, gmin = matrix_minima(self._confusion(data))
                ref_min, gen_min = rmin.cpu().numpy(), gmin.cpu().numpy()
            covr, matr, covp, matp = scores_from_minima(ref_min, gen_min, self.thresholds)
            covr_scores.append(covr); matr_scores.append(matr); covp_scores.append(covp); matp_scores.append(matp)
        table = lambda covr, matr, covp, matp: {
            "CoverageR": np.vstack(covr) if covr else np.zeros((0, self.thresholds.shape[0])),
            "MatchingR": np.array(matr),
            "thresholds": self.thresholds,
            "CoverageP": np.vstack(covp) if covp else np.zeros((0, self.thresholds.shape[0])),
            "MatchingP": np.array(matp),
        }
        res = Config(table(covr_scores, matr_scores, covp_scores, matp_scores))
        if self.either_hand:
            res["either_hand"] = Config(table(*either))
            res["mirror_nearest"] = np.array(mirror_nearest)
        return res

    def close(self):
        pass


def ez_report(samples_path, tags_path, device="cuda", print_fn=print):
    """{i: share}: for every molecule i with `pos_gen_<i>` in the samples file and `ez_quads_<i>` + `ez_<i>` (and atom_type_<i>, its
    bonds) in the tags file -- a test set or a references file -- the share of generated conformers with at least one tagged double
    bond of the wrong E/Z parity (agdiff_amd.ezbonds.wrong_share: the check only), one printed line each."""
    from .ezbonds import wrong_share
    zs, zt = np.load(samples_path), np.load(tags_path)
    shares = {}
    for key in sorted((k for k in zt.files if k.startswith("ez_quads_")), key=lambda k: int(k[len("ez_quads_"):])):
        i = key[len("ez_quads_"):]
        if "ez_" + i not in zt.files or "pos_gen_" + i not in zs.files:
            continue
        item = {"atom_type": zt["atom_type_" + i], "ez_quads": zt[key], "ez": zt["ez_" + i], "pos_gen": zs["pos_gen_" + i]}
        for k in ("bond_index", "bond_type", "edge_index", "edge_type"):
            if "%s_%s" % (k, i) in zt.files:
                item[k] = zt["%s_%s" % (k, i)]
        if not np.asarray(item["ez"]).any():
            continue
        shares[int(i)] = wrong_share(item, device=device)
        name = str(zt["name_" + i]) if "name_" + i in zt.files else "mol" + i
        print_fn("%s: %d tagged double bonds, %.4f of %d generated conformers have one with the wrong E/Z parity"
                 % (name, int((np.asarray(item["ez"]) != 0).sum()), shares[int(i)], np.asarray(item["pos_gen"]).reshape(-1, item["atom_type"].shape[0], 3).shape[0]))
    return shares


def main(argv=None):
    """python -m agdiff_amd.evaluation --samples samples_all.npz --refs refs.npz
    samples: `pos_gen_<i>` [G, n, 3] (agdiff_amd.driver output); refs: `pos_ref_<i>` [R, n, 3], `atom_type_<i>` [n],
    optional `smiles_<i>`, `bond_index_<i>` + `bond_type_<i>` (symmetry-aware RMSD) or `perms_<i>` [P, m].  Prints the COV / MAT table of the reference's eval_covmat.py.
    --either-hand: then a second table, labelled "either hand", from min(proper, mirror) -- every generated conformer scored as the
    better of itself and its mirror image -- and the fraction of generated conformers whose nearest reference is reached through
    the mirror image.
    --metric tfd: the tables over the torsion fingerprint deviation (agdiff_amd.torsions; the refs must carry the bonds) at the
    thresholds 0.01 .. 0.60 instead of the heavy-atom RMSD."""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--samples", required=True)
    ap.add_argument("--refs", required=True)
    ap.add_argument("--ratio", type=int, default=2)
    ap.add_argument("--either-hand", action="store_true",
                    help="also print the table computed from min(proper, mirror): what the run would score were handedness free")
    ap.add_argument("--metric", default="rmsd", choices=["rmsd", "tfd"],
                    help="'tfd': COV / MAT over the torsion fingerprint deviation (thresholds 0.01 .. 0.60) instead of the RMSD")
    ap.add_argument("--tfd-rings", action="store_true",
                    help="with --metric tfd: the rings are terms of the TFD too (agdiff_amd.rings)")
    ap.add_argument("--ez-report", action="store_true",
                    help="also print, per molecule with E/Z tags (ez_quads_<i> + ez_<i>: agdiff_amd.ezbonds), the share of generated "
                         "conformers with a double bond of the wrong parity; the tags and bonds are read from --testset, or from --refs "
                         "without one; the check only, the COV / MAT numbers do not change")
    ap.add_argument("--testset", default=None, help="with --ez-report: the test set that carries the tags (default: --refs)")
    args = ap.parse_args(argv)
    items = [item for _, item in reference_items(args.refs, args.samples)]
    res = CovMatEvaluator(ratio=args.ratio, either_hand=args.either_hand, metric=args.metric, tfd_rings=args.tfd_rings)(items)
    print_covmat_results(res)
    if args.ez_report:
        res.ez_wrong = ez_report(args.samples, args.testset or args.refs)
    if args.either_hand:
        print("\neither hand (every generated conformer scored as the better of itself and its mirror image):")
        print_covmat_results(res.either_hand)
        print("nearest reference reached through the mirror image: %.4f of the generated conformers (mean over %d molecules)"
              % (float(np.mean(res.mirror_nearest)) if len(res.mirror_nearest) else float("nan"), len(res.mirror_nearest)))
    return res


if __name__ == "__main__":
    main()
