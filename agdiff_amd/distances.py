"""Distance-distribution MMD between the generated and the reference conformers of a molecule.

COV / MAT say how close single conformers come to single references; a run can score well there and still put every bond 3 % long.
The ConfGF / CGCF / GraphDG line (from which the reference descends through GeoDiff) therefore also reports the maximum mean
discrepancy between the interatomic-distance DISTRIBUTIONS of the two ensembles.  Both parts run on the GPU (csrc/eval.hip; there is
no CPU fallback): the fp32 distance table is what agdiff_pair_bounds writes as `dist`, the all-pairs part is agdiff_mmd_all /
agdiff_mmd_single.

  X [R][K], Y [G][K]   distances of K atom pairs in the R reference and the G generated conformers, fp32; Z = [X; Y], M = R + G
  D2(a, b)   sum_k (Z[a][k] - Z[b][k])^2, all arithmetic in fp64 from the stored fp32 values
  b          sum_{a, b} D2(a, b) / (M^2 - M): the bandwidth (computed as 2 M sum_a |Z[a] - mu|^2 / (M^2 - M), mu the column mean)
  k(a, b)    sum_{i = 0 .. 4} exp(-D2(a, b) / (b 2^(i - 2)));  k(a, a) = 5, the diagonal is included (the biased V-statistic)
  mmd2       mean_{a, b in X} k + mean_{a, b in Y} k - 2 mean_{a in X, b in Y} k, stored as fp32
             b == 0 (all rows equal): 0.  A non-finite entry in the rows / columns involved: NaN.
  "all"      one problem over the K-dimensional rows
  "single"   K one-dimensional problems, one per atom pair; reported as their mean and their median
ConfGF's "pair" mode (all pairs of columns) is not built.

    python -m agdiff_amd.distances --samples out/samples_all.npz --refs refs.npz [--with-h] [--out mmd.npz]
"""
import numpy as np

from . import _lib
from .molecule import num_atoms, reference_items
from .validity import pair_bounds

MAX_CONFS = _lib.DEFINES["AGDIFF_MMD_MAX_CONFS"]


def pair_list(atom_type, ignore_h=True):
    """int32 [K, 2]: every atom pair i < j in lexicographic order; with ignore_h only the atoms that are not hydrogens (type 1)."""
    at = np.asarray(atom_type).reshape(-1)
    idx = np.nonzero(at != 1)[0] if ignore_h else np.arange(at.shape[0])
    i, j = np.triu_indices(idx.shape[0], k=1)
    return np.stack([idx[i], idx[j]], axis=1).astype(np.int32).reshape(-1, 2)


def distance_table(pos, pairs):
    """float32 [C, K] on pos's device: the distances of `pairs` (int32 [K, 2]) in the conformers pos [C, n, 3] (float32, contiguous,
    on the GPU), as agdiff_pair_bounds computes them: in fp64 from the fp32 coordinates, rounded once."""
    K = np.asarray(pairs).reshape(-1, 2).shape[0]
    return pair_bounds(pos, pairs, np.zeros(K, dtype=np.float32), np.full(K, np.inf, dtype=np.float32), want_dist=True)[3]


def _tables(tab_ref, tab_gen):
    for t in (tab_ref, tab_gen):
        _lib.require_device_table(t, "the distance tables must be contiguous float32 [conformers, pairs] tensors on the GPU")
    R, G, K = int(tab_ref.shape[0]), int(tab_gen.shape[0]), int(tab_ref.shape[1])
    if int(tab_gen.shape[1]) != K or tab_gen.device != tab_ref.device:
        raise ValueError("both tables must hold the same pairs on the same device (got %d and %d columns)" % (K, tab_gen.shape[1]))
    if R < 1 or G < 1 or K < 1:
        raise ValueError("need at least one reference, one generated conformer and one pair (got R = %d, G = %d, K = %d)" % (R, G, K))
    return R, G, K


def mmd_all(tab_ref, tab_gen):
    """agdiff_mmd_all on tab_ref [R, K] and tab_gen [G, K] (float32, contiguous, on the GPU): (mmd2 float32 [1], bandwidth float32
    [1]) on that device."""
    import torch
    R, G, K = _tables(tab_ref, tab_gen)
    T = (R + G + 15) // 16
    dev = tab_ref.device
    scratch = torch.empty(K + 1 + 3 * (T * (T + 1) // 2), dtype=torch.float64, device=dev)
    mmd2, bw = (torch.empty(1, dtype=torch.float32, device=dev) for _ in range(2))
    _lib.call("agdiff_mmd_all", tab_ref, tab_gen, R, G, K, scratch, mmd2, bw)
    return mmd2, bw


def mmd_single(tab_ref, tab_gen):
    """agdiff_mmd_single on tab_ref [R, K] and tab_gen [G, K]: (mmd2 float32 [K], bandwidth float32 [K]), one one-dimensional problem
    per column.  More than AGDIFF_MMD_MAX_CONFS conformers in all: AgdiffLimitError."""
    import torch
    R, G, K = _tables(tab_ref, tab_gen)
    dev = tab_ref.device
    scratch = torch.empty(2 * K + (K * (R + G) + 1) // 2, dtype=torch.float64, device=dev)
    mmd2, bw = (torch.empty(K, dtype=torch.float32, device=dev) for _ in range(2))
    _lib.call("agdiff_mmd_single", tab_ref, tab_gen, R, G, K, scratch, mmd2, bw)
    return mmd2, bw


def summarise(single):
    """(mean, median, number of NaN columns) of the per-pair values, the NaN columns left out; (nan, nan, .) when none is left."""
    s = np.asarray(single, dtype=np.float64).reshape(-1)
    ok = s[~np.isnan(s)]
    if ok.size == 0:
        return float("nan"), float("nan"), int(s.size)
    return float(ok.mean()), float(np.median(ok)), int(s.size - ok.size)


def distance_mmd(item, ignore_h=True, device="cuda", want_tables=False):
    """The three MMDs of one item (atom_type [n], pos_ref and pos_gen as [C * n, 3] or [C, n, 3]: what
    evaluation.get_rmsd_confusion_matrix takes) over all pairs of its heavy atoms (of all atoms with ignore_h=False).  Returns
        all            float            "all" mmd2
        single         float32 [K]      "single" mmd2 per pair (numpy)
        single_mean, single_median      over the pairs that are not NaN
        bandwidth_all  float
        pairs          int32 [K, 2]
        n_nan_columns  int
    and, with want_tables only (two more copies to the host),
        table_ref, table_gen            the float32 distance tables [R, K], [G, K] the numbers were computed from (numpy)
    A molecule with fewer than two such atoms has no pair: all NaN, `single` empty."""
    n = num_atoms(item)
    pairs = pair_list(item["atom_type"], ignore_h)
    ref = _lib.conformers(item["pos_ref"], n, device)
    gen = _lib.conformers(item["pos_gen"], n, device)
    if ref.shape[0] < 1 or gen.shape[0] < 1:
        raise ValueError("need at least one reference and one generated conformer")
    nan = float("nan")
    if pairs.shape[0] == 0:
        res = {"all": nan, "single": np.zeros((0,), dtype=np.float32), "single_mean": nan, "single_median": nan, "bandwidth_all": nan,
               "pairs": pairs, "n_nan_columns": 0}
        tr, tg = ref.new_zeros((ref.shape[0], 0)), gen.new_zeros((gen.shape[0], 0))
    else:
        tr, tg = distance_table(ref, pairs), distance_table(gen, pairs)
        m_all, b_all = mmd_all(tr, tg)
        single = mmd_single(tr, tg)[0].cpu().numpy()
        mean, median, n_nan = summarise(single)
        res = {"all": float(m_all.item()), "single": single, "single_mean": mean, "single_median": median,
               "bandwidth_all": float(b_all.item()), "pairs": pairs, "n_nan_columns": n_nan}
    if want_tables:
        res["table_ref"], res["table_gen"] = tr.cpu().numpy(), tg.cpu().numpy()
    return res


def main(argv=None):
    """python -m agdiff_amd.distances --samples samples_all.npz --refs refs.npz [--with-h] [--out mmd.npz]
    The files of agdiff_amd.evaluation: samples `pos_gen_<i>` [G, n, 3] (agdiff_amd.driver output); refs `pos_ref_<i>` [R, n, 3] and
    `atom_type_<i>` [n].  Prints the mean and the median over the molecules of single_mean, single_median and all.  --with-h: the
    pairs run over every atom, not the heavy atoms only.  --out: per molecule `all_<i>`, `single_<i>` float32 [K], `single_mean_<i>`,
    `single_median_<i>`, `bandwidth_all_<i>`, `pairs_<i>` int32 [K, 2], `n_nan_columns_<i>`."""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", required=True)
    ap.add_argument("--refs", required=True)
    ap.add_argument("--with-h", action="store_true", help="distances between all atoms, not between heavy atoms only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    out, rows = {}, []
    for i, item in reference_items(args.refs, args.samples):
        if "pos_gen" not in item:
            continue
        res = distance_mmd(item, ignore_h=not args.with_h, device=args.device)
        rows.append([res["single_mean"], res["single_median"], res["all"]])
        out["all_" + i] = np.float32(res["all"])
        out["single_" + i] = res["single"]
        out["single_mean_" + i] = np.float64(res["single_mean"])
        out["single_median_" + i] = np.float64(res["single_median"])
        out["bandwidth_all_" + i] = np.float32(res["bandwidth_all"])
        out["pairs_" + i] = res["pairs"]
        out["n_nan_columns_" + i] = np.int32(res["n_nan_columns"])
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    print("distance MMD over %d molecules (%s)" % (rows.shape[0], "all atoms" if args.with_h else "heavy atoms"))
    print("%-14s %12s %12s" % ("", "mean", "median"))
    for name, col in zip(("single_mean", "single_median", "all"), rows.T):
        ok = col[~np.isnan(col)]
        print("%-14s %12.6f %12.6f" % (name, ok.mean() if ok.size else np.nan, np.median(ok) if ok.size else np.nan))
    if args.out:
        np.savez_compressed(args.out, **out)
    return out


if __name__ == "__main__":
    main()
