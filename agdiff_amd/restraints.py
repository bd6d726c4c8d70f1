"""Conformers under distance restraints: flat-bottomed windows on interatomic distances, applied while the sampler runs.

A macrocycle or staple closure (these two atoms end up 1.3-1.6 A apart), an NOE contact (closer than 5 A), a pharmacophore or
docking distance, "keep the ensemble extended" (a lower bound).  The score network sees distances only, so a window [lo, hi] on a
distance is the constraint that fits this sampler: after a step's update every violated pair is pulled the fraction `weight` of
the way onto its violated bound (csrc/eval.hip: agdiff_restrain_pairs, fp64, one wave per graph of a packed batch; there is no
CPU fallback), and the network relaxes the rest of the molecule around it in the steps that follow.  A restraint is soft: nothing
is forced after the run, and `restr_viol` says what is left.  DESIGN.md 4.18.

    restraint_arguments  the checks of epsnet.LangevinRun's keywords restraint_pairs / _lo / _hi / _weight / _start_sigma / _sweeps
    restrain_pairs       one stand-alone launch on a packed batch
    add_restraints / load_restraints   the test set's `restr_pairs_<i>`, `restr_lo_<i>`, `restr_hi_<i>`
    pack_restraints      batch-level pairs of a driver.pack_batch result
    sample_restrained    one molecule x num_samples conformers, with the reference driver's retry rule
    python -m agdiff_amd.restraints   a sampling job under the test set's restraints, or --report on a finished one

Inside a run the restraints are constraints.PairRestraints, the first entry of constraints.ORDER; the launcher's prologue, the
sampling routine and the job's skeleton are shared with torsion_restraints.py and live in constraints.py too.

The CHEMISTRY IS UNVERIFIED: nobody has run this on a trained checkpoint.  Torsion restraints are torsion_restraints.py's (a
molecule may carry both kinds); no angle restraints, no symmetry-equivalent atom mappings, no --dist-mode shard; packed
multi-molecule jobs through driver.run_job are a follow-up.
"""
import numpy as np

from . import _lib, constraints
from .molecule import as_host

MAX_SWEEPS = 16


def _pair_arrays(pairs, lo, hi):
    """(pairs int32 [R, 2], lo float32 [R], hi float32 [R]) on the host; ValueError for a pair list that is not [R, 2] or bounds of
    another length."""
    pr = as_host(pairs)
    if pr.size and (pr.ndim != 2 or pr.shape[1] != 2):
        raise ValueError("restraint pairs must have shape [R, 2], got %s" % (tuple(pr.shape),))
    if pr.size and not np.issubdtype(pr.dtype, np.integer):
        raise ValueError("restraint pairs must be atom indices (an integer array), got %s" % pr.dtype)
    pr = np.array(pr, dtype=np.int32).reshape(-1, 2)
    if lo is None or hi is None:
        raise ValueError("restraint pairs need their lower and upper bounds (hi = inf: a lower bound only)")
    lo_, hi_ = (as_host(x, np.float32).reshape(-1) for x in (lo, hi))
    if lo_.shape[0] != pr.shape[0] or hi_.shape[0] != pr.shape[0]:
        raise ValueError("%d restraint pairs but %d lower and %d upper bounds" % (pr.shape[0], lo_.shape[0], hi_.shape[0]))
    return pr, lo_, hi_


def _table(N, pairs, lo, hi, batch):
    """The by-atom table of agdiff_restrain_pairs for a batch of N atoms with sorted graph ids `batch` [N]: (rs_ptr int32 [N + 1],
    rs_idx int32 [2R], rs_lo, rs_hi float32 [2R], the largest number of restrained atoms in one graph).  ValueError for what
    validity.bounds_csr refuses (an atom outside [0, N), a == b, lo > hi, a NaN), for lo < 0 or not finite, and for a pair across two
    graphs; AgdiffLimitError for more than AGDIFF_RESTRAIN_MAX_ATOMS restrained atoms in one graph."""
    from .validity import bounds_csr
    N = int(N)
    pr, lo_, hi_ = _pair_arrays(pairs, lo, hi)
    if pr.shape[0] and not (np.isfinite(lo_) & (lo_ >= 0.0)).all():
        raise ValueError("every restraint needs a finite lower bound >= 0 (0: an upper bound only)")
    table = bounds_csr(N, pr, lo_, hi_)
    most = 0
    if pr.shape[0]:
        if batch is None:
            raise ValueError("restraints need the batch's graph ids: both atoms of a pair lie in one graph")
        b = as_host(batch).reshape(-1)
        if b.shape[0] != N:
            raise ValueError("batch has %d entries, the batch %d atoms" % (b.shape[0], N))
        if (b[pr[:, 0]] != b[pr[:, 1]]).any():
            raise ValueError("a restraint pair names atoms of two different graphs")
        has_row = np.diff(table[0]) > 0
        most = int(np.bincount(b[has_row].astype(np.int64)).max())
        if most > _lib.DEFINES["AGDIFF_RESTRAIN_MAX_ATOMS"]:
            raise _lib.AgdiffLimitError("%d restrained atoms in one graph: agdiff_restrain_pairs takes AGDIFF_RESTRAIN_MAX_ATOMS = %d"
                                        % (most, _lib.DEFINES["AGDIFF_RESTRAIN_MAX_ATOMS"]))
    return table + (most,)


def _settings(weight, start_sigma, sweeps):
    w, start = constraints.weight_and_start(
        weight, start_sigma, "the restraint weight must lie in (0, 1] (got %r): 1 puts a lone violated pair onto its bound in one sweep",
        "the restraint start sigma must be a number (inf: restrain from the first step)")
    if isinstance(sweeps, bool) or int(sweeps) != sweeps or not (0 <= int(sweeps) <= MAX_SWEEPS):
        raise ValueError("restraint sweeps must be an integer in [0, %d] (got %r)" % (MAX_SWEEPS, sweeps))
    return w, start, int(sweeps)


def restraint_arguments(N, pairs, lo, hi, batch, weight=1.0, start_sigma=float("inf"), sweeps=1):
    """(rs_ptr int32 [N + 1], rs_idx int32 [2R], rs_lo float32 [2R], rs_hi float32 [2R], most restrained atoms of one graph, weight,
    start sigma, sweeps) on the host for a batch of N atoms with graph ids `batch` [N], or None when no pairs are given (None or an
    empty list).  pairs [R, 2] hold batch-level atom indices.  ValueError: bounds without pairs, a wrong shape, an atom outside the
    batch, a == b, a pair across two graphs, lo < 0, lo > hi, a NaN or an infinite lo (hi = inf is a lower bound only), a weight
    outside (0, 1], a start sigma that is NaN, sweeps outside [0, 16].  Needs no GPU."""
    settings = _settings(weight, start_sigma, sweeps)
    if pairs is None:
        if lo is not None or hi is not None:
            raise ValueError("restraint bounds need restraint pairs [R, 2]")
        return None
    table = _table(N, pairs, lo, hi, batch)
    if table[1].shape[0] == 0:
        return None
    return table + settings


def sampler_arguments(N, batch, restraint_pairs=None, restraint_lo=None, restraint_hi=None, restraint_weight=1.0,
                      restraint_start_sigma=float("inf"), restraint_sweeps=1):
    """restraint_arguments for epsnet.LangevinRun's keywords; inside a run restraint_sweeps must be >= 1 (a run that only measures
    restrains nothing)."""
    out = restraint_arguments(N, restraint_pairs, restraint_lo, restraint_hi, batch, restraint_weight, restraint_start_sigma, restraint_sweeps)
    if int(restraint_sweeps) < 1:
        raise ValueError("restraint_sweeps must be >= 1 inside a run (got %r)" % (restraint_sweeps,))
    return out


SAMPLER_KEYWORDS = constraints.PairRestraints.KEYWORDS


def restrain_pairs(pos, pairs, lo, hi, batch, weight=1.0, sweeps=1, fixed=None, skip=None, copy_out=None, device="cuda"):
    """One agdiff_restrain_pairs launch on the packed batch `pos` [N, 3]: (pos, viol).  A contiguous float32 tensor on the GPU is
    changed IN PLACE and returned; anything else is copied to `device` first.  `pairs` [R, 2] batch-level atom indices with their
    windows `lo`, `hi` [R]; `batch` [N] sorted graph ids; fixed [N] (!= 0: the atom is not moved, its partners take the whole step),
    skip [G] (!= 0 leaves the graph alone) and copy_out (a contiguous float32 GPU tensor [N, 3] that receives the new values of the
    atoms that have a restraint) are optional.  sweeps = 0 moves nothing and only measures.  viol float32 [G] on the device: each
    graph's largest violation BEFORE the call, 0 without restraints, NaN for a graph that was left alone."""
    import torch
    pos, gp, G, N, skip = constraints.launch_prologue(pos, batch, skip, copy_out, device)
    w, _, sweeps = _settings(weight, float("inf"), sweeps)
    rs_ptr, rs_idx, rs_lo, rs_hi, most = _table(N, pairs if pairs is not None else np.zeros((0, 2), dtype=np.int32),
                                                lo if pairs is not None else [], hi if pairs is not None else [], batch)
    if fixed is not None:
        fixed = as_host(fixed).reshape(-1)
        if fixed.shape[0] != N:
            raise ValueError("fixed has %d entries, pos %d atoms" % (fixed.shape[0], N))
        fixed = torch.from_numpy(np.ascontiguousarray(fixed != 0, dtype=np.uint8)).to(pos.device)
    D = lambda x: torch.from_numpy(x).to(pos.device)
    out = torch.empty(G, dtype=torch.float32, device=pos.device)
    R2 = int(rs_idx.shape[0])
    _lib.call("agdiff_restrain_pairs", pos, gp, D(rs_ptr), D(rs_idx) if R2 else None, D(rs_lo) if R2 else None, D(rs_hi) if R2 else None,
              fixed, skip, G, N, R2, most, w, sweeps, copy_out, out)
    return pos, out


# ---- the test set's fields -------------------------------------------------------------------------------------------------
def _molecule_restraints(n, pairs, lo, hi, what):
    """One molecule's restraints checked against its n atoms (molecule-level indices): (pairs int32 [R, 2], lo, hi float32 [R])."""
    try:
        _table(n, pairs, lo, hi, np.zeros(n, dtype=np.int64))
    except ValueError as e:
        raise ValueError("%s: %s" % (what, e))
    return _pair_arrays(pairs, lo, hi)


def add_restraints(testset_in, testset_out, restraints):
    """Copy the test set `testset_in` (driver.save_testset's .npz) to `testset_out` with `restr_pairs_<i>` int32 [R, 2] (molecule-level
    atom indices), `restr_lo_<i>` and `restr_hi_<i>` float32 [R] for every molecule index i of `restraints` = {i: (pairs, lo, hi)};
    fields a molecule already had are replaced, every other field is kept.  ValueError for an index outside the test set and for
    what restraint_arguments refuses."""
    z = np.load(testset_in, allow_pickle=False)
    out = {k: z[k] for k in z.files}
    count = int(z["count"])
    for i, (pairs, lo, hi) in restraints.items():
        i = int(i)
        if not 0 <= i < count:
            raise ValueError("restraints for molecule %d, the test set has %d molecules" % (i, count))
        n = int(np.asarray(z["atom_type_%d" % i]).reshape(-1).shape[0])
        pr, lo_, hi_ = _molecule_restraints(n, pairs, lo, hi, "molecule %d" % i)
        out["restr_pairs_%d" % i], out["restr_lo_%d" % i], out["restr_hi_%d" % i] = pr, lo_, hi_
    np.savez_compressed(testset_out, **out)


def load_restraints(testset):
    """{i: (pairs int32 [R, 2], lo float32 [R], hi float32 [R])} for the molecules of the test set that carry restraints."""
    z = np.load(testset, allow_pickle=False)
    out = {}
    for i in range(int(z["count"])):
        keys = ["restr_%s_%d" % (k, i) for k in ("pairs", "lo", "hi")]
        if all(k in z.files for k in keys):
            n = int(np.asarray(z["atom_type_%d" % i]).reshape(-1).shape[0])
            out[i] = _molecule_restraints(n, *(z[k] for k in keys), what="molecule %d" % i)
    return out


def pack_restraints(packed, per_molecule):
    """Batch-level (pairs int32 [R, 2], lo float32 [R], hi float32 [R]) for a driver.pack_batch result: `per_molecule` holds, for
    every molecule of the batch in order, None or its (pairs, lo, hi) with molecule-level indices; each list once per conformer,
    shifted by the spans."""
    spans = packed["spans"]
    if len(per_molecule) != len(spans):
        raise ValueError("%d restraint lists for a batch of %d molecules" % (len(per_molecule), len(spans)))
    prs, los, his = [np.zeros((0, 2), dtype=np.int32)], [np.zeros(0, dtype=np.float32)], [np.zeros(0, dtype=np.float32)]
    for k, (r, (off, n, g)) in enumerate(zip(per_molecule, spans)):
        if r is None:
            continue
        pr, lo_, hi_ = _molecule_restraints(n, *r, what="molecule %d of the batch" % k)
        shift = off + n * np.arange(g, dtype=np.int64)
        prs.append((pr[None, :, :].astype(np.int64) + shift[:, None, None]).reshape(-1, 2).astype(np.int32))
        los.append(np.tile(lo_, g))
        his.append(np.tile(hi_, g))
    return np.concatenate(prs), np.concatenate(los), np.concatenate(his)


def _of_molecule(mol):
    """(pairs, lo, hi) a molecule dict carries as restr_pairs / restr_lo / restr_hi, or None."""
    if mol.get("restr_pairs") is None or np.asarray(mol["restr_pairs"]).size == 0:
        return None
    return mol["restr_pairs"], mol.get("restr_lo"), mol.get("restr_hi")


def measure(pos_gen, restraints, device="cuda"):
    """viol float32 [G] (numpy) of one molecule's conformers pos_gen [G, n, 3] under its (pairs, lo, hi) (molecule-level indices):
    the sweeps = 0 launch.  All zeros without restraints; NaN for a conformer with a restrained coordinate that is not finite."""
    pos = np.asarray(pos_gen, dtype=np.float32)
    G, n = pos.shape[0], pos.shape[1]
    if restraints is None or G == 0:
        return np.zeros(G, dtype=np.float32)
    packed = dict(spans=[(0, n, G)])
    pr, lo, hi = pack_restraints(packed, [restraints])
    _, viol = restrain_pairs(pos.reshape(G * n, 3), pr, lo, hi, np.repeat(np.arange(G, dtype=np.int64), n), sweeps=0, device=device)
    return viol.cpu().numpy()


# ---- sampling ------------------------------------------------------------------------------------------------------------------
def sample_restrained(model, mol, num_samples, sampler_kwargs, device, weight=1.0, start_sigma=float("inf"), sweeps=1,
                      counter_seed=None, max_retry=2, log=print):
    """`num_samples` conformers of ONE molecule in one batch (the reference driver's own granularity), under the restraints the
    molecule dict carries as restr_pairs / restr_lo / restr_hi (molecule-level indices; without them it is sampled unrestrained):
    (pos_gen float32 [G, n, 3] numpy, viol float32 [G], ok).  Under DISTANCE restraints only: torsion restraints the molecule carries as
    well (tors_quads / ...) are not applied here -- torsion_restraints.sample_restrained samples under both.  The packing, the checks
    and the retry rule are constraints.sample_restrained's.  viol: each conformer's largest violation at the end of the run (zeros
    without restraints); ok False: every attempt failed, pos_gen and viol are NaN.  Holds no core."""
    settings = dict(weight=weight, start_sigma=start_sigma, sweeps=sweeps)
    res = constraints.sample_restrained(model, mol, num_samples, sampler_kwargs, device, pairs=settings, counter_seed=counter_seed,
                                        max_retry=max_retry, log=log)
    viol = res["restraint_viol"] if "restraint_viol" in res else constraints.no_violation(int(num_samples), res["ok"])
    return res["pos"], viol, res["ok"]


def build_parser():
    return constraints.job_parser(main.__doc__, "test set with restr_pairs_<i> / restr_lo_<i> / restr_hi_<i> (add_restraints)",
                                  "the fraction of the way a lone violated pair is moved onto its bound per sweep, in (0, 1]",
                                  extra=[("--sweeps", dict(type=int, default=1, help="Jacobi sweeps per step, 1 .. 16"))])


def main(argv=None):
    """python -m agdiff_amd.restraints --ckpt ckpt.pt --testset test.npz --out out/ [--num-confs 2x --n-steps 5000 --w-global 1.0
        --global-start-sigma 0.5 --clip 1000 --weight 1.0 --start-sigma inf --sweeps 1 --seed 2021 --noise default|counter
        --precision ... --start-idx --end-idx --trust-ckpt]
    samples every molecule of the range, ONE molecule per batch, under the restraints the test set carries for it (a molecule
    without restraints is sampled unrestrained, so the output is a complete job), and writes out/samples_all.npz: `pos_gen_<i>`
    [G, n, 3], `name_<i>` and `restr_viol_<i>` float32 [G], each conformer's largest violation on the saved positions (zeros for a
    molecule without restraints).  The post-sampling modules run on that file unchanged.
    python -m agdiff_amd.restraints --report --samples samples_all.npz --testset test.npz --out viol.npz
    measures a finished job: `restr_viol_<i>` for every molecule of the samples."""
    args = build_parser().parse_args(argv)
    own = load_restraints(args.testset)

    def check():
        _settings(args.weight, args.start_sigma, args.sweeps)
        if args.sweeps < 1:
            raise SystemExit("--sweeps must be >= 1")

    def attach(m):
        if m["index"] in own:
            m["restr_pairs"], m["restr_lo"], m["restr_hi"] = own[m["index"]]

    def sample(model, m, G, kw, device, counter_seed):
        pos, viol, ok = sample_restrained(model, m, G, kw, device, weight=args.weight, start_sigma=args.start_sigma, sweeps=args.sweeps,
                                          counter_seed=counter_seed)
        return dict(pos_gen=pos, restr_viol=viol), ok

    return constraints.restrained_job(args, own, check, attach, sample,
                                      lambda i, pos_gen: dict(restr_viol=measure(pos_gen, own.get(i), device=args.device)),
                                      ("restr_viol", "distance restraints",
                                       "largest violation left %.4f A, median of the molecules' largest %.4f A"))


if __name__ == "__main__":
    main()
