"""What a sampling run does to the positions after a step's update: the constraints of epsnet.LangevinRun, as objects in one ordered
table, and what their stand-alone launchers and their jobs share.

    PairRestraints / TorsionRestraints / CoreHold   one constraint of a run each (restraints.py, torsion_restraints.py, core.py)
    ORDER, build       the order they run in, and the constraints a run's keywords ask for
    weight_and_start   the check of a constraint's weight and start sigma
    launch_prologue    what hold_core, restrain_pairs and restrain_torsions do before their launch
    sample_restrained  one molecule x num_samples conformers under the restraints its dict carries
    job_parser / restrained_job   the command line and the job of python -m agdiff_amd.restraints / .torsion_restraints

A constraint is built on the host from the sampler's keywords (from_keywords: every check, no GPU), attached to a run once (attach:
tables to the device, NaN-filled outputs, the ctypes arguments of its launch) and then called by the run: after_update after every
step's update, measure after the last one, collect in finish().  A new kind is one class here and one entry of ORDER.  DESIGN.md 4.16.
"""
import ctypes
import math
import os

import numpy as np

from . import _lib
from .molecule import as_host


def weight_and_start(weight, start_sigma, weight_text, start_text):
    """(weight, start sigma) as floats: ValueError(weight_text % (weight,)) for a weight outside (0, 1] (a NaN included),
    ValueError(start_text) for a start sigma that is NaN."""
    w = float(weight)
    if not (0.0 < w <= 1.0):
        raise ValueError(weight_text % (weight,))
    start = float(start_sigma)
    if math.isnan(start):
        raise ValueError(start_text)
    return w, start


class _Constraint:
    """The gate every constraint shares: it acts after the update of a step with sigma < start, and after the LAST step of the
    schedule whatever sigma says.  A subclass has KEYWORDS, from_keywords, attach, launch(run, copy_out, last) and collect."""

    def _attach(self, run, fn, tensors):
        """Host arrays (None stays None) -> the device, kept alive with the launch's entry point; a NaN-filled float32 output per
        call of _output; the pointers every launch of a run shares."""
        import torch
        self._fn = getattr(run.lib, fn), fn
        self._keep = [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(run.pos.device) for x in tensors]
        # skipped: the graphs the update kernels have quarantined, which carry a placeholder (element 0 is the "any graph" flag)
        self._skip = ctypes.c_void_p(run.ws.nan_flag.data_ptr() + 4)
        return [_lib.ptr(x) for x in self._keep]

    def _output(self, run, size):
        import torch
        out = torch.full((int(size),), float("nan"), dtype=torch.float32, device=run.pos.device)
        self._keep.append(out)
        return out

    def _launch(self, changes):
        """The prebuilt launch (self._args, in the entry point's order) on the current stream, with the arguments that vary between
        two launches ({position: value}) put in."""
        a = self._args
        for i, v in changes.items():
            a[i] = v
        a[-1] = _lib.stream_ptr()
        _lib.check(self._fn[0](*a), self._fn[1])

    def after_update(self, run, k, sigma, last):
        """After the update of step k (launch-by-launch path only): over run.pos and the frame the update has just written."""
        if last or sigma < self.start:
            self.launch(run, run._traj_row(k), last)

    def measure(self, run):
        """After the closing launches of the last step: what is left in what the run returns."""


class PairRestraints(_Constraint):
    """Distance restraints (restraints.py): restraint_sweeps Jacobi sweeps of agdiff_restrain_pairs per gated step, at
    the given weight on the last step too (a restraint is soft); the atoms of a held core stay where they are (fixed)."""
    KEYWORDS = ("restraint_pairs", "restraint_lo", "restraint_hi", "restraint_weight", "restraint_start_sigma", "restraint_sweeps")

    @classmethod
    def from_keywords(cls, N, batch, bond_index, bond_type, num_graphs, frozen, **kw):
        from .restraints import sampler_arguments
        args = sampler_arguments(N, batch, **kw)
        return None if args is None else cls(args, frozen)

    def __init__(self, args, fixed):
        self.table, (self.most, self.weight, self.start, self.sweeps), self.fixed = args[:4], args[4:], fixed

    def attach(self, run):
        rs_ptr, rs_idx, rs_lo, rs_hi, fixed = self._attach(run, "agdiff_restrain_pairs", self.table + (self.fixed,))
        self.viol = self._output(run, run.topo.G)
        self._args = [run.pos_p, _lib.ptr(run.topo.graph_ptr), rs_ptr, rs_idx, rs_lo, rs_hi, fixed, self._skip, run.topo.G, run.topo.N,
                      int(self.table[1].shape[0]), self.most, self.weight, self.sweeps, None, _lib.ptr(self.viol), None]

    def launch(self, run, copy_out, last=False):
        self._launch({13: self.sweeps, 14: copy_out})

    def measure(self, run):
        self._launch({13: 0, 14: None})

    def collect(self, run, bad):
        run.restraint_viol = self.viol.cpu()
        run.restraint_viol[bad] = float("nan")                           # (also a graph that left the range at the very last poll)


class TorsionRestraints(_Constraint):
    """Torsion restraints (torsion_restraints.py): one agdiff_restrain_torsions launch per gated step, at the given
    weight on the last step too; the sides it turns hold no atom of a held core (frozen)."""
    KEYWORDS = ("torsion_quads", "torsion_target", "torsion_tol", "torsion_sides", "torsion_weight", "torsion_start_sigma")

    @classmethod
    def from_keywords(cls, N, batch, bond_index, bond_type, num_graphs, frozen, **kw):
        from .torsion_restraints import sampler_arguments
        args = sampler_arguments(N, batch, bond_index=bond_index, bond_type=bond_type, frozen=frozen, num_graphs=num_graphs, **kw)
        if args is not None and args[4] is None:
            raise ValueError("torsion restraints need the batch's bonds (bond_index, bond_type) or a side table (torsion_sides)")
        return None if args is None else cls(args)

    def __init__(self, args):
        self.tr_ptr, self.quads, self.centre, self.half, (self.side_row, self.side_ptr, self.side_idx), self.weight, self.start = args

    def attach(self, run):
        table = self._attach(run, "agdiff_restrain_torsions", (self.tr_ptr, self.quads, self.centre, self.half, self.side_row, self.side_ptr,
                                                               self.side_idx if self.side_idx.size else None))
        T = int(self.quads.shape[0])
        self.angle, self.viol = self._output(run, T), self._output(run, run.topo.G)
        self._args = [run.pos_p, _lib.ptr(run.topo.graph_ptr)] + table + [self._skip, run.topo.G, run.topo.N, T, int(self.side_ptr.shape[0]) - 1,
                                                                          self.weight, 1, None, _lib.ptr(self.angle), _lib.ptr(self.viol), None]

    def launch(self, run, copy_out, last=False):
        self._launch({15: 1, 16: copy_out})

    def measure(self, run):
        self._launch({15: 0, 16: None})

    def collect(self, run, bad):
        import torch
        run.torsion_viol, run.torsion_angle = self.viol.cpu(), self.angle.cpu()
        run.torsion_viol[bad] = float("nan")
        graph_of = np.repeat(np.arange(self.tr_ptr.shape[0] - 1), np.diff(self.tr_ptr))
        run.torsion_angle[bad[torch.from_numpy(graph_of)]] = float("nan")


class CoreHold(_Constraint):
    """The rigid core hold (core.py): one agdiff_hold_core launch per gated step, blended by core_weight; after the
    last step with weight 1, whatever core_weight says: what the run returns holds the core exactly.  Nothing to measure afterwards:
    that launch leaves core_dev, how far the last step had pulled each core out of shape."""
    KEYWORDS = ("core_pos", "core_select", "core_weight", "core_start_sigma")

    @classmethod
    def from_keywords(cls, N, batch, bond_index, bond_type, num_graphs, frozen, core_pos=None, core_select=None, **kw):
        from .core import core_arguments
        args = core_arguments(N, core_pos, core_select, **kw)
        return None if args is None else cls(*args)

    def __init__(self, template, select, weight, start):
        self.template, self.select, self.weight, self.start = template, select, weight, start

    def attach(self, run):
        tpl, sel = self._attach(run, "agdiff_hold_core", (self.template, self.select))
        self.dev = self._output(run, run.topo.G)
        self._args = [run.pos_p, tpl, sel, _lib.ptr(run.topo.graph_ptr), self._skip, run.topo.G, run.topo.N, self.weight, None,
                      _lib.ptr(self.dev), None]

    def launch(self, run, copy_out, last=False):
        self._launch({7: 1.0 if last else self.weight, 8: copy_out})

    def collect(self, run, bad):
        run.core_dev = self.dev.cpu()                                    # (the kernel skips a quarantined graph: NaN already)


# The order inside a step, after its update: the distance restraints first, with the core's atoms fixed (their partners take the
# whole step); then the torsion restraints, on sides free of core atoms; the hold last, so that the frame a step leaves holds the
# core.  After the last step the measuring launches follow the closing hold, in the same order.
ORDER = (PairRestraints, TorsionRestraints, CoreHold)


def build(N, batch, bond_index, bond_type, num_graphs, kwargs):
    """The constraints the sampler keywords in `kwargs` ask for, in ORDER ([] without any, or with empty lists): every check of the
    keywords, on the host.  The core is built first: its selection is what the other two must not move."""
    made = {}
    for cls in (CoreHold, PairRestraints, TorsionRestraints):
        frozen = made[CoreHold].select if made.get(CoreHold) is not None else None
        made[cls] = cls.from_keywords(N, batch, bond_index, bond_type, num_graphs, frozen, **{k: kwargs[k] for k in cls.KEYWORDS if k in kwargs})
    return [made[cls] for cls in ORDER if made[cls] is not None]


def launch_prologue(pos, batch, skip, copy_out, device):
    """What the stand-alone launchers share: (pos as a contiguous float32 tensor on the GPU -- the caller's own when it is one
    already --, graph_ptr int32 [G + 1] on that device, G, N, skip int32 [G] there or None).  ValueError, before anything touches
    the device: a pos that is not [N, 3], a batch of another length or not sorted, a copy_out that is not a contiguous float32 GPU
    tensor [N, 3], a skip of another length."""
    import torch
    from .trajectory import _graph_ptr
    if not torch.is_tensor(pos):
        pos = torch.from_numpy(as_host(pos, np.float32))
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError("pos must have shape [N, 3], got %s" % (tuple(pos.shape),))
    N = int(pos.shape[0])
    b = as_host(batch).reshape(-1)
    if b.shape[0] != N:
        raise ValueError("batch has %d entries, pos %d atoms" % (b.shape[0], N))
    gp, G = _graph_ptr(b)
    if copy_out is not None and not (torch.is_tensor(copy_out) and copy_out.is_cuda and copy_out.dtype == torch.float32 and
                                     copy_out.is_contiguous() and tuple(copy_out.shape) == (N, 3)):
        raise ValueError("copy_out must be a contiguous float32 tensor [N, 3] on the GPU")
    if skip is not None:
        skip = as_host(skip, np.int32).reshape(-1)
        if skip.shape[0] != G:
            raise ValueError("skip has %d entries, the batch %d graphs" % (skip.shape[0], G))
    if not (pos.is_cuda and pos.dtype == torch.float32 and pos.is_contiguous()):
        pos = pos.to(device, torch.float32).contiguous()
    return pos, torch.from_numpy(gp).to(pos.device), G, N, None if skip is None else torch.from_numpy(skip).to(pos.device)


# ---- sampling ------------------------------------------------------------------------------------------------------------------
def sample_restrained(model, mol, num_samples, sampler_kwargs, device, pairs=None, torsions=None, counter_seed=None, max_retry=2, log=print):
    """`num_samples` conformers of ONE molecule in one batch (the reference driver's own granularity) under the restraints its dict
    carries: the distance restraints restr_pairs / restr_lo / restr_hi when `pairs` = dict(weight, start_sigma, sweeps) is given, the
    torsion restraints tors_quads / tors_target / tors_tol when `torsions` = dict(weight, start_sigma) is (None: that kind is left
    out, whatever the molecule carries).  Packs with driver.pack_batch, checks every keyword before any sampling and samples with
    driver.run_part; the retry rule is scripts/test.py's, as driver.sample_passes applies it: a NaN anywhere samples the molecule
    again with clip_local=20, at most `max_retry` attempts in all (with counter noise a retry draws with attempt + 1); a run that
    only left the split-fp16 range is run again in split-bf16 and is not counted.  Returns a dict: pos float32 [G, n, 3] (numpy), ok
    (False: every attempt failed, everything NaN), and for each kind the molecule was sampled under restraint_viol [G], or
    torsion_viol [G] and torsion_angle [G, T]: what is left at the end of the run.  Holds no core."""
    from . import driver, restraints, torsion_restraints
    G = int(num_samples)
    packed = driver.pack_batch([mol], lambda _num_refs: G)
    n = int(packed["spans"][0][1])
    driver.check_counter(model, packed, counter_seed)
    extra, shapes = {}, {}
    own = torsion_restraints._of_molecule(mol) if torsions is not None else None
    if own is not None:
        q, tg, tl, sides = torsion_restraints.pack_torsion_restraints(packed, [own])
        extra.update(torsion_quads=q, torsion_target=tg, torsion_tol=tl, torsion_sides=sides, torsion_weight=torsions["weight"],
                     torsion_start_sigma=torsions["start_sigma"])
        shapes.update(torsion_viol=(G,), torsion_angle=(G, q.shape[0] // G))
    own = restraints._of_molecule(mol) if pairs is not None else None
    if own is not None:
        pr, lo, hi = restraints.pack_restraints(packed, [own])
        extra.update(restraint_pairs=pr, restraint_lo=lo, restraint_hi=hi, restraint_weight=pairs["weight"],
                     restraint_start_sigma=pairs["start_sigma"], restraint_sweeps=pairs["sweeps"])
        shapes.update(restraint_viol=(G,))
    build(packed["atom_type"].shape[0], packed["batch"], packed["bond_index"], packed["bond_type"], G, extra)   # (a ValueError before any sampling)

    def run_pass(sub, todo, clip_local, wide, tries, first):
        run, pos, _ = driver.run_part(model, sub, device, sampler_kwargs, counter_seed, tries, wide, clip_local=clip_local, save_traj=False,
                                      **extra)
        per_graph = {k: getattr(run, k) for k in shapes}
        if "torsion_angle" in shapes:                                # (per graph along the LAST dimension: angle as [T, G])
            per_graph["torsion_angle"] = run.torsion_angle.reshape(shapes["torsion_angle"]).t().contiguous()
        return pos.cpu(), None, run.nan_graphs().numpy(), getattr(run, "range_graphs", ()), per_graph

    ok, got = driver.sample_passes(packed, run_pass, max_retry, log)
    out = dict(pos=got["pos"].numpy().astype(np.float32).reshape(G, n, 3), ok=bool(ok[0]))
    for k, shape in shapes.items():                                  # ([G] stays [G]; the angles back to [G, T])
        out[k] = np.ascontiguousarray(got[k].numpy().astype(np.float32).T) if k in got else np.full(shape, np.nan, dtype=np.float32)
    return out


def no_violation(G, ok):
    """The violations [G] of a molecule that carries no restraint: zeros, NaN when its sampling failed."""
    return np.zeros(G, dtype=np.float32) if ok else np.full(G, np.nan, dtype=np.float32)


# ---- the jobs ------------------------------------------------------------------------------------------------------------------
def job_parser(doc, testset_help, weight_help, extra=()):
    """The command line both restrained jobs share; `extra`: (flag, keywords) of the options one job has alone, listed after
    --start-sigma."""
    import argparse
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt", default=None, help="reference checkpoint (dict with 'config' and 'model'); not with --report")
    ap.add_argument("--testset", required=True, help=testset_help)
    ap.add_argument("--out", required=True, help="output directory (samples_all.npz); with --report the .npz to write")
    ap.add_argument("--num-confs", default="2x")
    ap.add_argument("--start-idx", type=int, default=0)
    ap.add_argument("--end-idx", type=int, default=200)
    ap.add_argument("--n-steps", type=int, default=5000)
    ap.add_argument("--w-global", type=float, default=1.0)
    ap.add_argument("--global-start-sigma", type=float, default=0.5)
    ap.add_argument("--clip", type=float, default=1000.0)
    ap.add_argument("--weight", type=float, default=1.0, help=weight_help)
    ap.add_argument("--start-sigma", type=float, default=float("inf"),
                    help="restrain only after steps whose noise level sigma is below this (default: from the first step); the launch "
                         "after the last step always runs")
    for flag, kw in extra:
        ap.add_argument(flag, **kw)
    ap.add_argument("--seed", type=int, default=2021)
    ap.add_argument("--noise", default="default", choices=["default", "counter"], help="as agdiff_amd.driver's")
    ap.add_argument("--precision", default=None, choices=[None, "f32", "bf16x3", "f16x3"])
    ap.add_argument("--trust-ckpt", action="store_true", help="unpickle arbitrary classes from the checkpoint")
    ap.add_argument("--report", action="store_true", help="measure a finished job (--samples) instead of sampling")
    ap.add_argument("--samples", default=None, help="--report: the samples_all.npz to measure")
    ap.add_argument("--device", default="cuda")
    return ap


def restrained_job(args, own, check, attach, sample, measure, summary):
    """The job of a restrained command line (`args`: job_parser's), parameterised by what its kind alone knows.  own: {molecule index:
    restraints} of the test set, the kind the job reports on.  --report: measure(i, pos_gen) -> {field: array} for every pos_gen_<i>
    of --samples, saved as <field>_<i> to --out.  Otherwise: check() (the settings, before the model is loaded), then every molecule
    of the range, ONE per batch: attach(mol) puts what the test set carries for it into its dict, sample(model, mol, G, kw, device,
    counter_seed) -> ({"pos_gen": ..., field: array}, ok), saved as pos_gen_<i>, name_<i> and <field>_<i> to --out/samples_all.npz.
    summary: (the field with the violations, the closing line's opening, its format for the largest violation and the median).
    Returns what it saved."""
    from . import driver
    out = {}
    if args.report:
        if not args.samples:
            raise SystemExit("--report needs --samples")
        z = np.load(args.samples, allow_pickle=False)
        for key in z.files:
            if key.startswith("pos_gen_"):
                i = int(key.split("_")[-1])
                out.update({"%s_%d" % (k, i): v for k, v in measure(i, z[key]).items()})
        _summary(out, own, print, *summary)
        np.savez_compressed(args.out, **out)
        return out
    if not args.ckpt:
        raise SystemExit("sampling needs --ckpt")
    check()
    import torch
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    model = driver.load_model(args.ckpt, args.precision, args.trust_ckpt, device)
    mols = [m for m in driver.load_testset(args.testset) if args.start_idx <= m["index"] < args.end_idx]
    confs_of = driver.num_confs(args.num_confs)
    kw = dict(n_steps=args.n_steps, step_lr=1e-6, w_global=args.w_global, global_start_sigma=args.global_start_sigma, clip=args.clip)
    counter_seed = int(args.seed) if args.noise == "counter" else None
    os.makedirs(args.out, exist_ok=True)
    for m in mols:
        i = m["index"]
        attach(m)
        fields, ok = sample(model, m, confs_of(m["num_refs"]), kw, device, counter_seed)
        if not ok:
            print("molecule %s failed twice (NaN); skipped" % m["name"])
            continue
        out["pos_gen_%d" % i], out["name_%d" % i] = fields.pop("pos_gen"), np.str_(m["name"])
        out.update({"%s_%d" % (k, i): v for k, v in fields.items()})
    _summary(out, own, print, *summary)
    driver._save_npz_atomic(os.path.join(args.out, "samples_all.npz"), out)
    return out


def _summary(out, own, log, field, opening, figures):
    worst = [float(np.nanmax(v)) for k, v in out.items() if k.startswith(field + "_") and int(k.split("_")[-1]) in own and
             v.size and not np.isnan(v).all()]
    if worst:
        log(("%s: %d restrained molecules; " + figures) % (opening, len(worst), max(worst), float(np.median(worst))))
    else:
        log("%s: no restrained molecule in this job" % opening)
