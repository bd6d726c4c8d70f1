"""Conformers around a fixed core: the rigid core hold of the sampler.

A ligand series on a crystallographic core, a docking pose whose hinge binder stays put, a macrocycle ring kept while the side
chains are sampled: what rdkit's coordMap / ConstrainedEmbed are used for.  The score network sees distances only, so the
constraint holds the INTERNAL geometry of the core and lets it float rigidly with the rest of the molecule: after a step's update
the core atoms are replaced by the template's, superposed on where they are now (csrc/eval.hip: agdiff_hold_core, fp64 Horn /
Jacobi, one wave per graph of a packed batch; there is no CPU fallback).  The conformer is put into the template's frame once,
after the run (driver.run_job(hold_core=True)).  DESIGN.md 4.16.

    core_arguments     the checks of epsnet.LangevinRun's keywords core_pos / core_select / core_weight / core_start_sigma
    hold_core          one stand-alone launch on a packed batch
    to_template_frame  a molecule's conformers superposed on the template over the core atoms

The hold inside a run is constraints.CoreHold: the last entry of constraints.ORDER.
"""
import numpy as np

from . import _lib
from .constraints import launch_prologue, weight_and_start
from .molecule import as_host


def core_arguments(N, core_pos, core_select, core_weight=1.0, core_start_sigma=float("inf")):
    """(core_pos float32 [N, 3], core_select uint8 [N], weight, start sigma) on the host for a batch of N atoms, or None when
    neither array is given.  ValueError: one array without the other, a wrong shape, a weight outside (0, 1], a start sigma that
    is NaN.  Needs no GPU."""
    if core_pos is None and core_select is None:
        return None
    if core_select is None:
        raise ValueError("core_pos needs core_select [N] (bool): which atoms of the batch belong to the core")
    if core_pos is None:
        raise ValueError("core_select needs core_pos [N, 3]: the template the selected atoms are held to")
    N = int(N)
    pos = as_host(core_pos)
    if tuple(pos.shape) != (N, 3):
        raise ValueError("core_pos has shape %s, the batch %d atoms: expected [%d, 3]" % (tuple(pos.shape), N, N))
    sel = as_host(core_select)
    if tuple(sel.shape) != (N,):
        raise ValueError("core_select has shape %s, the batch %d atoms: expected [%d]" % (tuple(sel.shape), N, N))
    w, start = weight_and_start(core_weight, core_start_sigma,
                                "core_weight must lie in (0, 1] (got %r): 1 holds the core exactly, less pulls it that fraction of the way",
                                "core_start_sigma must be a number (inf: hold from the first step)")
    return np.array(pos, dtype=np.float32, order="C"), np.ascontiguousarray(sel != 0, dtype=np.uint8), w, start


def hold_core(pos, core_pos, select, batch, weight=1.0, skip=None, copy_out=None, device="cuda"):
    """One agdiff_hold_core launch on the packed batch `pos` [N, 3]: (pos, dev).  A contiguous float32 tensor on the GPU is
    changed IN PLACE and returned; anything else is copied to `device` first.  `core_pos` [N, 3], `select` [N], `batch` [N] sorted
    graph ids; skip [G] (!= 0 leaves the graph alone) and copy_out (a contiguous float32 GPU tensor [N, 3] that receives the
    selected atoms' new values) are optional.  dev float32 [G] on the device: the RMSD between each core before the call and
    its fit, NaN for a graph that was left alone."""
    import torch
    pos, gp, G, N, skip = launch_prologue(pos, batch, skip, copy_out, device)
    tpl, sel, w, _ = core_arguments(N, core_pos, select, weight)
    out = torch.empty(G, dtype=torch.float32, device=pos.device)
    _lib.call("agdiff_hold_core", pos, torch.from_numpy(tpl).to(pos.device), torch.from_numpy(sel).to(pos.device), gp, skip, G, N, w, copy_out,
              out)
    return pos, out


def to_template_frame(pos, core_pos, core_mask, device="cuda"):
    """The conformers pos [G, n, 3] (or [G * n, 3]) of ONE molecule superposed on its template core_pos [n, 3] over the atoms of
    core_mask [n] (agdiff_align_conformers: proper rotation + translation applied to all atoms): float32 [G, n, 3] on `device`.
    After a held run the core atoms then lie on the template's."""
    import torch
    from .ensemble import _align
    mask = as_host(core_mask).reshape(-1) != 0
    n = mask.shape[0]
    idx = np.nonzero(mask)[0].astype(np.int32)
    if idx.size == 0:
        raise ValueError("core_mask selects no atom: nothing to superpose on")
    tpl = as_host(core_pos, np.float32)
    if tpl.shape != (n, 3):
        raise ValueError("core_pos has shape %s, core_mask %d atoms: expected (%d, 3)" % (tpl.shape, n, n))
    tpl[~mask] = 0.0                                    # (rows outside the mask are not read; they need not be finite)
    out, _ = _align(_lib.conformers(pos, n, device), torch.from_numpy(idx).to(device), torch.from_numpy(tpl).to(device))
    return out
