"""Each conformer's RMSD to a target structure along the denoising run.

examples/test_alanine_dipeptide.py:106-164 (save_dcd_alanine, calc_rmsd) saves the whole trajectory and then superposes every
frame of every conformer on a target structure: the heavy-atom RMSD over the steps is the curve that shows the sampler
converging.  Here the curve is computed on the GPU (csrc/eval.hip: agdiff_traj_rmsd; there is no CPU fallback) from frames of a
PACKED batch, one 64-lane wave per (frame, graph), identity atom mapping like mdtraj's rmsd:

    rmsd_to_target     frames [S, N, 3] -> [S, G] (and the RMSD to the mirror image from the same diagonalisation)
    ring_spans         which rows of a ring of frames hold the steps [done, ready)
    RmsdTracker        what epsnet.LangevinRun holds with `rmsd_target`: one launch per NaN poll while the run samples, so that
                       the curve needs a small ring of frames and not the trajectory

    python -m agdiff_amd.trajectory --samples out/samples_all.npz --testset test.npz --out curves.npz [--mirror] [--all-atoms]
"""
import ctypes

import numpy as np

from . import _lib
from .molecule import as_host


def ring_spans(done, ready, ring_rows):
    """The contiguous row spans [(lo, hi), ...] of a ring of `ring_rows` frames, row = step % ring_rows, that hold the steps
    [done, ready), in step order: one span, or two when the steps wrap around the ring's end; none when done == ready.  More than
    `ring_rows` steps cannot all be in the ring still: ValueError."""
    done, ready, ring_rows = int(done), int(ready), int(ring_rows)
    if ring_rows <= 0 or done < 0 or ready < done:
        raise ValueError("ring_spans needs ring_rows > 0 and 0 <= done <= ready (got done=%d, ready=%d, ring_rows=%d)"
                         % (done, ready, ring_rows))
    count = ready - done
    if count > ring_rows:
        raise ValueError("steps [%d, %d) do not fit a ring of %d frames: the oldest have been overwritten" % (done, ready, ring_rows))
    if count == 0:
        return []
    lo = done % ring_rows
    if lo + count <= ring_rows:
        return [(lo, lo + count)]
    return [(lo, ring_rows), (0, lo + count - ring_rows)]


def _graph_ptr(batch, what="batch"):
    """(graph_ptr int32 [G + 1], G) of sorted graph ids `batch` [N] (numpy int64); ids 0 .. G - 1 with G = batch[-1] + 1."""
    b = np.asarray(batch).reshape(-1).astype(np.int64)
    if b.size == 0:
        raise ValueError("%s is empty" % what)
    if b[0] < 0 or np.any(np.diff(b) < 0):
        raise ValueError("%s must hold sorted, non-negative graph ids" % what)
    G = int(b[-1]) + 1
    return np.searchsorted(b, np.arange(G + 1)).astype(np.int32), G


def _selection(N, select, atom_type):
    """uint8 [N] (numpy): `select`, else the heavy atoms (atom_type != 1), else every atom."""
    if select is None:
        if atom_type is None:
            return np.ones(N, dtype=np.uint8)
        select = as_host(atom_type).reshape(-1) != 1
    sel = as_host(select).reshape(-1)
    if sel.shape[0] != N:
        raise ValueError("the selection has %d entries for %d atoms" % (sel.shape[0], N))
    return np.ascontiguousarray(sel != 0, dtype=np.uint8)


def _check_selected(sel, gp):
    """Every graph needs a selected atom (the kernel would write NaN for one without)."""
    upto = np.concatenate([[0], np.cumsum(sel, dtype=np.int64)])
    count = upto[gp[1:]] - upto[gp[:-1]]
    empty = np.nonzero(count == 0)[0]
    if empty.size:
        raise ValueError("graph %d has no selected atom (%d graphs in all): nothing to superpose" % (int(empty[0]), empty.size))


class RmsdTracker:
    """The device-side state of one tracked batch: target [N, 3], selection, graph_ptr, and `rows` [steps, G] (+ `rows_mirror`) that
    `evaluate` fills span by span on the current stream."""

    def __init__(self, target, select, graph_ptr, steps, device, mirror=False, atom_type=None):
        import torch
        gp = as_host(graph_ptr, np.int32).reshape(-1)
        self.G, self.N = gp.shape[0] - 1, int(gp[-1])
        tgt = torch.from_numpy(as_host(target, np.float32))
        if tuple(tgt.shape) != (self.N, 3):
            raise ValueError("the target has shape %s, the batch %d atoms: expected [%d, 3]" % (tuple(tgt.shape), self.N, self.N))
        sel = _selection(self.N, select, atom_type)
        _check_selected(sel, gp)
        self.target = tgt.to(device).contiguous()
        self.select = torch.from_numpy(sel).to(device)
        self.graph_ptr = torch.from_numpy(gp).to(device)
        self.rows = torch.empty((int(steps), self.G), dtype=torch.float32, device=device)
        self.rows_mirror = torch.empty_like(self.rows) if mirror else None

    def evaluate(self, frames, frame_stride, count, first_row):
        """One launch: `count` frames from the device tensor `frames` on, `frame_stride` floats apart -> rows [first_row,
        first_row + count)."""
        if count <= 0:
            return
        out = self.rows[first_row:first_row + count]
        mir = self.rows_mirror[first_row:first_row + count] if self.rows_mirror is not None else None
        _lib.call("agdiff_traj_rmsd", frames, int(frame_stride), self.target, self.select, self.graph_ptr, int(count), self.G, self.N,
                  out, mir)


def rmsd_to_target(frames, target, batch, select=None, atom_type=None, mirror=False, device="cuda"):
    """float32 [S, G] on the device: the RMSD of every graph of every frame of `frames` [S, N, 3] (tensor or array; a tensor on the
    GPU stays where it is) to `target` [N, 3] after the optimal proper rotation + translation, over the atoms of `select` [N]
    (default: the heavy atoms, atom_type != 1, when `atom_type` is given, else all atoms), identity atom mapping.  `batch` [N]:
    sorted graph ids.  mirror=True: the pair (RMSD, RMSD of the frame's mirror image).  Frames a constant number of floats apart
    (a slice or a strided view along the first dimension) are read in place."""
    import torch
    fr = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32))
    if fr.dim() != 3 or fr.shape[2] != 3:
        raise ValueError("frames must have shape [S, N, 3], got %s" % (tuple(fr.shape),))
    S, N = int(fr.shape[0]), int(fr.shape[1])
    b = as_host(batch).reshape(-1)
    if b.shape[0] != N:
        raise ValueError("batch has %d entries, the frames %d atoms" % (b.shape[0], N))
    gp, G = _graph_ptr(b)
    if tuple(target.shape) != (N, 3):
        raise ValueError("the target has shape %s, the frames %d atoms: expected [%d, 3]" % (tuple(target.shape), N, N))
    sel = _selection(N, select, atom_type)
    _check_selected(sel, gp)
    if not fr.is_cuda:
        fr = fr.to(device)
    fr = fr.to(torch.float32)
    # rows of [N, 3] floats, packed, a constant (positive) number of floats apart: passed as they lie
    if not (fr.stride(2) == 1 and fr.stride(1) == 3 and (S <= 1 or fr.stride(0) >= 3 * N)):
        fr = fr.contiguous()
    stride = int(fr.stride(0)) if S > 1 else 3 * N
    tr = RmsdTracker(target, sel, gp, S, fr.device, mirror=mirror)
    if S:       # (the address as it is: `ptr` would refuse the strided view)
        _lib.call("agdiff_traj_rmsd", ctypes.c_void_p(fr.data_ptr()), stride, tr.target, tr.select, tr.graph_ptr, S, G, N, tr.rows,
                  tr.rows_mirror)
    return (tr.rows, tr.rows_mirror) if mirror else tr.rows


def main(argv=None):
    """python -m agdiff_amd.trajectory --samples out/samples_all.npz --testset test.npz --out curves.npz [--mirror] [--all-atoms]
    For every molecule i of the test set with a saved trajectory `traj_<i>` [steps, g, n, 3] (driver --save-traj) and a target
    `pos_target_<i>` [n, 3]: `rmsd_traj_<i>` float32 [steps, g], the heavy-atom RMSD (--all-atoms: over every atom) of each
    conformer to the target, step by step; --mirror adds `rmsd_mirror_traj_<i>`, the RMSD of the mirror image.  Molecules without
    a trajectory or a target are listed and skipped."""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", required=True)
    ap.add_argument("--testset", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--mirror", action="store_true")
    ap.add_argument("--all-atoms", action="store_true")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    from .driver import load_testset
    zs = np.load(args.samples, allow_pickle=False)
    out, skipped = {}, []
    for m in load_testset(args.testset):
        i = m["index"]
        if "traj_%d" % i not in zs.files or m.get("pos_target") is None:
            skipped.append("%s (%s)" % (m["name"], "no traj_%d" % i if "traj_%d" % i not in zs.files else "no pos_target_%d" % i))
            continue
        traj = np.asarray(zs["traj_%d" % i], dtype=np.float32)
        steps, g, n = traj.shape[:3]
        at = np.asarray(m["atom_type"]).reshape(-1)
        if n != at.shape[0]:
            raise ValueError("traj_%d has %d atoms per conformer, the test set's molecule %d" % (i, n, at.shape[0]))
        res = rmsd_to_target(traj.reshape(steps, g * n, 3), np.tile(np.asarray(m["pos_target"], dtype=np.float32), (g, 1)),
                             np.repeat(np.arange(g), n), atom_type=None if args.all_atoms else np.tile(at, g), mirror=args.mirror,
                             device=args.device)
        proper, mir = res if args.mirror else (res, None)
        out["rmsd_traj_%d" % i] = proper.cpu().numpy()
        if mir is not None:
            out["rmsd_mirror_traj_%d" % i] = mir.cpu().numpy()
        last = out["rmsd_traj_%d" % i][-1]
        print("%s: %d steps x %d conformers, final RMSD to the target %.3f (mean) / %.3f (best)"
              % (m["name"], steps, g, float(np.nanmean(last)), float(np.nanmin(last))))
    for s in skipped:
        print("skipped: %s" % s)
    with open(args.out, "wb") as f:
        np.savez_compressed(f, **out)
    return out


if __name__ == "__main__":
    main()
