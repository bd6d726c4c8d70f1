"""Inputs of tests/test_hip_row_moves.py (GPU) and tests/test_row_moves_cases_cpu.py (their design, checked without a GPU): the smallest
lists at which the lane maps of the coalesced row moves (csrc/common.hpp: piece layout <-> operand layout) can go wrong.
  counts    1, 15, 16, 17, 33 entries: one live lane, a tile short of one row, a full tile, one and two full tiles plus one row
  pairs     which node rows a tile's rows name (PAIRS below)
  rows      node and attribute rows whose every element encodes (row, feature): a 16-byte piece that lands in the wrong lane, row or
            k-tile puts values of ANOTHER (row, feature) into the sum -- an error of the size of the operands, not of their rounding"""
import numpy as np
import torch

COUNTS = [1, 15, 16, 17, 33]
PAIRS = ["two_nodes", "ends", "one_node", "random"]
ACT = "gelu"
H_LO, ATTR_LO = 1.0, 0.25      # magnitudes of the coded node / attribute rows start here
VARIANTS = 64                  # sign patterns a case may choose from (head_case)
WELL = 0.2                     # a list's largest score is at least this share of what its last layer adds up (not a cancelled value)


def coded_rows(n, lo, width=128, seed=0):
    """float32 [n, width]: |element (r, f)| = lo + (width r + f + 1) / (width n), distinct for every (r, f) of the tensor, in (lo, lo + 1];
    signs drawn with `seed` (sums over features stay O(sqrt(width)), as for the random rows of the other tests)"""
    r, f = np.arange(n, dtype=np.float64)[:, None], np.arange(width, dtype=np.float64)[None, :]
    sign = np.random.default_rng(1000 + seed).choice([-1.0, 1.0], size=(n, width))
    return torch.from_numpy(((lo + (width * r + f + 1.0) / (float(width) * n)) * sign).astype(np.float32))


def pairs(kind, n_edges, seed=7):
    """(n_nodes, src, dst) int32 [n_edges]
      two_nodes  N = 2: every combination of node 0 and node N - 1 = 1, in turn, from (0, 1) on
      ends       N = 9: the source is node 0 or node N - 1 in turn, targets anywhere; the last entry the other way round
      one_node   N = 5: every row of every tile names node 2 as its source and node 3 as its target -- all rows of a tile read the
                 same two 512-byte rows
      random     N = 11"""
    i = np.arange(n_edges)
    rng = np.random.default_rng(seed + n_edges)
    if kind == "two_nodes":
        n, src, dst = 2, i % 2, (i // 2 + 1) % 2
    elif kind == "ends":
        n = 9
        src, dst = np.where(i % 2 == 0, 0, n - 1), rng.integers(0, n, n_edges)
        src[-1], dst[-1] = dst[-1], (n - 1 if n_edges % 2 else 0)
    elif kind == "one_node":
        n, src, dst = 5, np.full(n_edges, 2), np.full(n_edges, 3)
    else:
        n = 11
        src, dst = rng.integers(0, n, n_edges), rng.integers(0, n, n_edges)
    return n, src.astype(np.int32), dst.astype(np.int32)


def lengths(n_edges, cutoff, variant=0):
    """float32 [n_edges] in (0, cutoff], log-spaced from 0.4, dealt to the entries by a permutation seeded with `variant`; the last one
    exactly the cutoff (a lone entry: the variant's place on the log scale instead)"""
    if n_edges == 1:
        return torch.tensor([0.4 * (cutoff / 0.4) ** (variant / (VARIANTS - 1.0))], dtype=torch.float32).clamp(max=cutoff)
    d = np.logspace(np.log10(0.4), np.log10(cutoff), n_edges).astype(np.float32)
    d = d[np.random.default_rng(29 + n_edges + 1000 * variant).permutation(n_edges)]
    d[-1] = np.float32(cutoff)
    return torch.from_numpy(np.minimum(d, np.float32(cutoff)))


NODE_COUNTS = [1, 16, 17]
NODE_STAGE = 3


def node_case(n):
    """(h_in [n, 128], agg [n, 192]) of one node-stage case: coded rows of the size of the seeded draws the other node tests use"""
    return coded_rows(n, 0.25).numpy(), coded_rows(n, 0.25, width=192, seed=1).numpy()


def head_case(sd, kind, n_edges, head, encoder=None, cutoff=None):
    """(src, dst, h [N, 128], attr, ref [n_edges] float64) of one pair-head case.  encoder None: `attr` [n_edges, 128] are coded
    attribute rows; else (the polynomial head) `attr` are the lengths [n_edges] in (0, cutoff] and encoder(lengths) the float64 rows.
    The normwise gate divides by the list's largest score -- a lone score by itself -- so signs (and lengths) are the first of
    VARIANTS seeded choices for which that score is no cancelled value (WELL), decided on the float64 reference alone."""
    import pair_head_ref as R
    n, src, dst = pairs(kind, n_edges)
    for v in range(VARIANTS):
        h = coded_rows(n, H_LO, seed=v)
        attr = coded_rows(n_edges, ATTR_LO, seed=100 + v) if encoder is None else lengths(n_edges, cutoff, v)
        ref, _, pre2 = R.pair_head(sd, head, ACT, h, src, dst, attr if encoder is None else encoder(attr))
        if float(ref.abs().max() / R.score_weight(sd, head, ACT, pre2).max()) >= WELL:
            return src, dst, h, attr, ref
    raise AssertionError("no well-conditioned variant for %s E=%d %s" % (kind, n_edges, head))
