"""The rule of agdiff_butina_cluster (include/agdiff_hip.h) restated in numpy, and the packing of a boolean matrix into the bit
layout of agdiff_rmsd_self.  Shared by tests/test_butina_ref_cpu.py (which anchors it on hand-worked graphs) and
tests/test_hip_clusters.py (which holds the kernel to it bit for bit).  Not a test module."""
import numpy as np


def butina(adj, reorder, running=False):
    """(leader, count, rank) int32 [G] of the boolean matrix adj [G, G], straight from the rule: every conformer starts live;
    among the live ones take c with the largest neighbour count, ties to the lowest index; its cluster is c plus every live j
    with adj[c, j]; the members stop being live.  reorder: the count is over the conformers still live at the choice, else over
    all conformers, once.  The diagonal is taken as set.
    running=True keeps the live counts as a running total (minus the removed members' columns) where the plain form counts them
    afresh at every choice: G times cheaper, for the large cases; tests/test_butina_ref_cpu.py holds the two forms equal."""
    adj = np.array(adj, dtype=bool)
    G = adj.shape[0]
    adj[np.arange(G), np.arange(G)] = True
    live = np.ones(G, dtype=bool)
    leader = np.full(G, -1, dtype=np.int32)
    count = np.zeros(G, dtype=np.int32)
    rank = np.full(G, -1, dtype=np.int32)
    n = adj.sum(1)
    k = 0
    while live.any():
        if reorder and not running:
            n = adj[:, live].sum(1)
        c = int(np.argmax(np.where(live, n, -1)))          # (argmax returns the first, i.e. lowest, index of the maximum)
        members = live & adj[c]
        leader[members], rank[members], count[c] = c, k, members.sum()
        live &= ~members
        if reorder and running:
            n = n - adj[:, members].sum(1)
        k += 1
    return leader, count, rank


def pack(adj, garbage=None):
    """int64 numpy [G, pitch / 8] from the boolean matrix adj [G, G]: bit c of byte b of a row = column 8 b + c, the row pitch
    of ensemble.bits_pitch.  garbage=True fills the padding columns (G and up) with ones instead of zeros."""
    from agdiff_amd.ensemble import bits_pitch
    adj = np.asarray(adj, dtype=bool)
    G = adj.shape[0]
    wide = np.full((G, 8 * bits_pitch(G)), 1 if garbage else 0, dtype=np.uint8)
    wide[:, :G] = adj
    return np.packbits(wide, axis=1, bitorder="little").view(np.int64).copy()


def graph(G, edges):
    """symmetric boolean matrix with the diagonal set from a list of edges"""
    adj = np.eye(G, dtype=bool)
    for i, j in edges:
        adj[i, j] = adj[j, i] = True
    return adj


def random_graph(G, density, seed):
    rng = np.random.default_rng(seed)
    adj = np.triu(rng.random((G, G)) < density, 1)
    return adj | adj.T | np.eye(G, dtype=bool)


SEVEN = [(0, 1), (0, 2), (0, 3), (4, 1), (4, 2), (4, 5), (5, 6)]          # the graph on which the two modes differ
