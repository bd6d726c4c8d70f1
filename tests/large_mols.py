"""Molecules of more than AGDIFF_MAX_ATOMS_PER_GRAPH atoms for the large-molecule tests (test_large_molecules_cpu.py,
test_hip_large_molecules.py).  synth.random_molecule extends the bond graph with dense n x n matrix products, which takes
minutes at a few thousand atoms; here the same random bond tree + ring closures (synth.random_bonds) is extended by the sparse
restatement (topology.extend_graph_order_sparse, itself checked against the dense one in test_large_molecules_cpu.py)."""
import numpy as np

from agdiff_amd import synth
from agdiff_amd.topology import extend_graph_order_sparse


def large_molecule(rng, n):
    """atom_type [n], (row, col, type) of the order-3 extended bond graph sorted by (row, col) -- what synth.random_molecule
    returns, for any n."""
    at, src, dst, typ = synth.random_bonds(rng, n)
    r, c, t = extend_graph_order_sparse(n, src, dst, typ, order=3)
    return at, r, c, t


def batch_with_large(sizes, seed=0, small=(2, 2), copies=1):
    """A packed batch: one molecule per entry of `sizes` (each `copies` conformers), then small[0] Drugs-sized molecules x
    small[1] conformers.  Dict like synth.make_packed_batch's."""
    rng = np.random.default_rng(seed)
    ats, rs, cs, ts, bs = [], [], [], [], []
    node_off, g_off = 0, 0
    for n in sizes:
        at, r, c, t = large_molecule(rng, n)
        a2, r2, c2, t2, b2 = synth.repeat_molecule(at, r, c, t, copies, node_off, g_off)
        ats.append(a2); rs.append(r2); cs.append(c2); ts.append(t2); bs.append(b2)
        node_off += n * copies
        g_off += copies
    if small[0]:
        s = synth.make_packed_batch("drugs", small[0], small[1], seed=seed + 1)
        ats.append(s["atom_type"]); rs.append(s["bond_index"][0] + node_off); cs.append(s["bond_index"][1] + node_off)
        ts.append(s["bond_type"]); bs.append(s["batch"] + g_off)
        g_off += s["num_graphs"]
    return dict(atom_type=np.concatenate(ats), bond_index=np.stack([np.concatenate(rs), np.concatenate(cs)]),
                bond_type=np.concatenate(ts), batch=np.concatenate(bs), num_graphs=g_off)


def check_graph_properties(ws_arrays, topo_arrays, pos, cutoff):
    """What holds for every correct build, whatever the size (numpy arrays): in-lists with ascending sources and at most
    33 + local in-degree entries, ref2dst a permutation that sorts by (src, dst), every local edge present with its type,
    every radius edge shorter than the cutoff and inside its molecule, lengths = |pos_src - pos_dst|, mirror links
    consistent and the canonical list a partition of the edges."""
    E, C = ws_arrays["E"], ws_arrays["C"]
    src, dst, ty, ln = (ws_arrays[k][:E] for k in ("e_src", "e_dst", "e_type", "e_len"))
    ip, op, perm = ws_arrays["in_ptr"], ws_arrays["out_ptr"], ws_arrays["ref2dst"][:E]
    N = ip.shape[0] - 1
    batch, loc_src, loc_dst, loc_type = (topo_arrays[k] for k in ("batch", "loc_src", "loc_dst", "loc_type"))
    assert ip[0] == 0 and ip[-1] == E and op[0] == 0 and op[-1] == E
    assert np.all(np.diff(dst) >= 0) and np.array_equal(np.bincount(dst, minlength=N), np.diff(ip))
    assert np.all(np.diff(src)[np.diff(dst) == 0] > 0)                       # sources ascending inside a list: no duplicates
    locdeg = np.bincount(loc_dst, minlength=N)
    assert np.all(np.diff(ip) <= 33 + locdeg)
    assert np.all(np.bincount(dst[ty == 0], minlength=N) <= 33)
    assert np.array_equal(np.sort(perm), np.arange(E))
    key = src[perm].astype(np.int64) * N + dst[perm]
    assert np.all(np.diff(key) > 0)                                           # ref2dst sorts by (src, dst)
    assert np.array_equal(np.bincount(src, minlength=N), np.diff(op))
    assert np.array_equal(batch[src], batch[dst]) and np.all(src != dst)
    # local edges: all present, with their types, and nothing else carries a type
    lkey = loc_src.astype(np.int64) * N + loc_dst
    ekey = src.astype(np.int64) * N + dst
    o = np.argsort(ekey)
    at = np.searchsorted(ekey[o], lkey)
    assert np.all(at < E) and np.array_equal(ekey[o][np.minimum(at, E - 1)], lkey)
    assert np.array_equal(ty[o][at], loc_type)
    assert int((ty > 0).sum()) == lkey.shape[0]
    d = pos[src].astype(np.float64) - pos[dst].astype(np.float64)
    true_len = np.sqrt((d * d).sum(1))
    assert np.all(np.abs(ln - true_len) <= 1e-6 * np.maximum(true_len, 1.0))
    assert np.all(ln[ty == 0] < cutoff)
    # canonical list
    cp, cm = ws_arrays["c_pos"][:C], ws_arrays["c_mir"][:C]
    assert 0 < C <= E and np.all(np.diff(cp) > 0)
    assert np.array_equal(ws_arrays["c_src"][:C], src[cp]) and np.array_equal(ws_arrays["c_dst"][:C], dst[cp])
    assert np.array_equal(ws_arrays["c_type"][:C], ty[cp])
    assert np.array_equal(ws_arrays["c_len"][:C].view(np.int32), ln[cp].view(np.int32))
    has = cm >= 0
    assert np.all(cm[~has] == -1)
    m = cm[has]
    assert np.array_equal(src[m], dst[cp[has]]) and np.array_equal(dst[m], src[cp[has]])
    assert np.array_equal(ty[m], ty[cp[has]]) and np.array_equal(ln[m].view(np.int32), ln[cp[has]].view(np.int32))
    assert np.all(src[cp[has]] < dst[cp[has]])
    cover = np.zeros(E, dtype=np.int64)
    np.add.at(cover, cp, 1)
    np.add.at(cover, m, 1)
    assert np.all(cover == 1)
    # an unpaired canonical edge has no mirror: its reverse is absent or carries another type
    un = cp[~has]
    rkey = dst[un].astype(np.int64) * N + src[un]
    at = np.minimum(np.searchsorted(ekey[o], rkey), E - 1)
    present = ekey[o][at] == rkey
    assert np.all(~present | (ty[o][at] != ty[un]))
