"""Host side of the large-molecule path (molecules of more than AGDIFF_MAX_ATOMS_PER_GRAPH = 512 atoms): topology, limits,
the sparse bond-graph extension, batch planning.  No GPU."""
import time

import numpy as np
import pytest

from agdiff_amd import _lib, driver, synth
from agdiff_amd.topology import BatchTopology, extend_graph_order_sparse
from large_mols import batch_with_large, large_molecule


def _check_quads_and_tiles(tp, batch):
    """The invariants of test_host_logic.test_local_quad_tiles, vectorised (that test loops over quads x edges)."""
    gt = tp.group_targets
    rt = 16 // gt
    qt, ltp = tp.quad_tgt.numpy().reshape(-1, 4), tp.lt_ptr.numpy()
    lsrc, ldst, ltyp = tp.loc_src.numpy(), tp.loc_dst.numpy(), tp.loc_type.numpy()
    src, typ = tp.lt_src.numpy(), tp.lt_type.numpy()
    Q = tp.Q
    assert qt.shape[0] == Q == tp.struct.num_quads and ltp[-1] == tp.T == tp.struct.num_local_tiles
    assert np.array_equal(np.sort(qt[qt >= 0]), np.arange(tp.N)) and np.all(qt[:, 0] >= 0)
    assert np.all(qt[:, gt:] < 0)
    live = qt >= 0
    assert np.all(np.diff(live.astype(int), axis=1) <= 0)                                  # -1 only at the end of a group
    assert np.all(np.where(live, batch[np.maximum(qt, 0)], batch[qt[:, :1]]) == batch[qt[:, :1]])     # one molecule per group
    sizes = np.bincount(batch)
    assert int((qt[:, :gt] < 0).sum()) == int(((gt - sizes % gt) % gt).sum())
    # tiles per group: sum over the types of the max over its targets of ceil(in-edges of the type / RT)
    types = np.unique(ltyp)
    cnt = np.zeros((tp.N, types.size), dtype=np.int64)
    np.add.at(cnt, (ldst, np.searchsorted(types, ltyp)), 1)
    need = (cnt + rt - 1) // rt
    want = np.where(live[:, :, None], need[np.maximum(qt, 0)], 0).max(axis=1).sum(axis=1)
    assert np.array_equal(np.diff(ltp), want)
    # rows: every local edge in exactly one row, of its target's slot in its target's group, in a tile of its type
    rows = np.arange(16 * tp.T)
    quad_of_tile = np.repeat(np.arange(Q), np.diff(ltp))
    tgt = qt[quad_of_tile[rows // 16], (rows % 16) // rt]
    real, eid = tp.lt_real, tp.lt_eid
    assert int(real.sum()) == tp.L and np.array_equal(np.sort(eid[real]), np.arange(tp.L)) and np.all(eid[~real] == -1)
    assert np.array_equal(ldst[eid[real]], tgt[real]) and np.array_equal(src[real], lsrc[eid[real]])
    assert np.array_equal(typ[real], ltyp[eid[real]])
    assert np.all(typ.reshape(-1, 16) == typ.reshape(-1, 16)[:, :1])                       # one type per tile
    first = qt[quad_of_tile[rows // 16], 0]
    assert np.array_equal(src[~real], np.where(tgt >= 0, tgt, first)[~real])               # pad rows point at the target itself
    # in-edges of a (target, type) in source order inside the target's rows
    r_real = rows[real]
    order = np.lexsort((r_real, typ[real], tgt[real]))
    same = (np.diff(tgt[real][order]) == 0) & (np.diff(typ[real][order]) == 0)
    assert np.all(np.diff(src[real][order])[same] > 0)
    lc_pos, lc_mir = tp.lc_pos.numpy(), tp.lc_mir.numpy()
    tpos, tmir = tp.lc_tpos.numpy(), tp.lc_tmir.numpy()
    assert np.array_equal(eid[tpos], lc_pos)
    assert np.array_equal(eid[tmir[lc_mir >= 0]], lc_mir[lc_mir >= 0]) and np.all(tmir[lc_mir < 0] == -1)


def test_topology_of_a_batch_with_large_molecules():
    """A 513-atom and a 2500-atom molecule next to Drugs-sized ones: the topology builds (NotImplementedError before the large
    path existed), max_atoms_per_graph is the largest molecule's, no mask arrays are allocated, and the CSR views, the
    canonical local list, the quads and the local tiles satisfy what the host-logic tests check at small sizes.
    Measured: 0.4 s for the whole test (three topologies of 3,100 atoms)."""
    b = batch_with_large([513, 2500], seed=3, small=(3, 2))
    t0 = time.time()
    tp = BatchTopology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], b["num_graphs"], device="cpu", group_targets=4)
    took = time.time() - t0
    assert tp.struct.max_atoms_per_graph == tp.max_atoms == 2500 and tp.large
    assert tp.loc_bits is None and not tp.struct.loc_bits
    assert took < 60.0, "topology of a 2500-atom molecule took %.1f s" % took
    assert tp.L == b["bond_type"].shape[0]                  # (the list is already coalesced)
    src, dst = tp.loc_src.numpy(), tp.loc_dst.numpy()
    ip, ie, op = tp.loc_in_ptr.numpy(), tp.loc_in_eid.numpy(), tp.loc_out_ptr.numpy()
    assert np.array_equal(dst[ie], np.repeat(np.arange(tp.N), np.diff(ip)))
    assert np.all(np.diff(src[ie])[np.diff(dst[ie]) == 0] > 0)
    assert np.array_equal(src, np.repeat(np.arange(tp.N), np.diff(op)))
    locdeg = np.diff(ip)
    n_of = np.bincount(b["batch"])[b["batch"]]
    assert tp.max_edges == int(np.minimum(n_of - 1, np.minimum(33, n_of - 1) + locdeg).sum())
    cp, cm, typ = tp.lc_pos.numpy(), tp.lc_mir.numpy(), tp.loc_type.numpy()
    has = cm >= 0
    assert np.array_equal(src[cm[has]], dst[cp[has]]) and np.array_equal(typ[cm[has]], typ[cp[has]])
    cover = np.zeros(tp.L, dtype=np.int64)
    np.add.at(cover, cp, 1)
    np.add.at(cover, cm[has], 1)
    assert np.all(cover == 1)
    _check_quads_and_tiles(tp, b["batch"])
    for gt in (2, 1):
        _check_quads_and_tiles(BatchTopology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], b["num_graphs"],
                                             device="cpu", group_targets=gt), b["batch"])
    # a small batch keeps its masks
    s = synth.make_packed_batch("drugs", 2, 2, seed=1)
    ts = BatchTopology(s["atom_type"], s["bond_index"], s["bond_type"], s["batch"], device="cpu")
    assert not ts.large and ts.loc_bits is not None and ts.struct.loc_bits


def test_topology_at_and_past_the_large_limit():
    """AGDIFF_MAX_ATOMS_LARGE atoms build (in seconds: the quad grouping of a large molecule is a sort, not the pairwise-swap
    search); one atom more still raises, with the new number in the message."""
    nmax = _lib.MAX_ATOMS_LARGE
    assert nmax >= 4096 and _lib.MAX_ATOMS_PER_GRAPH == 512
    for n, ok in ((nmax, True), (nmax + 1, False)):
        at = np.ones(n, dtype=np.int64)
        i = np.arange(n - 1)
        bi = np.stack([np.concatenate([i, i + 1]), np.concatenate([i + 1, i])])
        bt = np.ones(2 * (n - 1), dtype=np.int64)
        t0 = time.time()
        if ok:
            tp = BatchTopology(at, bi, bt, np.zeros(n, dtype=np.int64), device="cpu")
            assert tp.max_atoms == nmax and tp.large and time.time() - t0 < 60.0
        else:
            with pytest.raises(NotImplementedError, match=str(nmax)):
                BatchTopology(at, bi, bt, np.zeros(n, dtype=np.int64), device="cpu")


@pytest.mark.parametrize("n", [1, 2, 7, 60, 300])
def test_sparse_bond_graph_extension_equals_the_dense_one(n):
    rng = np.random.default_rng(n)
    at, src, dst, typ = synth.random_bonds(rng, n)
    for order in (1, 2, 3):
        want = synth.extend_graph_order_np(n, src, dst, typ, order=order)
        got = extend_graph_order_sparse(n, src, dst, typ, order=order)
        for w, g in zip(want, got):
            assert np.array_equal(w, g)


def test_extend_order_of_a_large_molecule_in_the_topology():
    """forward(extend_order=True) hands the raw bond list over: past 512 atoms the topology extends it with the sparse form.
    1500 atoms: 0.02 s."""
    n = 1500
    rng = np.random.default_rng(9)
    at, src, dst, typ = synth.random_bonds(rng, n)
    tp = BatchTopology(at, np.stack([src, dst]), typ, np.zeros(n, dtype=np.int64), extend_order=True, device="cpu")
    r, c, t = extend_graph_order_sparse(n, src, dst, typ)
    assert np.array_equal(tp.loc_index64.numpy(), np.stack([r, c])) and np.array_equal(tp.loc_type64.numpy(), t)


def _mol(rng, n, index):
    at, r, c, t = large_molecule(rng, n)
    return dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=t, num_refs=1, name="m%d" % index, index=index)


def test_driver_plans_and_prepares_a_batch_with_a_large_molecule():
    """plan_batches keeps molecules past 512 atoms out of batches of small ones (those keep the fused sampler front);
    prepare_batch returns a topology for the large batch."""
    from agdiff_amd import get_model, qm9_model_config
    rng = np.random.default_rng(4)
    mols = [_mol(rng, n, k) for k, n in enumerate([40, 700, 35, 50, 600])]
    confs = driver.num_confs("2")
    batches = driver.plan_batches(mols, confs, 100000)
    kinds = [sorted(int(m["atom_type"].shape[0]) > 512 for m in b) for b in batches]
    assert len(batches) == 2 and all(k[0] == k[-1] for k in kinds)
    assert sorted(m["index"] for b in batches for m in b) == list(range(5))
    big = [b for b in batches if b[0]["atom_type"].shape[0] > 512][0]
    model = get_model(qm9_model_config())
    packed, topo = driver.prepare_batch(model, big, confs)
    assert topo is not None and topo.large and topo.max_atoms == 700 and topo.G == packed["num_graphs"] == 4
    # a sub-batch of it (the NaN / range retry) and its shards build as well
    sub = driver.subset_batch(packed, [1])
    ts = BatchTopology(sub["atom_type"], sub["bond_index"], sub["bond_type"], sub["batch"], sub["num_graphs"], device="cpu")
    assert ts.large and ts.G == 2
    from agdiff_amd import dist
    cuts = dist.shard_graphs(*dist.graph_weights(packed), 2)
    assert cuts[0][0] == 0 and cuts[-1][1] == packed["num_graphs"] and all(a < b for a, b in cuts)
    part = dist.shard_of(packed, 1, 2)[0]
    tr = BatchTopology(part["atom_type"], part["bond_index"], part["bond_type"], part["batch"], part["num_graphs"], device="cpu")
    assert tr.large
