"""The local pair head with the edge_attr half of its first layer from per-type polynomials (csrc/edge.hip k_pair_head_typed behind
agdiff_local_head), over the type-pure tiles of the canonical local list (agdiff_topo_t.lh_*, topology.head_tile_permutation).

GPU: one packed batch of three hand-made 16-atom molecules, 220 canonical local edges of seven types whose row counts over the batch
are 17, 16, 15 and 1 (types 1, 2, 3, 12: a second tile of a type, a full tile, pad rows, a tile of one row), 20 (type 4, which is
refused a slot: its tiles read the edge_attr rows), 40 (type 23) and 111 (type 24); with two sets kept in LDS (types 24 and 23)
the sets of types 1, 2, 3, 12 and every far set are read from L2.  The lengths are written by the test.  Expected values: float64 from the state dict -- MLPEdgeEncoder(d, type) and the
head as tests/pair_head_ref.py restates them (reference: models/common.py:44-109, models/epsnet/dualenc.py:226-239) -- under
helpers.check_close at its own tolerances, the gate tests/test_hip_pair_head.py applies to k_pair_head.
Host (no GPU): the permutation of a product-shape batch."""
import ctypes

import numpy as np
import pytest
import torch

import pair_head_ref as R
from helpers import check_close, t

PRECISIONS = ["f16x3", "bf16x3", "f32"]
TYPE_ROWS = ((1, 17), (2, 16), (3, 15), (12, 1), (4, 20), (23, 40), (24, 111))
REFUSED = 4
N_ATOMS, N_MOLS = 16, 3
_STATE = {}


def _molecules():
    """atom types, the bond list (both directions of a bond, except one edge of type 12 and three of type 24, which have no mirror)
    and the graph ids: every unordered pair of a molecule's atoms is a candidate, drawn in a seeded order and dealt to the three
    molecules in turn, types in the order of TYPE_ROWS"""
    rng = np.random.default_rng(5)
    pairs = [(i, j) for i in range(N_ATOMS) for j in range(i + 1, N_ATOMS)]
    per_mol = [rng.permutation(len(pairs)) for _ in range(N_MOLS)]
    types = np.concatenate([np.full(n, ty) for ty, n in TYPE_ROWS])
    src, dst, typ = [], [], []
    one_way = {int(np.nonzero(types == 12)[0][0])} | set(int(k) for k in np.nonzero(types == 24)[0][:3])
    for k, ty in enumerate(types):
        m, slot = k % N_MOLS, k // N_MOLS
        i, j = pairs[per_mol[m][slot]]
        i, j = i + m * N_ATOMS, j + m * N_ATOMS
        src.append(i), dst.append(j), typ.append(ty)
        if k not in one_way:
            src.append(j), dst.append(i), typ.append(ty)
    at = rng.choice([1, 6, 7, 8], size=N_ATOMS * N_MOLS)
    return (at.astype(np.int64), np.stack([np.array(src), np.array(dst)]).astype(np.int64), np.array(typ).astype(np.int64),
            np.repeat(np.arange(N_MOLS), N_ATOMS).astype(np.int64))


def _model(precision):
    from agdiff_amd import get_model, qm9_model_config
    from oracle import agdiff_oracle as O
    if "model" not in _STATE:
        cfg = qm9_model_config()
        sd = O.synth_state_dict_for(cfg, head_scale=1.0)
        m = get_model(cfg)
        m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
        m.poly_refuse_types = (REFUSED,)
        _STATE["model"] = (m.to("cuda:0").eval(), sd, cfg)
    m, sd, cfg = _STATE["model"]
    m.precision = m.precision_local = precision
    return m, sd, cfg


def _tile_paths(topo, pk, length, cutoff):
    """per head tile: 'near' / 'far' (a coefficient set) or 'rows', by the rule of include/agdiff_hip.h: agdiff_local_head"""
    idx = topo.lh_idx.cpu().numpy().reshape(-1, 16)
    tt = topo.lh_type.cpu().numpy()
    near, far = pk.head_local_sets["near"], pk.head_local_sets["far"]
    far_hi = np.float32(10.0 * cutoff)
    out = []
    for row, ty in zip(idx, tt):
        d = length[row[row >= 0]]
        with np.errstate(invalid="ignore"):
            if near[ty] >= 0 and np.all((d >= 0) & (d <= np.float32(cutoff))):
                out.append("near")
            elif near[ty] >= 0 and far[ty] >= 0 and np.all((d > np.float32(cutoff)) & (d <= far_hi)):
                out.append("far")
            else:
                out.append("rows")
    return np.array(out), idx, tt


def _lengths(topo, cutoff):
    """[Lc] float32: mid-range values, then by head tile -- 1e-3 and exactly the cutoff in tiles that stay inside [0, cutoff]; one
    whole tile of type 23 beyond the cutoff with 5 x and 10 x cutoff in it (the far set's range, its end included); in tiles of
    type 24 a length just beyond the cutoff next to in-range ones, 3 x cutoff next to in-range ones, a length beyond 10 x cutoff
    and a NaN"""
    idx = topo.lh_idx.cpu().numpy().reshape(-1, 16)
    tt = topo.lh_type.cpu().numpy()
    rng = np.random.default_rng(9)
    d = rng.uniform(0.3, cutoff - 0.3, topo.Lc).astype(np.float32)
    rc = np.float32(cutoff)
    t1, t23, t24 = (np.nonzero(tt == ty)[0] for ty in (1, 23, 24))
    assert len(t1) == 2 and len(t23) == 3 and len(t24) == 7
    d[idx[t1[0], 0]] = 1e-3
    d[idx[t1[0], 5]] = rc
    d[idx[t24[0], 2]] = 1e-3
    d[idx[t24[0], 9]] = rc
    far_rows = idx[t23[1]]
    d[far_rows] = rng.uniform(1.2 * cutoff, 9.5 * cutoff, 16).astype(np.float32)
    d[far_rows[3]], d[far_rows[11]] = 5 * rc, 10 * rc
    d[idx[t24[1], 4]] = rc * np.float32(1 + 1e-6)
    d[idx[t24[2], 7]] = 3 * rc
    d[idx[t24[3], 1]] = 10 * rc * np.float32(1.25)
    d[idx[t24[4], 13]] = np.nan
    assert d[idx[t24[1], 4]] > rc
    return d


def _run(lib, pk, topo, ws, off, lds_sets):
    from agdiff_amd import _lib
    pk.set_tuning(local_head_poly_off=int(off), local_head_lds_sets=lds_sets)
    ws.l_inv.copy_(R.payload(ws.l_inv.numel(), "cuda"))
    ws.range_rows.zero_()
    ws.variant_log.zero_()
    assert lib.agdiff_local_head(ctypes.byref(pk.struct), ctypes.byref(topo.struct), ctypes.byref(ws.struct), 1, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    return ws.l_inv.clone(), int(ws.variant_log.item())


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_typed_local_head(precision):
    """l_inv against float64 for every finite length; the tiles that read the edge_attr rows bit-identical to the local_head_poly_off
    run; two runs the same bits; nothing written beyond the lc_pos / lc_mir targets; the variant bit follows the switch.

    Measured on MI355X (normwise / element-wise figure of the typed run against float64, gates 2e-5 / 5e-3, 3e-5 / 3e-2, 5e-6 / 2e-3):
    see profiles/local_head_poly_timing.txt."""
    from agdiff_amd import _lib
    from oracle import agdiff_oracle as O
    m, sd, cfg = _model(precision)
    lib, st = _lib.load(), _lib.stream_ptr()
    at, bi, bt, ba = [t(x).cuda() for x in _molecules()]
    with torch.no_grad():
        pk = m._renorm_embedding(at)
        topo, ws = m._batch(at, bi, bt, ba, None, False)
    assert (pk.precision, pk.precision_local) == (precision, precision) and pk.poly_kt == 1
    P, Tp, Wp = ctypes.byref(pk.struct), ctypes.byref(topo.struct), ctypes.byref(ws.struct)
    lc_type = topo.lc_type.cpu().numpy()
    assert sorted((int(ty), int((lc_type == ty).sum())) for ty in np.unique(lc_type)) == sorted(TYPE_ROWS)
    near = pk.head_local_sets["near"]
    assert near[REFUSED] < 0 and all(near[ty] >= 0 for ty, _ in TYPE_ROWS if ty != REFUSED)
    assert near[24] < 2 and near[1] >= 2 and pk.head_local_sets["far"][23] >= 2      # types 24 / 1: from LDS / L2 with two sets in LDS
    # the permutation: every canonical edge once, one type per tile, a segment per type (three molecules: one run)
    idx_all = topo.lh_idx.cpu().numpy()
    assert sorted(idx_all[idx_all >= 0].tolist()) == list(range(topo.Lc)) and topo.head_run_molecules >= N_MOLS
    assert topo.Th == sum((n + 15) // 16 for _, n in TYPE_ROWS) and topo.L % 16 != 0

    cutoff = float(cfg.cutoff)
    length = _lengths(topo, cutoff)
    ws.lc_len[: topo.Lc].copy_(t(length))
    ws.hl.copy_(torch.randn(ws.hl.shape, generator=torch.Generator().manual_seed(53)).cuda())
    assert lib.agdiff_local_edge_rows(P, Tp, Wp, st) == 0
    torch.cuda.synchronize()
    paths, idx, tt = _tile_paths(topo, pk, length, cutoff)
    assert (paths == "near").sum() >= 8 and (paths == "far").sum() == 1 and set(tt[paths == "rows"]) == {REFUSED, 24}
    assert (paths[tt == 24] == "rows").sum() == 4 and (paths[tt == 24] == "near").sum() == 3

    off, log_off = _run(lib, pk, topo, ws, True, 2)
    on, log_on = _run(lib, pk, topo, ws, False, 2)
    again, _ = _run(lib, pk, topo, ws, False, 2)
    all_lds, _ = _run(lib, pk, topo, ws, False, 0)
    flags = int(ws.range_rows.sum())
    pk.set_tuning(local_head_poly_off=0, local_head_lds_sets=0)
    bit = _lib.DEFINES["AGDIFF_VAR_LOCAL_HEAD_POLY"]
    assert log_on & bit and not (log_off & bit)                                           # 5
    assert torch.equal(R.bits(on), R.bits(again))                                         # 3
    assert torch.equal(R.bits(on), R.bits(all_lds))                                       # (a set from L2 or from LDS: the same bits)

    pos, mir = topo.lc_pos.cpu().long(), topo.lc_mir.cpu().long()
    has = mir >= 0
    assert int((~has).sum()) == 4
    named = torch.zeros(ws.l_inv.numel(), dtype=torch.bool)
    named[pos] = True
    named[mir[has]] = True
    assert int(named.sum()) == topo.L == topo.Lc + int(has.sum())
    for out in (on, off):                                                                 # 4
        rest = out.cpu()[~named]
        assert rest.numel() > 0 and torch.equal(R.bits(rest), R.bits(R.payload(rest.numel())))
        assert torch.equal(R.bits(out.cpu()[mir[has]]), R.bits(out.cpu()[pos[has]]))
    # 2: rows of tiles outside the sets' domain
    on_c, off_c = on.cpu()[pos], off.cpu()[pos]
    rows_path = torch.from_numpy(np.concatenate([r[r >= 0] for r in idx[paths == "rows"]])).long()
    set_path = torch.from_numpy(np.concatenate([r[r >= 0] for r in idx[paths != "rows"]])).long()
    assert torch.equal(R.bits(on_c[rows_path]), R.bits(off_c[rows_path]))
    assert not torch.equal(R.bits(on_c[set_path]), R.bits(off_c[set_path]))               # (the sets were used)
    # 1: float64
    finite = np.isfinite(length)
    assert int((~finite).sum()) == 1            # (the NaN length has no float64 value: its row is covered by the bit comparison above)
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith("edge_encoder_global.")}
    keep = torch.from_numpy(np.nonzero(finite)[0]).long()
    attr = O.mlp_edge_encoder(sd64, "edge_encoder_global", t(length).double().view(-1, 1)[keep], t(lc_type).long()[keep])
    src, dst = topo.lc_src.cpu().long()[keep], topo.lc_dst.cpu().long()[keep]
    ref = R.pair_head(sd, "local", cfg.mlp_act, ws.hl.view(-1, 128).cpu(), src.numpy(), dst.numpy(), attr)[0]
    in_set = torch.zeros(topo.Lc, dtype=torch.bool)
    in_set[set_path] = True
    from helpers import elem_err, rel_err
    for name, sel in (("all finite rows", torch.ones_like(keep, dtype=torch.bool)), ("rows by polynomial", in_set[keep])):
        print("local head %s %s: typed %.3g / %.3g, rows %.3g / %.3g (normwise / element-wise vs float64)" % (
            precision, name, rel_err(on_c[keep][sel], ref[sel]), elem_err(on_c[keep][sel], ref[sel]),
            rel_err(off_c[keep][sel], ref[sel]), elem_err(off_c[keep][sel], ref[sel])))
    check_close("local head typed, rows by polynomial", on_c[keep][in_set[keep]], ref[in_set[keep]], precision)
    check_close("local head typed, all finite rows", on_c[keep], ref, precision)
    assert flags == 0


def test_head_tile_permutation_of_a_product_shape_batch():
    """Host: the permutation of a Drugs-shaped batch (40 molecules x 12 conformers, order-3 local edges as the data set items carry
    them): every canonical edge exactly once, one type per tile, pad rows under 10 % of the rows."""
    from agdiff_amd import synth
    from agdiff_amd.topology import BatchTopology
    b = synth.make_packed_batch("drugs", 40, 12, seed=11)
    topo = BatchTopology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], b["num_graphs"], device="cpu")
    idx, tt = topo.lh_idx.numpy(), topo.lh_type.numpy()
    assert idx.shape[0] == 16 * tt.shape[0] == 16 * topo.Th and topo.struct.num_head_tiles == topo.Th
    real = idx >= 0
    assert np.array_equal(np.sort(idx[real]), np.arange(topo.Lc))
    lc_type = topo.lc_type.numpy()
    assert len(np.unique(lc_type)) >= 5
    assert np.array_equal(lc_type[idx[real]], np.repeat(tt, 16)[real])
    assert real.reshape(-1, 16)[:, 0].all()                                   # no tile of pad rows only
    pads = 1.0 - real.mean()
    print("pad rows: %d of %d = %.2f %%, runs of %d molecules" % ((~real).sum(), real.size, 100 * pads, topo.head_run_molecules))
    assert pads < 0.10
    # the rows' other columns are the canonical list's
    for name, ref, pad in (("lh_src", topo.lc_src, 0), ("lh_dst", topo.lc_dst, 0), ("lh_pos", topo.lc_pos, -1), ("lh_mir", topo.lc_mir, -1)):
        col = getattr(topo, name).numpy()
        assert np.array_equal(col[real], ref.numpy()[idx[real]]) and np.all(col[~real] == pad)
    # a run's rows stay together: the molecules of a tile lie within one run of head_run_molecules consecutive ones
    mol = b["batch"][topo.lc_src.numpy()]
    run = np.where(real, mol[np.maximum(idx, 0)] // topo.head_run_molecules, -1).reshape(-1, 16)
    assert all(len(set(r[r >= 0])) == 1 for r in run)
