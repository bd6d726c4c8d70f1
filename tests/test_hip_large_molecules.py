"""GPU (MI355X): molecules of more than AGDIFF_MAX_ATOMS_PER_GRAPH = 512 atoms -- agdiff_graph_build_large (csrc/graph.hip,
k_lg_*) against the oracle's radius graph and, bit for bit, against the LDS build where both exist; forward, sampler, loss and
the driver on batches that hold such a molecule.  Gates: those of tests/test_hip_parity.py (helpers.check_close; index
tensors np.array_equal)."""
import ctypes
import time

import numpy as np
import pytest
import torch

from helpers import check_close, load_golden, rel_err, t
from large_mols import batch_with_large, check_graph_properties, large_molecule

pytestmark = pytest.mark.gpu

PRECISIONS = ["f32", "bf16x3", "f16x3"]
CUTOFF = 10.0


def _gpu_model(cfg, head_scale=1e-3, precision="f16x3"):
    from agdiff_amd import get_model
    from oracle import agdiff_oracle as O
    sd = O.synth_state_dict_for(cfg, head_scale=head_scale)
    m = get_model(cfg)
    m.precision = precision
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    return m.to("cuda:0").eval(), sd


def _positions(b, seed, dilute):
    """Compact: randn x 3 (every atom of a molecule inside the cutoff of every other: the 33-cap decides everywhere).  Dilute:
    a molecule of n > 512 atoms is spread with standard deviation (2.1 n)^(1/3): the pair distance of two atoms is then normal
    with variance 2 s^2 per axis, an atom at the centre sees n (4 pi / 3) 10^3 / (4 pi s^2)^(3/2) = 94 n / s^3 ~ 45 others
    inside the cutoff and the outer atoms fewer than 32 -- capped and uncapped targets in one molecule."""
    n_of = np.bincount(b["batch"])[b["batch"]]
    scale = np.where(n_of > 512, np.cbrt(2.1 * n_of), 3.0) if dilute else np.full(n_of.shape, 3.0)
    pos = torch.randn(n_of.shape[0], 3, generator=torch.Generator().manual_seed(seed))
    return (pos * torch.from_numpy(scale).float()[:, None]).contiguous()


def _in_range_counts(pos, b, g):
    """Candidates inside the cutoff (self excluded) of every atom of graph g, the rule's own fp32 arithmetic."""
    p = pos[torch.from_numpy(b["batch"] == g)]
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return ((d2 < torch.tensor(CUTOFF) * torch.tensor(CUTOFF)).sum(1) - 1).numpy()


def _arrays(ws, topo):
    torch.cuda.synchronize()
    E, C = int(ws.num_edges.item()), int(ws.num_canon.item())
    w = {k: getattr(ws, k).cpu().numpy() for k in ("e_src", "e_dst", "e_type", "e_len", "in_ptr", "out_ptr", "ref2dst", "c_pos",
                                                    "c_mir", "c_src", "c_dst", "c_type", "c_len")}
    w.update(E=E, C=C)
    tp = dict(batch=topo.batch64.cpu().numpy(), loc_src=topo.loc_src.cpu().numpy(), loc_dst=topo.loc_dst.cpu().numpy(),
              loc_type=topo.loc_type.cpu().numpy())
    return w, tp


# every output of a graph build (agdiff_ws_t), whole buffers: what a build does not write stays as the host allocated it
OUTPUTS = ("num_edges", "graph_edge_cnt", "graph_edge_ptr", "in_ptr", "out_ptr", "e_src", "e_dst", "e_type", "e_len", "ref2dst",
           "e_loc", "num_canon", "graph_canon_cnt", "graph_canon_ptr", "c_len", "c_type", "c_src", "c_dst", "c_pos", "c_mir",
           "rad_cnt", "rad_src", "rad_len", "r_scale")


def _build(lib, variant, P, topo, ws, pos, large):
    from agdiff_amd import _lib
    T, W, st, c = ctypes.byref(topo.struct), ctypes.byref(ws.struct), _lib.stream_ptr(), ctypes.c_float(CUTOFF)
    name, ronly = variant
    if large:
        rc = lib.agdiff_graph_build_large(P if name == "scaled" else None, T, W, _lib.ptr(pos), c, ronly, st)
    elif name == "plain":
        rc = lib.agdiff_graph_build(T, W, _lib.ptr(pos), c, st)
    elif name == "ex":
        rc = lib.agdiff_graph_build_ex(T, W, _lib.ptr(pos), c, ronly, st)
    else:
        rc = lib.agdiff_graph_build_scaled(P, T, W, _lib.ptr(pos), c, ronly, st)
    assert rc == 0, (variant, large, rc)
    torch.cuda.synchronize()


VARIANTS = [("plain", 0), ("ex", 1), ("scaled", 0), ("scaled", 1)]


def _small_batches():
    from agdiff_amd import synth
    out = {}
    for case in ("g3_forward_qm9_small", "g3_forward_smooth_sparse", "g3_forward_drugs_capped"):
        g = load_golden(case)
        out[case] = (dict(atom_type=g["atom_type"], bond_index=g["bond_index"], bond_type=g["bond_type"], batch=g["batch"],
                          num_graphs=int(g["batch"].max()) + 1), t(g["pos"]).float().contiguous())
    b = synth.make_packed_batch("drugs", 8, 4, seed=17)
    out["drugs_8x4_compact"] = (b, _positions(b, 5, False))
    out["drugs_8x4_spread"] = (b, _positions(b, 6, False) * 2.5)
    for n in (385, 512):
        a1, r1, c1, t1 = synth.random_molecule(np.random.default_rng(n), n)
        s = synth.make_packed_batch("drugs", 2, 2, seed=4)
        b = dict(atom_type=np.concatenate([a1, s["atom_type"]]), bond_index=np.concatenate([np.stack([r1, c1]), s["bond_index"] + n], axis=1),
                 bond_type=np.concatenate([t1, s["bond_type"]]), batch=np.concatenate([np.zeros(n, dtype=np.int64), s["batch"] + 1]),
                 num_graphs=1 + s["num_graphs"])
        out["n%d_compact" % n] = (b, _positions(b, 13, False))
        out["n%d_spread" % n] = (b, _positions(b, 14, False) * 2.7)
    return out


@pytest.mark.parametrize("case", ["g3_forward_qm9_small", "g3_forward_smooth_sparse", "g3_forward_drugs_capped", "drugs_8x4_compact",
                                  "drugs_8x4_spread", "n385_compact", "n385_spread", "n512_compact", "n512_spread"])
def test_large_build_equals_the_lds_build_bit_for_bit(case):
    """agdiff_graph_build_large called directly on batches the LDS build (k_graph) handles: EVERY output buffer equal, for the
    plain build, the sampler's radius-only canonical list and the scaled variant with its pad rows.  Pins order and canonical
    choice, which a comparison of edge sets against the oracle does not."""
    from agdiff_amd import _lib, drugs_model_config
    from agdiff_amd.topology import Workspace
    lib = _lib.load()
    b, pos = _small_batches()[case]
    m, _ = _gpu_model(drugs_model_config())
    at = t(b["atom_type"]).cuda()
    with torch.no_grad():
        pk = m._renorm_embedding(at)
        topo, ws_small = m._batch(at, t(b["bond_index"]), t(b["bond_type"]), t(b["batch"]), b["num_graphs"], False)
    assert not topo.large
    P = ctypes.byref(pk.struct)
    posd = pos.cuda().contiguous()
    for variant in VARIANTS:
        ws_a, ws_b = Workspace(topo), Workspace(topo)
        _build(lib, variant, P, topo, ws_a, posd, large=False)
        _build(lib, variant, P, topo, ws_b, posd, large=True)
        assert not int(ws_a.variant_log.item()) & _lib.DEFINES["AGDIFF_VAR_GRAPH_LARGE"]
        assert int(ws_b.variant_log.item()) & _lib.DEFINES["AGDIFF_VAR_GRAPH_LARGE"]
        assert int(ws_a.num_edges.item()) > 0
        for name in OUTPUTS:
            x, y = getattr(ws_a, name).cpu().numpy(), getattr(ws_b, name).cpu().numpy()
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), (case, variant, name, int((x != y).sum()))


@pytest.mark.parametrize("dilute", [False, True])
@pytest.mark.parametrize("n", [513, 1000, 4096])
def test_large_graph_bit_exact_against_the_oracle(n, dilute):
    """A molecule of n > 512 atoms next to small ones: edge set, order, types bit-exact and lengths <= 1e-6 against the oracle's
    radius graph (O.extend_graph_order_radius, extend_order=False), through all three entry points, which take the large path
    by themselves.  Compact: every atom of the molecule at the cap (mean in-degree > 31).  Dilute: 20..80 % of its atoms
    have fewer than 32 candidates inside the cutoff, the others more.
    CPU side (oracle radius graph + lengths with extend_order=False; the bond graph comes extended from large_mols), measured:
    under 0.1 s at 513 and 1000 atoms, 0.3 s at 4096 atoms per geometry; the dense [n, n, 3] evaluation needs ~0.5 GB there,
    which is why 4096 and not AGDIFF_MAX_ATOMS_LARGE is the largest oracle-checked size."""
    from agdiff_amd import _lib, drugs_model_config
    from agdiff_amd.topology import Workspace
    from oracle import agdiff_oracle as O
    lib = _lib.load()
    b = batch_with_large([n], seed=n, small=(2, 2))
    pos = _positions(b, 21 + n, dilute)
    t0 = time.time()
    ei, et = O.extend_graph_order_radius(pos.shape[0], pos, t(b["bond_index"]), t(b["bond_type"]), t(b["batch"]), cutoff=CUTOFF,
                                         extend_order=False)
    elen = O.get_distance(pos, ei)
    print("oracle graph of %d atoms: %.1f s" % (n, time.time() - t0))
    cnt = _in_range_counts(pos, b, 0)
    share = float((cnt < 32).mean())
    print("share of atoms with fewer than 32 radius neighbours: %.2f" % share)
    if dilute:
        assert 0.2 <= share <= 0.8
    else:
        assert share == 0.0
    m, _ = _gpu_model(drugs_model_config())
    at = t(b["atom_type"]).cuda()
    with torch.no_grad():
        pk = m._renorm_embedding(at)
        topo, _ws = m._batch(at, t(b["bond_index"]), t(b["bond_type"]), t(b["batch"]), b["num_graphs"], False)
    assert topo.large and topo.max_atoms == n and topo.loc_bits is None
    P = ctypes.byref(pk.struct)
    posd = pos.cuda().contiguous()
    grid = (ctypes.c_int64 * 2)()
    assert lib.agdiff_graph_large_grid(ctypes.byref(topo.struct), grid) == 0
    assert grid[0] * grid[1] >= topo.N and grid[1] * 2 <= n          # more than one workgroup per large molecule
    for variant in VARIANTS:
        ws = Workspace(topo)
        assert ws.g_inbits is None
        _build(lib, variant, P, topo, ws, posd, large=False)
        assert int(ws.variant_log.item()) & _lib.DEFINES["AGDIFF_VAR_GRAPH_LARGE"]
        E = int(ws.num_edges.item())
        assert E == ei.shape[1] and E <= topo.max_edges
        perm = ws.ref2dst[:E].long()
        assert np.array_equal(np.sort(perm.cpu().numpy()), np.arange(E))
        assert np.array_equal(torch.stack([ws.e_src[:E][perm], ws.e_dst[:E][perm]]).cpu().numpy(), ei.numpy())
        assert np.array_equal(ws.e_type[:E][perm].cpu().numpy(), et.numpy())
        assert rel_err(ws.e_len[:E][perm].cpu().numpy(), elen.numpy()) < 1e-6
        indeg = np.diff(ws.in_ptr.cpu().numpy())
        if not dilute:
            assert indeg[:n].mean() > 31
        # the radius rows by target are the type-0 edges of the full list
        rc = ws.rad_cnt.cpu().numpy()
        ety, esrc, edst = ws.e_type[:E].cpu().numpy(), ws.e_src[:E].cpu().numpy(), ws.e_dst[:E].cpu().numpy()
        assert np.array_equal(rc, np.bincount(edst[ety == 0], minlength=topo.N))
        rs = ws.rad_src.cpu().numpy().reshape(topo.N, -1)
        rows = np.arange(rs.shape[1])[None, :] < rc[:, None]
        assert np.array_equal(rs[rows], esrc[ety == 0])
        if variant[1] == 0:
            w, tp = _arrays(ws, topo)
            check_graph_properties(w, tp, pos.numpy(), CUTOFF)
        else:                # the sampler's list: one entry per mirror pair of radius edges, every radius edge covered once
            C = int(ws.num_canon.item())
            cp, cm = ws.c_pos[:C].cpu().numpy(), ws.c_mir[:C].cpu().numpy()
            mk = cm >= 0
            assert np.all(ety[cp] == 0) and np.all(ety[cm[mk]] == 0)
            assert np.array_equal(esrc[cm[mk]], edst[cp[mk]]) and np.array_equal(edst[cm[mk]], esrc[cp[mk]])
            assert np.all(esrc[cp[mk]] < edst[cp[mk]])
            cover = np.bincount(np.concatenate([cp, cm[mk]]), minlength=E)
            assert np.array_equal(cover, (ety == 0).astype(cover.dtype))


def test_large_graph_properties_at_the_atom_limit():
    """AGDIFF_MAX_ATOMS_LARGE atoms in one molecule (beyond what the dense CPU oracle affords), two conformers, next to small
    molecules, capped and uncapped targets: the properties every correct build has (large_mols.check_graph_properties), the
    cap rule itself on a sample of targets, two builds bitwise equal, and the launch spreads the molecule over many
    workgroups."""
    from agdiff_amd import _lib
    from agdiff_amd.topology import BatchTopology, Workspace
    lib = _lib.load()
    n = _lib.MAX_ATOMS_LARGE
    b = batch_with_large([n], seed=2, small=(2, 2), copies=2)
    pos = _positions(b, 77, True)
    topo = BatchTopology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], b["num_graphs"], device="cuda")
    assert topo.large and topo.max_atoms == n
    grid = (ctypes.c_int64 * 2)()
    assert lib.agdiff_graph_large_grid(ctypes.byref(topo.struct), grid) == 0
    assert grid[0] >= 2 * (n // grid[1]) > topo.G
    posd = pos.cuda().contiguous()
    out = []
    for _ in range(2):
        ws = Workspace(topo)
        _build(lib, ("plain", 0), None, topo, ws, posd, large=False)
        out.append(ws)
    for name in OUTPUTS[:-1]:
        assert torch.equal(getattr(out[0], name), getattr(out[1], name)), name
    w, tp = _arrays(out[0], topo)
    check_graph_properties(w, tp, pos.numpy(), CUTOFF)
    # the rule on sampled targets of the big molecule: radius sources = the first 33 in-range candidates (self included, then
    # dropped) that are not local sources
    E = w["E"]
    p = pos[:n]
    r2 = torch.tensor(CUTOFF) * torch.tensor(CUTOFF)
    capped = uncapped = 0
    for i in list(range(0, n, 257)) + [n - 1]:
        d = p[i][None, :] - p
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        cand = np.nonzero((d2 < r2).numpy())[0]
        capped += cand.size > 33
        uncapped += cand.size <= 33
        keep = cand[:33]
        keep = keep[keep != i]
        lo, hi = w["in_ptr"][i], w["in_ptr"][i + 1]
        src, ty = w["e_src"][lo:hi], w["e_type"][lo:hi]
        loc = set(src[ty > 0].tolist())
        assert src[ty == 0].tolist() == [int(j) for j in keep if int(j) not in loc]
    assert capped and uncapped


def _forward_batch():
    b = batch_with_large([600], seed=31, small=(2, 2))
    return b, _positions(b, 8, False)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_with_a_large_molecule_matches_the_oracle(precision):
    from agdiff_amd import _lib, drugs_model_config, synth
    from oracle import agdiff_oracle as O
    cfg = drugs_model_config()
    m, sd = _gpu_model(cfg, precision=precision)
    b, pos = _forward_batch()
    at, bi, bt, ba = [t(b[k]) for k in ("atom_type", "bond_index", "bond_type", "batch")]
    out = m(at.cuda(), pos.cuda(), bi.cuda(), bt.cuda(), ba.cuda(), None, return_edges=True, extend_order=False)
    inv_g, inv_l, ei, et, elen, lm = [o.cpu().numpy() for o in out]
    assert int(m._batch_cache[2].variant_log.item()) & _lib.DEFINES["AGDIFF_VAR_GRAPH_LARGE"]
    ref = O.forward(sd, cfg, at, pos, bi, bt, ba, extend_order=False)
    assert np.array_equal(ei, ref[2].numpy()) and np.array_equal(et, ref[3].numpy()) and np.array_equal(lm, ref[5].numpy())
    assert rel_err(elen, ref[4].numpy()) < 1e-6
    check_close("large forward inv_g", inv_g, ref[0].numpy(), precision)
    check_close("large forward inv_l", inv_l, ref[1].numpy(), precision)
    # a small batch does not take the large path
    s = synth.make_packed_batch("drugs", 2, 2, seed=3)
    m(t(s["atom_type"]).cuda(), torch.randn(s["atom_type"].shape[0], 3).cuda() * 3, t(s["bond_index"]).cuda(), t(s["bond_type"]).cuda(),
      t(s["batch"]).cuda(), None, extend_order=False)
    assert not int(m._batch_cache[2].variant_log.item()) & _lib.DEFINES["AGDIFF_VAR_GRAPH_LARGE"]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_sampler_with_a_large_molecule_matches_the_oracle(precision):
    """Four steps of langevin_dynamics_sample_diffusion with injected noise on a batch with a 600-atom molecule: the unfused
    front (no AGDIFF_VAR_FUSED_FRONT) with the large build, against the oracle; two runs bitwise identical; model.step_graphs =
    True on such a batch runs launch by launch and gives the same bits."""
    from agdiff_amd import _lib, drugs_model_config
    from oracle import agdiff_oracle as O
    cfg = drugs_model_config(num_diffusion_timesteps=8, beta_end=2e-3)
    m, sd = _gpu_model(cfg, head_scale=1e-2, precision=precision)
    b, _ = _forward_batch()
    at, bi, bt, ba = [t(b[k]) for k in ("atom_type", "bond_index", "bond_type", "batch")]
    N, G, n_steps = at.shape[0], b["num_graphs"], 4
    gen = torch.Generator().manual_seed(19)
    pos_init, noise = torch.randn(N, 3, generator=gen), torch.randn(n_steps, N, 3, generator=gen)
    kw = dict(n_steps=n_steps, step_lr=1e-6, w_global=1.0, global_start_sigma=float("inf"), clip=1000.0)

    def run():
        pos, traj = m.langevin_dynamics_sample_diffusion(at.cuda(), pos_init.cuda(), bi.cuda(), bt.cuda(), ba.cuda(), G,
                                                         extend_order=False, noise=noise.cuda(), **kw)
        log = int(m._batch_cache[2].variant_log.item())
        assert log & _lib.DEFINES["AGDIFF_VAR_GRAPH_LARGE"] and not log & _lib.DEFINES["AGDIFF_VAR_FUSED_FRONT"]
        return pos.cpu(), torch.stack(traj)
    p1, tr1 = run()
    p2, tr2 = run()
    assert torch.equal(p1, p2) and torch.equal(tr1, tr2)
    m.step_graphs = True
    p3, tr3 = run()
    assert torch.equal(p1, p3) and torch.equal(tr1, tr3)
    ref, ref_traj = O.langevin_dynamics_sample_diffusion(sd, cfg, at, pos_init, bi, bt, ba, G, False, noise=noise, **kw)
    check_close("large sampler traj", tr1.numpy(), torch.stack(ref_traj).numpy(), precision)
    check_close("large sampler pos", p1.numpy(), ref.numpy(), precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_loss_with_a_large_molecule_matches_the_oracle(precision):
    from agdiff_amd import drugs_model_config
    from oracle import agdiff_oracle as O
    cfg = drugs_model_config()
    m, sd = _gpu_model(cfg, head_scale=1.0, precision=precision)
    b, pos = _forward_batch()
    at, bi, bt, ba = [t(b[k]) for k in ("atom_type", "bond_index", "bond_type", "batch")]
    G = b["num_graphs"]
    gen = torch.Generator().manual_seed(23)
    time_step = torch.randint(0, cfg.num_diffusion_timesteps, (G,), generator=gen)
    pos_noise = torch.randn(at.shape[0], 3, generator=gen)
    loss, lg, ll = m.get_loss(at.cuda(), pos.cuda(), bi.cuda(), bt.cuda(), ba.cuda(), None, G, return_unreduced_loss=True,
                              extend_order=False, time_step=time_step.cuda(), pos_noise=pos_noise.cuda())
    ref = O.get_loss_diffusion(sd, cfg, at, pos, bi, bt, ba, G, time_step, pos_noise, extend_order=False)
    check_close("large loss global", lg.cpu().numpy(), ref[1].numpy(), precision)
    check_close("large loss local", ll.cpu().numpy(), ref[2].numpy(), precision)
    check_close("large loss", loss.cpu().numpy(), ref[0].numpy(), precision)


def test_driver_samples_a_test_set_with_a_large_molecule():
    """driver.plan_batches + sample_batch end to end: the large molecule gets a batch of its own and is sampled (finite
    positions, every molecule ok), against the oracle for the large batch."""
    from agdiff_amd import driver, drugs_model_config, synth
    from oracle import agdiff_oracle as O
    cfg = drugs_model_config(num_diffusion_timesteps=8, beta_end=2e-3)
    m, sd = _gpu_model(cfg, head_scale=1e-2)
    rng = np.random.default_rng(41)
    mols = []
    for k, n in enumerate([30, 640, 41]):
        at, r, c, ty = large_molecule(rng, n)
        mols.append(dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=ty, num_refs=1, name="m%d" % k, index=k))
    confs = driver.num_confs("2")
    batches = driver.plan_batches(mols, confs, 100000)
    assert len(batches) == 2
    kw = dict(n_steps=3, step_lr=1e-6, w_global=1.0, global_start_sigma=float("inf"), clip=1000.0)
    for bm in batches:
        packed, topo = driver.prepare_batch(m, bm, confs)
        N = packed["atom_type"].shape[0]
        gen = torch.Generator().manual_seed(N)
        pos_init, noise = torch.randn(N, 3, generator=gen), torch.randn(3, N, 3, generator=gen)
        pos, _, ok = driver.sample_batch(m, packed, "cuda:0", kw, pos_init=pos_init, noise=noise, topology=topo)
        assert ok.all() and torch.isfinite(pos).all()
        if topo.large:
            ref, _ = O.langevin_dynamics_sample_diffusion(sd, cfg, t(packed["atom_type"]), pos_init, t(packed["bond_index"]),
                                                          t(packed["bond_type"]), t(packed["batch"]), packed["num_graphs"], False,
                                                          noise=noise, **kw)
            check_close("driver large batch pos", pos.numpy(), ref.numpy(), "f16x3")
