"""GPU (MI355X): the Langevin update -- agdiff_langevin_update (k_langevin_update, csrc/node.hip) and the update phase of
agdiff_sampler_front (k_sampler_front, csrc/front.hip), two hand-maintained copies of the same arithmetic -- and the loss
kernels agdiff_perturb_positions / agdiff_diffusion_loss, each called through its own C-ABI entry point and compared with the
float64 NumPy reference of tests/step_ref.py (anchored on the CPU by tests/test_step_ref_cpu.py).

One launch per setting, no sampler loops.  Scores are seeded random numbers, not network outputs, written straight into
ws.l_inv, ws.e_inv_global (destination order) and ws.inv_r (radius rows), every radius edge with the same value in both
layouts; the local edges (type > 0) of the destination-sorted list carry garbage that the global term must ignore.  The
reference gets the edges the device itself built (the graph build has its own bit-exact tests), so these tests isolate the
update.  Batches (step_ref.RECIPES) put the largest molecule at the last and first size of every launch shape -- lanes per
atom P = 16 / 8 / 4 / 2 / 1, 256 / 512 / 1024 threads -- next to a 1-atom, a 2-atom and a 23-atom molecule; the move is of
the order of the positions, so one missing edge is a percent-level error on its atom.  Every comparison: helpers.check_close
at the "f32" gates."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import step_ref as R
from helpers import TOL_NORM, check_close, t
from test_hip_kernels import _step_args

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
PAD = 96                 # floats past the last atom's row in pos_out / traj_out: nothing may be written there


@functools.lru_cache(maxsize=None)
def _model():
    from agdiff_amd import _lib, drugs_model_config, get_model
    from oracle import agdiff_oracle as O
    cfg = drugs_model_config()
    assert cfg.cutoff == R.CUTOFF
    m = get_model(cfg)
    m.precision = "f32"
    m.load_state_dict({k: v.clone() for k, v in O.synth_state_dict_for(cfg).items()}, strict=True)
    return m.to("cuda:0").eval(), cfg, _lib.load()


class Case:
    """One batch on the device: topology, workspace, graph of `pos`, and that graph's edges read back for the reference."""

    def __init__(self, name, pos=None):
        from agdiff_amd import _lib
        m, cfg, lib = _model()
        b = R.make_batch(name)
        self.name, self.b, self.lib = name, b, lib
        at = t(b["atom_type"]).cuda()
        with torch.no_grad():
            self.pk = m._renorm_embedding(at)
            topo, ws = m._batch(at, t(b["bond_index"]), t(b["bond_type"]), t(b["batch"]), b["num_graphs"], b["extend_order"])
        self.topo, self.ws = topo, ws
        self.N, self.G, self.L = topo.N, topo.G, topo.L
        self.RS = _lib.DEFINES["AGDIFF_RAD_STRIDE"]
        self.pos = (t(b["pos"]) if pos is None else pos).float().cuda().contiguous()
        self.P, self.T, self.W = ctypes.byref(self.pk.struct), ctypes.byref(topo.struct), ctypes.byref(ws.struct)
        self.cutoff = ctypes.c_float(cfg.cutoff)
        st = _lib.stream_ptr()
        assert topo.large == (max(b["sizes"]) > _lib.MAX_ATOMS_PER_GRAPH)
        if topo.large:
            assert lib.agdiff_graph_build_large(None, self.T, self.W, _lib.ptr(self.pos), self.cutoff, 0, st) == 0
        else:
            assert lib.agdiff_graph_build(self.T, self.W, _lib.ptr(self.pos), self.cutoff, st) == 0
        assert lib.agdiff_local_lengths(self.T, self.W, _lib.ptr(self.pos), st) == 0
        torch.cuda.synchronize()
        E = self.E = int(ws.num_edges.item())
        self.e_src, self.e_dst, self.e_type = (getattr(ws, k)[:E].cpu().numpy().astype(np.int64) for k in ("e_src", "e_dst", "e_type"))
        self.t0 = np.nonzero(self.e_type == 0)[0]
        self.loc = (topo.loc_src.cpu().numpy().astype(np.int64), topo.loc_dst.cpu().numpy().astype(np.int64))
        self.rad = (self.e_src[self.t0], self.e_dst[self.t0])
        assert np.all(np.diff(self.e_dst) >= 0)                       # destination order, as draw_scores counts the radius edges
        self.fused = not topo.large
        if self.fused:       # the radius rows of the fused kernel: the same edges, by target
            sa0 = _lib.StepArgs()
            sa0.pos_in = _lib.ptr(self.pos)
            ws.canon_counter.zero_()
            assert lib.agdiff_sampler_front(self.P, self.T, self.W, ctypes.byref(sa0), 2 | 4, self.cutoff, st) == 0
            torch.cuda.synchronize()
            cnt = ws.rad_cnt.cpu().numpy().astype(np.int64)
            self.row_live = np.arange(self.RS)[None, :] < cnt[:, None]
            rsrc = ws.rad_src.view(self.N, self.RS).cpu().numpy()
            assert np.array_equal(rsrc[self.row_live], self.rad[0])
            assert np.array_equal(np.repeat(np.arange(self.N), cnt), self.rad[1])
        self.batch = b["batch"]
        self.graph_ptr = np.concatenate([[0], np.cumsum(b["sizes"])])

    def write_scores(self, s_local, s_radius):
        ws = self.ws
        ws.l_inv.zero_()
        ws.l_inv[: self.L].copy_(t(np.ascontiguousarray(s_local, dtype=np.float32)).cuda())
        junk = np.random.default_rng(1).standard_normal(self.E).astype(np.float32) * 50.0     # on the local edges of the full list
        junk[self.t0] = s_radius
        ws.e_inv_global.zero_()
        ws.e_inv_global[: self.E].copy_(t(junk).cuda())
        if self.fused:
            rows = np.full((self.N, self.RS), 1e3, dtype=np.float32)                          # (slots past a row's count: never read)
            rows[self.row_live] = s_radius
            ws.inv_r.view(self.N, self.RS).copy_(t(rows).cuda())

    def run(self, kernel, kw, noise, in_place=False, traj=True):
        """One launch.  Returns (pos_out, traj_out or None) as float32 arrays [N, 3]; checks nan_flag and the pad."""
        from agdiff_amd import _lib
        ws, n3 = self.ws, 3 * self.N
        buf = torch.full((n3 + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
        trj = torch.full((n3 + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
        if in_place:
            buf[:n3].copy_(self.pos.view(-1))
        pos_in = buf if in_place else self.pos.clone()
        scratch = torch.full((n3,), float("nan"), dtype=torch.float32, device="cuda")
        nz = t(noise).cuda().contiguous()
        sa = _step_args(pos_in, buf, scratch, nz, step_size=kw["step_size"], use_global=kw["use_global"], clip=kw["clip"],
                        clip_local=kw["clip_local"], w_global=kw["w_global"])
        sa.sigma, sa.noise_scale, sa.clip_pos = float(kw["sigma"]), float(kw["noise_scale"]), float(kw["clip_pos"])
        if traj:
            sa.traj_out = _lib.ptr(trj)
        ws.nan_flag.zero_()
        st = _lib.stream_ptr()
        if kernel == "fused":
            assert self.fused
            assert self.lib.agdiff_sampler_front(self.P, self.T, self.W, ctypes.byref(sa), 1, self.cutoff, st) == 0
        else:
            assert self.lib.agdiff_langevin_update(self.T, self.W, ctypes.byref(sa), st) == 0
        torch.cuda.synchronize()
        assert int(ws.nan_flag.abs().sum().item()) == 0
        out, tr = buf.cpu().numpy(), trj.cpu().numpy()
        assert np.all(out[n3:] == SENTINEL) and np.all(tr[n3:] == SENTINEL)
        if not in_place:
            assert torch.equal(pos_in, self.pos)                      # the input is read only
        if not traj:
            assert np.all(tr == SENTINEL)
        return out[:n3].reshape(-1, 3), (tr[:n3].reshape(-1, 3) if traj else None)


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = _case(name)
    s_local, s_radius = R.draw_scores(name, c.L, c.t0.shape[0])
    return s_local, s_radius, R.draw_noise(name, c.N)


@functools.lru_cache(maxsize=None)
def _reference(name, setting):
    """The float64 result of `setting` on batch `name`, computed once and shared (returned arrays are not modified)."""
    c = _case(name)
    s_local, s_radius, noise = _inputs(name)
    kw = R.FULL if setting == "full" else R.ISOLATING[setting]
    if setting == "no_local":
        s_local = np.zeros_like(s_local)
    # the whole destination-sorted list with its types: the reference itself drops what is not type 0
    s_all = np.zeros(c.E, dtype=np.float32)
    s_all[c.t0] = s_radius
    new, masks = R.langevin_step(c.pos.cpu().numpy(), c.batch, c.loc + (s_local,), (c.e_src, c.e_dst, s_all, c.e_type), noise, **kw)
    return new, masks


# (the fused front keeps a molecule in LDS: up to AGDIFF_MAX_ATOMS_PER_GRAPH = 512 atoms)
KERNEL_BATCHES = [(k, n) for n in R.RECIPES for k in ("unfused", "fused") if k == "unfused" or max(R.recipe_sizes(n)) <= 512]
IDS = ["%s-%s" % kb for kb in KERNEL_BATCHES]


def _launch_shape(kernel, sizes):
    """(threads, lanes per atom of the launch) as the launchers choose them (csrc/node.hip, csrc/front.hip)."""
    mx, many = max(sizes), len(sizes) >= 512
    if kernel == "fused":
        bd, parts = (512 if many else 1024), 1
        while parts < 16 and 2 * parts * mx <= bd:
            parts *= 2
        return bd, parts
    bd, parts = 256, 16
    while bd < (512 if many else 1024) and parts * mx > bd:
        bd *= 2
    while parts > 1 and parts * mx > bd:
        parts //= 2
    return bd, parts


def test_the_batches_reach_every_launch_shape():
    """The sizes in step_ref.RECIPES against the launchers' own rules: every P and every block size of the unfused kernel, the
    second pass of the 1025-atom molecule, a.parts at its minimum and at 16 for the fused one, and the 512-thread launch."""
    shapes = {n: _launch_shape("unfused", R.make_batch(n)["sizes"]) for n in R.RECIPES}
    want = {"max16": (256, 16), "max17": (512, 16), "max64": (1024, 16), "max65": (1024, 8), "max128": (1024, 8), "max129": (1024, 4),
            "max256": (1024, 4), "max257": (1024, 2), "max512": (1024, 2), "max513": (1024, 1), "max1025": (1024, 1),
            "many512": (512, 8)}
    assert {n: shapes[n] for n in want} == want
    assert _launch_shape("fused", R.make_batch("mixed")["sizes"]) == (1024, 2)         # (2 x 512 lanes: the fused minimum)
    assert _launch_shape("fused", R.make_batch("small")["sizes"]) == (1024, 16)
    assert _launch_shape("fused", R.make_batch("many512")["sizes"]) == (512, 8)
    c = _case("dendrimer")
    indeg = np.bincount(c.loc[1], minlength=c.N)
    assert indeg[0] == 52 and indeg[0] > 32                           # the centre's local lists: more than a half-wave


@pytest.mark.parametrize("kernel,name", KERNEL_BATCHES, ids=IDS)
def test_full_step_vs_float64_reference(kernel, name):
    """Setting 1: non-zero noise and noise_scale, sigma != 1, w_global = 0.3, use_global = 1, both clips and clip_pos finite,
    traj_out set.  The reference's masks show every branch taken on 10 % to 90 % of the atoms; pos_out against the reference;
    traj_out == pos_out bit for bit; nan_flag all zero (Case.run)."""
    c = _case(name)
    c.write_scores(*_inputs(name)[:2])
    ref, masks = _reference(name, "full")
    for what, m in zip(("local clip", "global clip", "clamp"), masks):
        assert 0.1 <= m.mean() <= 0.9, (what, float(m.mean()))
    out, traj = c.run(kernel, R.FULL, _inputs(name)[2])
    assert np.array_equal(out.view(np.int32), traj.view(np.int32))
    check_close("%s step full[%s]" % (kernel, name), out, ref, "f32")


@pytest.mark.parametrize("kernel,name", KERNEL_BATCHES, ids=IDS)
def test_in_place_step_equals_the_out_of_place_one(kernel, name):
    """Setting 2: pos_out == pos_in, as the sampler runs it (epsnet.py: a.pos_in = a.pos_out), bit for bit the out-of-place
    result; with and without a trajectory row."""
    c = _case(name)
    c.write_scores(*_inputs(name)[:2])
    noise = _inputs(name)[2]
    out, _ = c.run(kernel, R.FULL, noise)
    inp, traj = c.run(kernel, R.FULL, noise, in_place=True)
    assert np.array_equal(out.view(np.int32), inp.view(np.int32))
    assert np.array_equal(out.view(np.int32), traj.view(np.int32))
    inp2, _ = c.run(kernel, R.FULL, noise, in_place=True, traj=False)
    assert np.array_equal(out.view(np.int32), inp2.view(np.int32))
    check_close("%s step in place[%s]" % (kernel, name), inp, _reference(name, "full")[0], "f32")


@pytest.mark.parametrize("setting", list(R.ISOLATING))
@pytest.mark.parametrize("kernel,name", [("unfused", "max65"), ("fused", "mixed")])
def test_one_term_at_a_time(kernel, name, setting):
    """Setting 3: use_global = 0; local scores zero; no clip (clip_local = -1, clip = 1e30); step_size = 0 (centring and
    clamping alone)."""
    c = _case(name)
    s_local, s_radius, noise = _inputs(name)
    c.write_scores(np.zeros_like(s_local) if setting == "no_local" else s_local, s_radius)
    ref, masks = _reference(name, setting)
    assert 0.1 <= masks[2].mean() <= 0.9
    out, traj = c.run(kernel, R.ISOLATING[setting], noise)
    assert np.array_equal(out.view(np.int32), traj.view(np.int32))
    check_close("%s step %s[%s]" % (kernel, setting, name), out, ref, "f32")
    if setting == "no_step":         # (and not the full step's result)
        assert np.abs(out - _reference(name, "full")[0]).max() > 0.1


@pytest.mark.parametrize("kernel", ["unfused", "fused"])
def test_rows_depend_on_their_own_molecule_only(kernel):
    """Setting 4 on the mixed batch: nothing is written past 3 N (Case.run checks the sentinel pad of pos_out and traj_out in
    every launch of this module), and with the scores and the noise of ONE molecule changed every other molecule keeps its
    bits."""
    name = "mixed"
    c = _case(name)
    s_local, s_radius, noise = _inputs(name)
    c.write_scores(s_local, s_radius)
    base, _ = c.run(kernel, R.FULL, noise)
    for g in (4, 7, 12):                                              # the 33-, the 128- and the 23-atom molecule (the last one)
        lo, hi = c.graph_ptr[g], c.graph_ptr[g + 1]
        mine = lambda idx: (idx >= lo) & (idx < hi)
        s_l2, s_r2, nz2 = s_local.copy(), s_radius.copy(), noise.copy()
        s_l2[mine(c.loc[0])] *= -1.5
        s_r2[mine(c.rad[0])] *= -1.5
        nz2[lo:hi] += 1.0
        c.write_scores(s_l2, s_r2)
        out, _ = c.run(kernel, R.FULL, nz2)
        other = ~mine(np.arange(c.N))
        assert np.array_equal(out[other].view(np.int32), base[other].view(np.int32)), g
        assert np.abs(out[lo:hi] - base[lo:hi]).max() > 0.1


# ------------------------------------------------------------------------------------------------- loss kernels
@functools.lru_cache(maxsize=None)
def _loss_setup():
    """The loss batch (dendrimer, 1, 85, 86, 300 atoms), every graph with an alpha of the model's own schedule -- the first and
    the last time step among them --, perturbed on the device, graph and local lengths built on the perturbed positions."""
    from agdiff_amd import _lib
    m, cfg, lib = _model()
    b = R.make_batch("loss")
    time_step = torch.tensor([2500, 100, 0, cfg.num_diffusion_timesteps - 1, 1500])
    alpha = m.alphas.detach().cpu()[time_step].to(torch.float32).contiguous()
    noise = R.draw_noise("loss", b["pos"].shape[0])
    c0 = Case("loss")
    pert = torch.full((3 * c0.N + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    a_dev, nz = alpha.cuda(), t(noise).cuda()
    assert lib.agdiff_perturb_positions(c0.T, _lib.ptr(c0.pos), _lib.ptr(nz), _lib.ptr(a_dev), _lib.ptr(pert), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((pert[3 * c0.N:] == SENTINEL).all())
    pert = pert[: 3 * c0.N].view(-1, 3).clone()
    return b, alpha.numpy(), noise, pert, a_dev, Case("loss", pos=pert)


def test_perturb_positions_vs_float64_reference():
    """k_perturb_positions on molecules of 1, 85, 86 and 300 atoms (3 n = 3, 255, 258, 900: below, at the edge of and several
    rounds of its 256 threads) and the 53-atom dendrimer."""
    b, alpha, noise, pert, _, _ = _loss_setup()
    assert alpha.max() > 0.99999 and alpha.min() < 0.01
    check_close("perturb_positions", pert, R.perturb(b["pos"], noise, alpha, b["batch"]), "f32")


@pytest.mark.parametrize("roles", ["all", "row<col", "row>col"])
def test_diffusion_loss_vs_float64_reference(roles):
    """k_diffusion_loss: (total, global, local) rows against step_ref.diffusion_loss, with random scores on every edge, then only
    on the edges with row < col, then only on those with row > col: an atom then meets a scored edge either as its row or as
    its column, so a sign or index slip in one of the four loops (local / global x out / in) cannot cancel against its mirror.
    The build never emits a type-0 edge longer than the cutoff (asserted below), so the kernel's d <= cutoff mask stays true
    in these runs; lengths are not forged to exercise it.
    Compared per graph.  d_target = (d_gt - d_pert) sqrt(a) / sqrt(1 - a) subtracts two float32 distances that differ by
    O(sqrt(1 - a)): at the first time step (1 - a = 5e-6) their rounding alone, amplified 444 times, moves the loss by ~5e-5
    relative (float32 distances emulated in NumPy), in the kernel as in the reference project's own float32 arithmetic.  A graph's gate is therefore the larger of
    the f32 gate and what step_ref's model of that rounding (FLOAT32_DISTANCE on both distances, independent per edge) gives
    for it, computed from the inputs alone; measured: see the parity record (scale 1 for the graphs at t >= 1500)."""
    from agdiff_amd import _lib
    b, alpha, _, pert, a_dev, c = _loss_setup()
    assert float(c.ws.e_len[: c.E][torch.from_numpy(c.t0).cuda()].max()) <= R.CUTOFF
    s_local, s_radius = R.draw_scores("loss", c.L, c.t0.shape[0])
    if roles != "all":
        keep = (lambda r, k: r < k) if roles == "row<col" else (lambda r, k: r > k)
        s_local = np.where(keep(*c.loc), s_local, 0.0).astype(np.float32)
        s_radius = np.where(keep(*c.rad), s_radius, 0.0).astype(np.float32)
    c.write_scores(s_local, s_radius)
    pos_gt = t(b["pos"]).cuda().contiguous()
    loss = torch.full((3 * c.N + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    assert c.lib.agdiff_diffusion_loss(c.P, c.T, c.W, _lib.ptr(pos_gt), _lib.ptr(pert), _lib.ptr(a_dev), _lib.ptr(loss),
                                       _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((loss[3 * c.N:] == SENTINEL).all())
    got = loss[: 3 * c.N].view(3, -1).cpu().numpy()
    s_all = np.zeros(c.E, dtype=np.float32)
    s_all[c.t0] = s_radius
    ref = R.diffusion_loss(b["pos"], pert.cpu().numpy(), alpha, b["batch"], c.loc + (s_local,), (c.e_src, c.e_dst, s_all, c.e_type),
                           R.CUTOFF, rounding=True)
    assert (ref[1] > 0).any() and (ref[2] > 0).any()
    for g in range(c.G):
        lo, hi = c.graph_ptr[g], c.graph_ptr[g + 1]
        if ref[0][lo:hi].max() == 0.0:                               # (the 1-atom molecule: no edge, no loss)
            assert np.all(got[:, lo:hi] == 0.0)
            continue
        for k, row in enumerate(("total", "global", "local")):
            if ref[k][lo:hi].max() > 0.0:
                model = float(ref[3][k][lo:hi].max() / ref[k][lo:hi].max())
                scale = max(1.0, model / TOL_NORM["f32"])
                print("graph %d (%d atoms, alpha %.7f) %s: rounding model %.2e -> gate scale %.1f" % (g, hi - lo, alpha[g], row, model, scale))
                check_close("diffusion_loss %s[%s, graph %d]" % (row, roles, g), got[k, lo:hi], ref[k][lo:hi], "f32", scale=scale)
