"""CPU: tests/step_ref.py (the float64 NumPy reference the GPU tests of tests/test_hip_step_kernels.py compare the update and
loss kernels with) anchored against the oracle in float64, against the reference project's recorded G4 arrays, and checked
for the branch coverage the GPU tests rely on."""
import numpy as np
import pytest
import torch

import step_ref as R
from helpers import FORWARD_CASES, check_close, load_golden, rel_err, t
from oracle import agdiff_oracle as O

TIGHT = 1e-12            # two float64 evaluations of the same sums, in different orders
# the branches a setting keeps live (local clip, global clip, clamp): what must engage on 10 % to 90 % of the atoms
LIVE = {"full": (1, 1, 1), "no_global": (1, 0, 1), "no_local": (0, 1, 1), "no_clips": (0, 0, 1), "no_step": (0, 0, 1)}


def _random_graph(seed, sizes, edges_per_atom=6):
    rng = np.random.default_rng(seed)
    batch = np.repeat(np.arange(len(sizes)), sizes)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    pos = rng.standard_normal((batch.shape[0], 3)) * 3.0
    rows, cols = [], []
    for g, n in enumerate(sizes):
        if n < 2:
            continue
        r = rng.integers(0, n, size=edges_per_atom * n)
        c = (r + rng.integers(1, n, size=r.shape[0])) % n            # never a self loop; duplicates and one-way edges allowed
        rows.append(r + ptr[g]); cols.append(c + ptr[g])
    return pos, batch, np.concatenate(rows), np.concatenate(cols), rng


@pytest.mark.parametrize("seed,sizes", [(0, (1, 2, 23, 40)), (1, (65, 1, 7)), (2, (300,))])
def test_eq_term_clip_norm_center_equal_the_oracle_in_float64(seed, sizes):
    pos, batch, row, col, rng = _random_graph(seed, sizes)
    score = rng.standard_normal(row.shape[0])
    ei = torch.from_numpy(np.stack([row, col]))
    p = torch.from_numpy(pos)
    want = O.eq_transform(torch.from_numpy(score).unsqueeze(-1), p, ei, O.get_distance(p, ei).unsqueeze(-1)).numpy()
    got = R.eq_term(pos, row, col, score)
    assert rel_err(got, want) < TIGHT
    for limit in (0.5, 3.0, 1e30):
        assert rel_err(R.clip_norm(got, limit), O.clip_norm(torch.from_numpy(want), limit).numpy()) < TIGHT
    assert np.array_equal(R.clip_norm(got, -1.0), got)
    assert np.abs(np.linalg.norm(R.clip_norm(got, 0.5), axis=1)).max() <= 0.5 * (1 + 1e-15)
    assert rel_err(R.center(pos, batch), O.center_pos(p, torch.from_numpy(batch)).numpy()) < TIGHT


@pytest.mark.parametrize("case", ["g3_forward_qm9_small", "g3_forward_drugs_capped"])
def test_reference_reproduces_the_recorded_g4_arrays(case):
    """eq_local, eq_global, clip_local_20 and center of the reference project's forward fixtures, from the fixture's own edges,
    scores and positions."""
    g = load_golden(case)
    ei, et = g["edge_index"], g["edge_type"]
    lm = et > 0
    eq_l = R.eq_term(g["pos"], ei[0][lm], ei[1][lm], g["edge_inv_local"])
    check_close("step_ref eq_local[%s]" % case, eq_l, g["eq_local"], "f32")
    eq_g = R.eq_term(g["pos"], ei[0][~lm], ei[1][~lm], g["edge_inv_global"].reshape(-1)[~lm])
    check_close("step_ref eq_global[%s]" % case, eq_g, g["eq_global"], "f32")
    # (the fixture clips its own float32 eq_local x 1e4)
    check_close("step_ref clip_local_20[%s]" % case, R.clip_norm(g["eq_local"].astype(np.float64) * 1e4, 20.0), g["clip_local_20"], "f32")
    check_close("step_ref center[%s]" % case, R.center(g["pos"], g["batch"]), g["center"], "f32")


def _oracle_batch(seed=5):
    from agdiff_amd import drugs_model_config, synth
    cfg = drugs_model_config()
    b = synth.make_packed_batch("qm9", 2, 1, seed=seed)
    at, bi, bt, ba = [t(b[k]) for k in ("atom_type", "bond_index", "bond_type", "batch")]
    return cfg, b, at, bi, bt, ba


def test_langevin_step_equals_three_steps_of_the_oracles_update():
    """dualenc.py:506-545 composed from the oracle's eq_transform / clip_norm / center_pos in float64, fed with O.forward's scores
    (a head scale that brings them to order 1), both clips and clip_pos live.  Both sides start every step from the oracle's
    positions."""
    cfg, b, at, bi, bt, ba = _oracle_batch()
    sd = O.synth_state_dict_for(cfg, head_scale=1.0)
    gen = torch.Generator().manual_seed(11)
    pos = torch.randn(at.shape[0], 3, generator=gen, dtype=torch.float64) * 2.0
    kw = dict(sigma=0.7, step_size=0.35, noise_scale=0.5, w_global=0.3, use_global=1)
    engaged = np.zeros(3)
    for step in range(3):
        inv_g, inv_l, ei, et, _, lm = O.forward(sd, cfg, at, pos.float(), bi, bt, ba, extend_order=False)
        inv_g, inv_l = inv_g.double(), inv_l.double()
        eq_l_raw = O.eq_transform(inv_l, pos, ei[:, lm], O.get_distance(pos, ei[:, lm]).unsqueeze(-1))
        eq_g_raw = O.eq_transform(inv_g * (1 - lm.view(-1, 1).double()), pos, ei, O.get_distance(pos, ei).unsqueeze(-1))
        # limits at the median norms of this step's terms: each clip engages on half of the atoms
        clip_local = float(np.float32(eq_l_raw.norm(dim=1).median()))
        clip = float(np.float32(eq_g_raw.norm(dim=1).median()))
        eps = O.clip_norm(eq_l_raw, clip_local) + O.clip_norm(eq_g_raw, clip) * R._s(kw["w_global"])
        noise = torch.randn(at.shape[0], 3, generator=gen, dtype=torch.float64)
        new = O.center_pos(pos + R._s(kw["step_size"]) * eps / R._s(kw["sigma"]) + noise * R._s(kw["noise_scale"]), ba)
        clip_pos = float(np.float32(new.abs().amax(dim=1).median()))
        want = torch.clamp(new, min=-clip_pos, max=clip_pos)
        e = ei.numpy()
        got, masks = R.langevin_step(pos.numpy(), b["batch"], (e[0][lm], e[1][lm], inv_l.numpy()),
                                     (e[0], e[1], inv_g.numpy().reshape(-1), et.numpy()), noise.numpy(),
                                     clip=clip, clip_local=clip_local, clip_pos=clip_pos, **kw)
        assert rel_err(got, want.numpy()) < TIGHT
        assert np.array_equal(masks[0], (eq_l_raw.norm(dim=1) > clip_local).numpy())
        assert np.array_equal(masks[1], (eq_g_raw.norm(dim=1) > clip).numpy())
        assert np.array_equal(masks[2], (new.abs() > clip_pos).any(dim=1).numpy())
        engaged += [m.mean() for m in masks]
        pos = want
    assert np.all(engaged / 3 > 0.3) and np.all(engaged / 3 < 0.7)


def test_perturb_and_diffusion_loss_equal_the_oracle_on_a_two_molecule_batch():
    """O.get_loss_diffusion (float32, return_unreduced_loss form) on two molecules at time steps 1500 and T - 1 (sqrt(1 - a) = 0.26
    and 1.0: d_gt - d_perturbed does not cancel in the oracle's float32); the reference takes the oracle's own edges and the
    scores of O.forward on the perturbed positions.  Gate: the oracle's float32 arithmetic (helpers' f32 gates)."""
    cfg, b, at, bi, bt, ba = _oracle_batch(seed=9)
    sd = O.synth_state_dict_for(cfg, head_scale=1.0)
    gen = torch.Generator().manual_seed(13)
    pos = torch.randn(at.shape[0], 3, generator=gen) * 2.0
    pos_noise = torch.randn(at.shape[0], 3, generator=gen)
    time_step = torch.tensor([1500, cfg.num_diffusion_timesteps - 1])
    want = O.get_loss_diffusion(sd, cfg, at, pos, bi, bt, ba, 2, time_step, pos_noise, extend_order=False)
    _, alphas, _ = O.schedule_tensors(cfg)
    alpha = alphas[time_step].numpy()
    pert64 = R.perturb(pos.numpy(), pos_noise.numpy(), alpha, b["batch"])
    a_pos = alphas[time_step][ba].unsqueeze(-1)
    pert = pos + pos_noise * (1.0 - a_pos).sqrt() / a_pos.sqrt()
    check_close("step_ref perturb", pert64, pert.numpy(), "f32")
    inv_g, inv_l, ei, et, _, lm = O.forward(sd, cfg, at, pert, bi, bt, ba, extend_order=False)
    e, lm = ei.numpy(), lm.numpy()
    got = R.diffusion_loss(pos.numpy(), pert.numpy(), alpha, b["batch"], (e[0][lm], e[1][lm], inv_l.numpy()),
                           (e[0], e[1], inv_g.numpy().reshape(-1), et.numpy()), cfg.cutoff)
    for name, x, y in zip(("total", "global", "local"), got, want):
        check_close("step_ref loss %s" % name, x, y.numpy().reshape(-1), "f32")
    assert (got[1] > 0).any() and (got[2] > 0).any()


@pytest.mark.parametrize("name", list(R.RECIPES))
def test_every_branch_of_the_update_is_taken_in_every_batch(name):
    """What the GPU tests rely on: on every batch recipe, with the scores, noise and limits they use, the reference reports
    10 % to 90 % of the atoms with the local clip engaged, with the global clip engaged and with a clamped coordinate -- on
    the oracle's radius graph of the same positions.  Fixes step_ref.FULL here, not by trial on the GPU."""
    b = R.make_batch(name)
    n = b["pos"].shape[0]
    sizes = np.bincount(b["batch"])
    assert set(R.tail_of(int(sizes.max()))) <= set(sizes.tolist())
    (lr, lc), (rr, rc) = R.reference_edges(b)
    d = b["pos"][rr].astype(np.float64) - b["pos"][rc]
    assert np.sqrt((d * d).sum(1)).max() < R.CUTOFF
    big = np.argmax(sizes)
    if sizes[big] >= 64:      # part of the larger molecules lies beyond the cutoff
        p = b["pos"][b["batch"] == big].astype(np.float64)
        assert (np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1)) > R.CUTOFF).mean() > 0.02
    if name == "dendrimer":
        assert np.bincount(lc, minlength=n)[0] == 52 and np.bincount(lr, minlength=n)[0] == 52
    sl, sg = R.draw_scores(name, lr.shape[0], rr.shape[0])
    noise = R.draw_noise(name, n)
    for label, kw in [("full", R.FULL)] + list(R.ISOLATING.items()):
        sl_ = np.zeros_like(sl) if label == "no_local" else sl
        new, masks = R.langevin_step(b["pos"], b["batch"], (lr, lc, sl_), (rr, rc, sg), noise, **kw)
        assert np.isfinite(new).all()
        for what, m, on in zip(("local clip", "global clip", "clamp"), masks, LIVE[label]):
            if on:
                assert 0.1 <= m.mean() <= 0.9, (name, label, what, float(m.mean()))
