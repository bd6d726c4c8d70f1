"""CPU: the float64 pair-head reference (tests/pair_head_ref.py) against a float32 torch restatement (the oracle's head_mlp: the
reference project's own arithmetic), and the design of the inputs tests/test_hip_pair_head.py runs the kernels on -- which values
the activations are evaluated at, that the hidden layers stay inside the split-fp16 range, that the scores make the normwise figure
meaningful.  Prints, per activation, what float32 torch itself misses float64 by: the figures any `scale=` of the GPU tests cites."""
import numpy as np
import pytest
import torch

import pair_head_ref as R
from helpers import TOL_ELEM, TOL_NORM, elem_err, rel_err


@pytest.fixture(scope="module")
def world():
    from agdiff_amd import qm9_model_config
    from oracle import agdiff_oracle as O
    sd = O.synth_state_dict_for(qm9_model_config(), head_scale=1.0)
    src, dst = R.edges(R.E_SWEEP, R.N_SWEEP)
    return {"A": sd, "rows_A": R.sweep_rows(), "B": sd, "rows_B": R.scaled_rows(), "src": src, "dst": dst, "h": R.node_rows(R.N_SWEEP)}


def _float32_torch(sd, head, act, h, src, dst, attr):
    from oracle import agdiff_oracle as O
    s, d = torch.from_numpy(src).long(), torch.from_numpy(dst).long()
    feat = torch.cat([h[s] * h[d], torch.from_numpy(attr)], dim=-1)
    sd32 = {k: v.float() for k, v in sd.items() if k.startswith(R.HEADS[head])}
    return O.head_mlp(sd32, R.HEADS[head], feat, R.activation(act)).view(-1)


def test_sweep_holds_the_listed_values_and_both_tails():
    rows = R.sweep_rows()
    assert rows.shape == (16 * 13 + 5, 128) and rows.dtype == np.float32
    v = np.sort(np.abs(rows.ravel().astype(np.float64)))
    for x in (0.5, 1.0, 3.0, 6.0, 20.0):
        f = np.float32(x)
        for y in (f, np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(np.inf))):
            assert y in rows and -y in rows, y
    for x in (0.0, 1e-4, 1e-2, 4.1 * np.sqrt(2.0), 8.0, 17.0, 19.9, 20.1, 30.0, 40.0):
        assert np.float32(x) in rows and np.float32(-x) in rows, x
    # the rest: both signs, every decade from 1e-6 up to 40 populated
    for lo in 10.0 ** np.arange(-6, 1):
        for sign in (1.0, -1.0):
            assert np.count_nonzero((sign * rows >= lo) & (sign * rows < 10.0 * lo)) > 1000, (sign, lo)
    assert v[-1] == 40.0
    assert np.array_equal(rows, R.sweep_rows())                       # fixed seed


def test_scatter_indices_are_an_injection_with_position_zero_as_a_mirror():
    for n in (1, 2, 7, R.E_SWEEP):
        pos, mir = R.scatter_indices(n)
        named = np.concatenate([pos, mir[mir >= 0]])
        assert named.min() >= 0 and named.max() < 2 * n and np.unique(named).size == named.size
        assert 0 in mir and np.count_nonzero(mir < 0) == n // 3


@pytest.mark.parametrize("act", R.ACTS)
def test_reference_and_inputs(world, act):
    src, dst, h = world["src"], world["dst"], world["h"]
    for case in ("A", "B"):
        sd, attr = world[case], world["rows_" + case]
        if case == "A":
            sd = R.pass_through_state_dict(sd, act)
        for head in ("global", "local"):
            out, pre1, pre2 = R.pair_head(sd, head, act, h, src, dst, attr)
            assert out.dtype == torch.float64 and out.shape == (R.E_SWEEP,) and pre1.shape == (R.E_SWEEP, 128) and pre2.shape == (R.E_SWEEP, 64)
            R.check_hidden((pre1, R.activation(act)(pre1), pre2, R.activation(act)(pre2)))
            assert torch.isfinite(out).all()
            if case == "A":
                R.check_scores(out)
                assert np.array_equal(pre1.numpy(), attr.astype(np.float64))      # the attribute row IS the first pre-activation
                R.check_sweep_hit(pre1)
            else:
                R.check_bins(pre1)
            f32 = _float32_torch(sd, head, act, h, src, dst, attr)
            rn, re_ = rel_err(f32.numpy(), out.numpy()), elem_err(f32.numpy(), out.numpy())
            print("float32 torch vs float64 %-11s %s %-6s normwise %.2e  elementwise %.2e%s" % (
                act, case, head, rn, re_, "   MISSES the f32 gate" if (rn >= TOL_NORM["f32"] or re_ >= TOL_ELEM["f32"]) else ""))
            assert rn <= 1e-5, (act, case, head, rn)


def test_same_reference_in_float32_is_the_restatement(world):
    """pair_head(dtype=float32) and the oracle's head_mlp are two statements of one formula"""
    sd, attr = world["B"], world["rows_B"]
    a = R.pair_head(sd, "global", "gelu", world["h"], world["src"], world["dst"], attr, dtype=torch.float32)[0]
    b = _float32_torch(sd, "global", "gelu", world["h"], world["src"], world["dst"], attr)
    assert rel_err(a.numpy(), b.numpy()) < 1e-6
