"""CPU: the design of tests/test_hip_row_moves.py's inputs (tests/row_moves_cases.py).  For the reference alone every case stays inside
the gates the GPU tests apply: the float64 restatement (tests/pair_head_ref.py, oracle.agdiff_oracle.mlp_edge_encoder) against its own
float32 evaluation meets helpers.check_close at the exact-fp32 mode's tolerances -- the tightest of the three -- on every list, so a GPU
failure there is the kernel's, not the case's."""
import numpy as np
import pytest
import torch

import pair_head_ref as R
import row_moves_cases as C
from helpers import check_close

_SD = {}


def _sd():
    from agdiff_amd import qm9_model_config
    from oracle import agdiff_oracle as O
    if not _SD:
        cfg = qm9_model_config(mlp_act=C.ACT)
        _SD["sd"], _SD["cfg"] = O.synth_state_dict_for(cfg, head_scale=1.0), cfg
    return _SD["sd"], _SD["cfg"]


def _encoder(sd, length, types, dtype):
    from oracle import agdiff_oracle as O
    sdt = {k: v.to(dtype) for k, v in sd.items() if k.startswith("edge_encoder_global.")}
    return O.mlp_edge_encoder(sdt, "edge_encoder_global", torch.as_tensor(length).to(dtype).view(-1, 1), torch.as_tensor(types).long())


def test_coded_rows_name_their_place():
    for n in (2, 5, 33):
        v = C.coded_rows(n, C.H_LO).numpy()
        assert np.unique(np.abs(v)).size == v.size                       # every (row, feature) has a magnitude of its own
        assert C.H_LO < np.abs(v).min() and np.abs(v).max() <= C.H_LO + 1.0
        assert 255.0 > np.abs(v).max() ** 2                              # (node states the heads multiply: csrc/common.hpp)
        assert 0.3 < (v > 0).mean() < 0.7
    for kind in C.PAIRS:
        for e in C.COUNTS:
            n, src, dst = C.pairs(kind, e)
            assert src.shape == dst.shape == (e,) and 0 <= min(src.min(), dst.min()) and max(src.max(), dst.max()) < n
    n, src, dst = C.pairs("two_nodes", 17)
    assert n == 2 and {(int(a), int(b)) for a, b in zip(src, dst)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    n, src, dst = C.pairs("ends", 16)
    assert {0, n - 1} <= set(src.tolist()) and (0 in dst.tolist() or n - 1 in dst.tolist())
    n, src, dst = C.pairs("one_node", 33)
    assert set(src.tolist()) == {2} and set(dst.tolist()) == {3}


@pytest.mark.parametrize("kind", C.PAIRS)
def test_reference_in_float32_meets_the_gates(kind):
    """every case finds a well-conditioned sign pattern (head_case raises otherwise), and float32 meets the exact-fp32 gates on it"""
    sd, cfg = _sd()
    for e in C.COUNTS:
        for head in ("global", "local"):
            src, dst, h, attr, ref = C.head_case(sd, kind, e, head)
            f32 = R.pair_head(sd, head, C.ACT, h, src, dst, attr, dtype=torch.float32)[0]
            check_close("reference rows %s %s E=%d" % (kind, head, e), f32, ref, "f32")
        zero = np.zeros(e, dtype=np.int64)
        src, dst, h, length, ref = C.head_case(sd, kind, e, "global", encoder=lambda d: _encoder(sd, d, zero, torch.float64), cutoff=cfg.cutoff)
        assert 0.0 < float(length.min()) and float(length.max()) <= cfg.cutoff
        f32 = R.pair_head(sd, "global", C.ACT, h, src, dst, _encoder(sd, length, zero, torch.float32), dtype=torch.float32)[0]
        check_close("reference poly %s E=%d" % (kind, e), f32, ref, "f32")


def test_encoder_rows_in_float32_meet_the_gates():
    sd, cfg = _sd()
    for e in (1, 16, 17):
        types = np.array([1, 2, 3, 12, 23, 24])[np.arange(e) % 6]
        length = C.lengths(e, cfg.cutoff)
        check_close("reference edge_attr E=%d" % e, _encoder(sd, length, types, torch.float32), _encoder(sd, length, types, torch.float64), "f32")


@pytest.mark.parametrize("n", C.NODE_COUNTS)
def test_node_stage_reference_in_float32_meets_the_gates(n):
    import node_ref as NR
    from agdiff_amd import drugs_model_config
    cfg = drugs_model_config()
    sd = NR.state_dict(cfg)
    sd32 = {k: v.float() for k, v in sd.items()}
    h_in, agg = C.node_case(n)
    z = NR.atom_types(n)
    h64, xs64 = NR.stage(NR.to64(sd), cfg, C.NODE_STAGE, h_in, agg, z)
    h32, xs32 = NR.stage(sd32, cfg, C.NODE_STAGE, h_in, agg, z)
    check_close("reference node h n=%d" % n, h32, h64, "f32")
    check_close("reference node h-h_in n=%d" % n, h32.double().numpy() - h_in, h64.numpy() - h_in, "f32")
    check_close("reference node xs n=%d" % n, xs32, xs64, "f32")
