"""Plain-torch float64 restatement of the two pair heads as include/agdiff_hip.h defines them (agdiff_pair_head, agdiff_pair_head_poly):
feat = [h[src] * h[dst] | edge_attr] (256) -> Linear(256, 128) -> act -> Linear(128, 64) -> act -> Linear(64, 1), written from that formula,
plus the inputs the kernel tests are run on (an activation sweep with exact arguments, per-edge scaled random rows, scatter index arrays)
and what those inputs must satisfy.  Test infrastructure only."""
import numpy as np
import torch
import torch.nn.functional as F

HEADS = {"global": "grad_global_dist_mlp", "local": "grad_local_dist_mlp"}     # the state-dict prefixes agdiff_amd/packing.py reads
ACTS = ["relu", "gelu", "silu", "tanh", "sigmoid", "softplus", "leaky_relu", "elu", "celu", "relu6", "hardtanh", "selu", "mish", "hardswish",
        "hardsigmoid", "softsign", "logsigmoid", "hardshrink", "softshrink", "rrelu"]
PAYLOAD_BITS = 0x7FC0BEEF                     # a quiet NaN with a payload: what an entry no launch may touch is pre-filled with
E_SWEEP, N_SWEEP = 16 * 13 + 5, 37            # thirteen full tiles and a partial one; the nodes the edges draw from
HIDDEN_LIMIT = 6.0e4                          # below 65000, where a split-fp16 head flags its source node (csrc/common.hpp)
B_ATTR_MAX = 64.0                             # test B: the per-edge row scale runs geometrically from 1e-3 up to this
B_BINS = ((0.0, 0.5), (0.5, 3.0), (3.0, 6.0), (6.0, 20.0), (20.0, 60.0))


def activation(name):
    """getattr(torch.nn.functional, name) as MultiLayerPerceptron applies it at evaluation (rrelu: training=False; every other
    argument at its default, so celu is elu with alpha 1)"""
    if name == "rrelu":
        return lambda x: F.rrelu(x, training=False)
    return getattr(F, name)


def pair_head(sd, head, act, node_h, src, dst, attr, dtype=torch.float64):
    """(out [E], pre1 [E, 128], pre2 [E, 64]): the head's scores and the two hidden layers before their activation, in `dtype`"""
    p = HEADS[head]
    w = lambda k: sd[p + k].detach().cpu().to(dtype)
    h = torch.as_tensor(node_h).detach().cpu().to(dtype)
    s, d = (torch.as_tensor(np.asarray(x)).long() for x in (src, dst))
    fn = activation(act)
    feat = torch.cat([h[s] * h[d], torch.as_tensor(attr).detach().cpu().to(dtype)], dim=1)
    pre1 = feat @ w(".layers.0.weight").t() + w(".layers.0.bias")
    pre2 = fn(pre1) @ w(".layers.1.weight").t() + w(".layers.1.bias")
    out = fn(pre2) @ w(".layers.2.weight").t() + w(".layers.2.bias")
    return out.view(-1), pre1, pre2


def score_weight(sd, head, act, pre2):
    """[E]: sum_j |w3_j act(pre2)_j| + |b3|, the size of what the last layer adds up -- a score far below it is a cancelled value"""
    w3, b3 = (sd[HEADS[head] + k].detach().cpu().double() for k in (".layers.2.weight", ".layers.2.bias"))
    return activation(act)(pre2).abs() @ w3.abs().view(-1) + b3.abs()


# ------------------------------------------------------------------------------------------------ test A: exact arguments
def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def sweep_listed():
    """float32 values every activation must be seen at: the breakpoints of the switch in csrc/common.hpp (0, +-0.5, +-1, +-3, +-6,
    +-20, +-4.1 sqrt 2) with their two float32 neighbours, and points on the tails"""
    brk = _f32([0.0, 0.5, 1.0, 3.0, 6.0, 20.0, 4.1 * np.sqrt(2.0)])
    brk = np.concatenate([brk, -brk[1:]])
    nb = np.concatenate([brk, np.nextafter(brk, np.float32(np.inf)), np.nextafter(brk, np.float32(-np.inf))])
    tails = _f32([1e-4, 1e-2, 8.0, 17.0, 19.9, 20.1, 30.0, 40.0])
    return np.unique(np.concatenate([nb, tails, -tails]))


def sweep_rows(seed=5):
    """float32 [E_SWEEP, 128]: the listed values, then magnitudes log-spaced over [1e-6, 40] on both signs, dealt to the rows by a
    fixed permutation (every row mixes the ranges)"""
    listed = sweep_listed()
    n = E_SWEEP * 128 - listed.size
    mag = np.logspace(-6.0, np.log10(40.0), n)
    rest = _f32(np.where(np.arange(n) % 2 == 0, mag, -mag))
    v = np.concatenate([listed, rest])
    return v[np.random.default_rng(seed).permutation(v.size)].reshape(E_SWEEP, 128)


def edges(n_edges, n_nodes, seed=11):
    """(src, dst) int32 [n_edges] drawn from [0, n_nodes); edge 1 is a self pair and edges 2, 3 are identical (when they exist)"""
    rng = np.random.default_rng(seed)
    src, dst = (rng.integers(0, n_nodes, n_edges).astype(np.int32) for _ in range(2))
    if n_edges > 1:
        dst[1] = src[1]
    if n_edges > 3:
        src[3], dst[3] = src[2], dst[2]
    return src, dst


def node_rows(n_nodes, seed=13):
    return torch.randn(n_nodes, 128, generator=torch.Generator().manual_seed(seed))


def with_head_weights(sd, head, tensors):
    """A copy of state dict `sd` with the head's tensors {".layers.0.weight": ..} replaced under both of their names (attribute path
    and ModuleList alias)"""
    from agdiff_amd import synth
    out = dict(sd)
    for k in sd:
        leaf = synth.canonical_key(k)[len(HEADS[head]):]
        if synth.canonical_key(k).startswith(HEADS[head] + ".") and leaf in tensors:
            out[k] = tensors[leaf].to(sd[k].dtype).reshape(sd[k].shape).clone()
    return out


def pass_through_state_dict(sd, act, seed=17):
    """`sd` with both heads rewritten for test A, differently for the two heads:
      layers.0         [0 | I], bias 0: hands the attribute row to the first activation unchanged, whatever h[src] * h[dst] is
      layers.1         seeded uniform +-1.7 / sqrt(fan_in), the filler's width; bias +-0.1
      layers.2.weight  seeded uniform +-0.5: wide enough that the bounded activations reach |score| 0.1
      layers.2.bias    minus the float64 median of the sweep's scores under `act`, rounded to float32: an activation with values
                       in (0, 1) would otherwise give scores of one sign"""
    gen = torch.Generator().manual_seed(seed)
    u = lambda *shape, a: (torch.rand(*shape, generator=gen) * 2.0 - 1.0) * a
    rows, none = sweep_rows(), np.zeros(E_SWEEP, dtype=np.int32)
    for head in ("global", "local"):
        w0 = torch.zeros(128, 256)
        w0[:, 128:] = torch.eye(128)
        new = {".layers.0.weight": w0, ".layers.0.bias": torch.zeros(128), ".layers.1.weight": u(64, 128, a=1.7 / np.sqrt(128.0)),
               ".layers.1.bias": u(64, a=0.1), ".layers.2.weight": u(1, 64, a=0.5), ".layers.2.bias": torch.zeros(1)}
        sd = with_head_weights(sd, head, new)
        mid = pair_head(sd, head, act, torch.zeros(1, 128), none, none, rows)[0].median()
        sd = with_head_weights(sd, head, {".layers.2.bias": -mid.float().view(1)})
    return sd


# ------------------------------------------------------------------------------------------------ test B: random weights
def scaled_rows(n_edges=E_SWEEP, seed=19, top=B_ATTR_MAX):
    """float32 [n_edges, 128] ~ N(0, 1), row e times 1e-3 (top / 1e-3)^(e / (n_edges - 1))"""
    base = torch.randn(n_edges, 128, generator=torch.Generator().manual_seed(seed))
    scale = torch.logspace(-3.0, float(np.log10(top)), n_edges)
    return (base * scale[:, None]).float().numpy()


# ------------------------------------------------------------------------------------------------ what the inputs must satisfy
def check_hidden(pres):
    """hidden layers (before and after the activation) inside the split-fp16 range: no flag, no fall-back path"""
    worst = max(float(p.abs().max()) for p in pres)
    assert worst < HIDDEN_LIMIT, worst


def check_scores(out):
    """scores of both signs and not all tiny: the normwise figure divides by max |out|"""
    out = out.numpy()
    assert np.isfinite(out).all() and out.min() < 0.0 < out.max() and np.abs(out).max() >= 0.1, (out.min(), out.max())


def check_sweep_hit(pre1):
    """every listed value is a first-layer pre-activation, exactly"""
    got = np.unique(pre1.numpy())
    missing = [float(v) for v in sweep_listed().astype(np.float64) if v not in got]
    assert not missing, missing


def check_bins(pre1):
    v = pre1.numpy().ravel()
    assert v.max() >= 20.0 and v.min() <= -20.0, (v.min(), v.max())
    for sign in (1.0, -1.0):
        for lo, hi in B_BINS:
            n = int(np.count_nonzero((sign * v >= lo) & (sign * v < hi)))
            assert n >= 16, (sign, lo, hi, n)


# ------------------------------------------------------------------------------------------------ test D: scatter
def scatter_indices(n_edges, seed=23):
    """(pos_index, mir_index) int32 [n_edges]: pos_index a random injection into [0, 2 n_edges); mir_index a free position of its
    own for two edges in three, -1 for the rest.  Position 0 is a MIRROR position: it must be written like any other."""
    perm = np.random.default_rng(seed).permutation(2 * n_edges)
    perm = perm[perm != 0]
    pos = perm[:n_edges].astype(np.int32)
    free = np.concatenate([[0], perm[n_edges:]])
    mir = np.full(n_edges, -1, dtype=np.int32)
    has = np.nonzero(np.arange(n_edges) % 3 != 2)[0]
    mir[has] = free[:has.size]
    return pos, mir


def payload(n, device="cpu"):
    return torch.full((n,), PAYLOAD_BITS, dtype=torch.int32, device=device).view(torch.float32)


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)
