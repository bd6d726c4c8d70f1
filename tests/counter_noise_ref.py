"""Plain-numpy restatement of the counter-based normal generator (include/agdiff_hip.h: agdiff_counter_noise): Philox4x32-10
and the Box-Muller mapping in float64.  Test infrastructure only."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key bumps per round
MASK = 0xFFFFFFFF
POS_INIT_STEP = 0xFFFFFFFF               # c1 reserved for the initial positions (steps = -1)


def philox4x32_10(counter, key):
    """counter: four uint32 words (scalars or arrays that broadcast), key: two -> four uint32 output words (a tuple of arrays)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                    # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return tuple(np.asarray(c, dtype=np.uint32) for c in (c0, c1, c2, c3))


def unit(x):
    """u = ((x >> 8) + 0.5) 2^-24, strictly inside (0, 1)."""
    return ((np.asarray(x, dtype=np.uint32) >> 8).astype(np.float64) + 0.5) * 2.0 ** -24


def normals(seed, stream_ids, graph_sizes, steps):
    """[len(steps), sum(graph_sizes), 3] float64: what agdiff_counter_noise writes for graphs of `graph_sizes` atoms with the
    64-bit `stream_ids`, key `seed` (64-bit) and the counter words `steps` (-1 = the initial positions)."""
    seed = int(seed) & (2 ** 64 - 1)
    sizes = np.asarray(graph_sizes, dtype=np.int64)
    sid = np.repeat(np.asarray([int(s) & (2 ** 64 - 1) for s in stream_ids], dtype=np.uint64), sizes)
    atom = np.concatenate([np.arange(n, dtype=np.uint64) for n in sizes]) if sizes.size else np.zeros(0, dtype=np.uint64)
    c1 = np.asarray([int(s) & MASK for s in steps], dtype=np.uint64)[:, None]
    x0, x1, x2, x3 = philox4x32_10((atom[None, :], c1, (sid & MASK)[None, :], (sid >> 32)[None, :]), (seed & MASK, seed >> 32))
    r0, r1 = np.sqrt(-2.0 * np.log(unit(x0))), np.sqrt(-2.0 * np.log(unit(x2)))
    a0, a1 = 2.0 * np.pi * unit(x1), 2.0 * np.pi * unit(x3)
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1)], axis=-1)
