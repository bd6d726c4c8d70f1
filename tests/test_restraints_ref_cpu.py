"""CPU: the float64 restatement of the distance-restraint sweep (tests/restraints_ref.py) anchored by known answers, so that the
GPU comparison in tests/test_hip_restraints.py rests on something.  KNOWN lists the answers that test repeats on the GPU."""
import numpy as np

import restraints_ref as R


def _two(d=5.0):
    """Two atoms d apart along a skew direction, plus a bystander, in one graph."""
    u = np.array([2.0, -1.0, 2.0]) / 3.0
    pos = np.array([[1.0, 2.0, -1.0], [1.0, 2.0, -1.0], [7.0, 7.0, 7.0]]) + np.outer([0.0, d, 0.0], u)
    return pos.astype(np.float32), np.zeros(3, dtype=np.int64)


def test_one_pair_lands_on_its_upper_bound_and_keeps_its_centroid():
    pos, batch = _two(5.0)
    out, viol, written = R.restrain_pairs(pos, [[0, 1]], [0.0], [3.0], batch)
    assert abs(R.distances(out, [[0, 1]])[0] - 3.0) < 1e-6 and abs(viol[0] - 2.0) < 1e-6
    assert np.abs(out[:2].astype(np.float64).mean(0) - pos[:2].astype(np.float64).mean(0)).max() < 1e-6
    assert np.array_equal(out[2], pos[2]) and written.tolist() == [True, True, False]
    assert abs(np.linalg.norm(out[0].astype(np.float64) - pos[0]) - 1.0) < 1e-6           # each end moves half of the 2 Angstrom


def test_with_one_end_fixed_the_other_moves_the_whole_way():
    pos, batch = _two(5.0)
    out, _, _ = R.restrain_pairs(pos, [[0, 1]], [0.0], [3.0], batch, fixed=[1, 0, 0])
    assert np.array_equal(out[0], pos[0]) and abs(np.linalg.norm(out[1].astype(np.float64) - pos[1]) - 2.0) < 1e-6
    assert abs(R.distances(out, [[0, 1]])[0] - 3.0) < 1e-6
    out, _, _ = R.restrain_pairs(pos, [[0, 1]], [0.0], [3.0], batch, fixed=[1, 1, 0])     # both ends fixed: nothing moves
    assert np.array_equal(out, pos)


def test_a_lower_bound_pushes_the_atoms_apart():
    pos, batch = _two(2.0)
    out, viol, _ = R.restrain_pairs(pos, [[1, 0]], [3.5], [np.inf], batch)
    assert abs(R.distances(out, [[0, 1]])[0] - 3.5) < 1e-6 and abs(viol[0] - 1.5) < 1e-6


def test_inside_the_window_the_bytes_are_unchanged():
    pos, batch = _two(4.0)
    pos[0, 0] = -0.0                                       # (a signed zero is kept too)
    d = float(R.distances(pos, [[0, 1]])[0])
    for lo, hi in ((0.7 * d, 1.3 * d), (0.0, np.inf), (d - 1e-3, d + 1e-3)):
        out, viol, _ = R.restrain_pairs(pos, [[0, 1]], [lo], [hi], batch, sweeps=3)
        assert out.tobytes() == pos.tobytes() and viol[0] == 0.0


def test_a_hub_divides_each_entry_by_its_row_length():
    rng = np.random.default_rng(2)
    k = 5
    pos = np.concatenate([np.zeros((1, 3)), rng.normal(size=(k, 3)) * 4.0]).astype(np.float32)
    batch = np.zeros(k + 1, dtype=np.int64)
    pairs = [[0, j] for j in range(1, k + 1)]
    d = R.distances(pos, pairs)
    out, _, _ = R.restrain_pairs(pos, pairs, np.zeros(k), 0.5 * d, batch)
    # the hub: the mean of the k single-pair moves (each half of its violation towards the partner); a leaf: its own half move
    want = sum(0.5 * (0.5 * d[j - 1]) * (pos[j].astype(np.float64) / d[j - 1]) for j in range(1, k + 1)) / k
    assert np.abs(out[0] - want).max() < 1e-6
    for j in range(1, k + 1):
        assert abs(np.linalg.norm(out[j].astype(np.float64) - pos[j]) - 0.25 * d[j - 1]) < 1e-6


def test_a_pair_listed_twice_counts_twice():
    pos, batch = _two(5.0)
    once, _, _ = R.restrain_pairs(pos, [[0, 1]], [0.0], [3.0], batch)
    twice, _, _ = R.restrain_pairs(pos, [[0, 1], [0, 1]], [0.0, 0.0], [3.0, 3.0], batch)
    assert np.abs(once.astype(np.float64) - twice).max() < 1e-6          # two equal entries over a row of length two


def test_two_sweeps_equal_two_one_sweep_calls():
    c = R.case("strong")
    a, va, _ = R.restrain_pairs(c["pos"], c["pairs"], c["lo"], c["hi"], c["batch"], weight=0.5, sweeps=2)
    b1, vb, _ = R.restrain_pairs(c["pos"], c["pairs"], c["lo"], c["hi"], c["batch"], weight=0.5, sweeps=1)
    b2, _, _ = R.restrain_pairs(b1, c["pairs"], c["lo"], c["hi"], c["batch"], weight=0.5, sweeps=1)
    assert a.tobytes() == b2.tobytes() and np.array_equal(va, vb) and a.tobytes() != b1.tobytes()


def test_half_the_weight_moves_half_as_far_on_the_first_sweep():
    c = R.case("strong")
    full, _, _ = R.restrain_pairs(c["pos"], c["pairs"], c["lo"], c["hi"], c["batch"], weight=1.0)
    half, _, _ = R.restrain_pairs(c["pos"], c["pairs"], c["lo"], c["hi"], c["batch"], weight=0.5)
    p = c["pos"].astype(np.float64)
    assert np.abs((half - p) - 0.5 * (full - p)).max() < 4e-6 and np.abs(full - p).max() > 0.1


def test_zero_sweeps_only_measure_and_coincident_atoms_do_not_move():
    c = R.case("mild")
    out, viol, _ = R.restrain_pairs(c["pos"], c["pairs"], c["lo"], c["hi"], c["batch"], sweeps=0)
    assert out.tobytes() == c["pos"].tobytes()
    per_pair = R.violations(c["pos"], c["pairs"], c["lo"], c["hi"])
    for g in range(c["G"]):
        rows = c["batch"][c["pairs"][:, 0]] == g
        assert viol[g] == (per_pair[rows].max() if rows.any() else 0.0)
    assert viol[0] == 0.0 and viol[1] == 0.0 and (viol[2:] > 0.01).all()
    pos = np.zeros((2, 3), dtype=np.float32) + 1.5
    out, viol, _ = R.restrain_pairs(pos, [[0, 1]], [1.0], [2.0], np.zeros(2, dtype=np.int64))
    assert out.tobytes() == pos.tobytes() and viol[0] == 1.0


def test_skipped_and_non_finite_graphs_are_left_alone():
    c = R.case("strong")
    skip = np.zeros(7, dtype=np.int32)
    skip[4] = 1
    pos = c["pos"].copy()
    bad = np.nonzero((c["batch"] == 6) & (c["rows"] > 0))[0][100]
    pos[bad, 1] = np.nan
    out, viol, written = R.restrain_pairs(pos, c["pairs"], c["lo"], c["hi"], c["batch"], skip=skip)
    for g in (4, 6):
        rows = c["batch"] == g
        assert np.isnan(viol[g]) and out[rows].tobytes() == pos[rows].tobytes() and not written[rows].any()
    assert np.isfinite(viol[[0, 1, 2, 3, 5]]).all() and out[c["batch"] == 5].tobytes() != pos[c["batch"] == 5].tobytes()


def test_the_violation_of_a_consistent_set_does_not_increase():
    """A set of windows that some configuration satisfies (here: all windows contain the pairs' distances in a TARGET geometry),
    started from another geometry: the largest violation never goes up over 50 one-sweep calls, and comes down."""
    rng = np.random.default_rng(9)
    n = 24
    target = rng.uniform(-5.0, 5.0, size=(n, 3))
    pairs = np.asarray([(i, j) for i in range(n) for j in range(i + 1, n) if (i + 2 * j) % 5 == 0], dtype=np.int32)
    d = R.distances(target, pairs)
    lo, hi = (0.9 * d).astype(np.float32), (1.1 * d).astype(np.float32)
    batch = np.zeros(n, dtype=np.int64)
    pos = (target + rng.normal(size=(n, 3)) * 1.0).astype(np.float32)
    seen = []
    for _ in range(50):
        pos, viol, _ = R.restrain_pairs(pos, pairs, lo, hi, batch, weight=1.0, sweeps=1)
        seen.append(viol[0])
    assert all(b_ <= a + 1e-6 for a, b_ in zip(seen, seen[1:])), seen
    assert seen[0] > 0.5 and seen[-1] < 0.25 * seen[0]


KNOWN = ("upper bound", "fixed end", "lower bound", "inside")
