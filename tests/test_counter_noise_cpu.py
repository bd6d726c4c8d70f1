"""CPU: the counter-based noise mode's host side -- the numpy restatement of the generator against the published
Philox4x32-10 vectors, stream-id packing, and the ids' way through pack_batch / subset_batch / shard_of and two different
plans of the same job.  Nothing here computes on a GPU."""
import numpy as np
import pytest

import counter_noise_ref as R
from agdiff_amd import _lib, driver, synth
from agdiff_amd.dist import shard_of


def _mols(k=6, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(k):
        at, r, c, t = synth.random_molecule(rng, int(rng.integers(8, 20)))
        out.append(dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=t, num_refs=2 + i % 3, name="m%d" % i, index=10 + 3 * i))
    return out


@pytest.mark.parametrize("counter,key,expect", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_restatement_reproduces_the_published_philox4x32_10_vectors(counter, key, expect):
    assert tuple(int(x) for x in R.philox4x32_10(counter, key)) == expect
    # ... and element-wise on arrays, as `normals` calls it
    got = R.philox4x32_10(tuple(np.full((2, 3), c, dtype=np.uint64) for c in counter), key)
    assert all(np.all(g == e) for g, e in zip(got, expect))


def test_restatement_mapping_counter_words_and_range():
    """u lies strictly inside (0, 1) at both ends of the word range, so no draw is infinite and |z| <= sqrt(50 ln 2) = 5.887; the
    counter words are (atom in graph, step, id low, id high) and the key the two halves of the seed."""
    assert R.unit(0) == 2.0 ** -25 and R.unit(0xFFFFFFFF) == 1.0 - 2.0 ** -25
    assert np.sqrt(-2.0 * np.log(R.unit(0))) < 5.9
    seed, ids, sizes, steps = (7 << 32) | 5, [(9 << 32) | 4, 2 ** 63 - 1], [3, 2], [0, 11, -1]
    z = R.normals(seed, ids, sizes, steps)
    assert z.shape == (3, 5, 3) and np.isfinite(z).all()
    for (s, a, g, la) in ((1, 1, 0, 1), (2, 4, 1, 1), (0, 3, 1, 0)):       # (row, atom, its graph, its index there)
        c1 = 0xFFFFFFFF if steps[s] < 0 else steps[s]
        x = R.philox4x32_10((la, c1, ids[g] & 0xFFFFFFFF, ids[g] >> 32), (5, 7))
        u = [float(R.unit(v)) for v in x]
        r0, r1 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
        want = [r0 * np.cos(2 * np.pi * u[1]), r0 * np.sin(2 * np.pi * u[1]), r1 * np.cos(2 * np.pi * u[3])]
        assert np.allclose(z[s, a], want, rtol=0, atol=1e-15)
    # the same graph elsewhere in another batch, or alone: the same numbers
    alone = R.normals(seed, ids[1:], sizes[1:], steps)
    assert np.array_equal(alone, z[:, 3:])


def test_stream_id_packing_and_unpacking():
    assert driver.stream_id(0, 0) == 0
    assert driver.stream_id(17, 3) == (17 << 32) | 3 and driver.stream_id(17, 3, 1) == (17 << 32) | (1 << 24) | 3
    top = driver.stream_id(2 ** 31 - 1, 2 ** 24 - 1, 255)
    assert top == 2 ** 63 - 1 and driver.split_stream_id(top) == (2 ** 31 - 1, 2 ** 24 - 1, 255)
    assert driver.split_stream_id(driver.stream_id(5, 6, 7)) == (5, 6, 7)
    ids = driver.stream_id(4, np.arange(5))
    assert ids.dtype == np.int64 and ids.tolist() == [(4 << 32) + k for k in range(5)]
    m, c, a = driver.split_stream_id(driver.with_attempt(ids, 2))
    assert m.tolist() == [4] * 5 and c.tolist() == list(range(5)) and a.tolist() == [2] * 5
    assert np.array_equal(driver.with_attempt(driver.with_attempt(ids, 2), 0), ids)
    # all ids of a job are distinct: (molecule, conformer, attempt) -> id is one to one
    grid = driver.stream_id(np.arange(3)[:, None, None], np.arange(4)[None, :, None], np.arange(2)[None, None, :])
    assert np.unique(grid).size == 24


@pytest.mark.parametrize("args", [(0, 1 << 24), (0, -1), (0, 0, 256), (0, 0, -1), (-1, 0), (1 << 31, 0)])
def test_stream_id_rejects_out_of_range_fields(args):
    with pytest.raises(ValueError):
        driver.stream_id(*args)
    with pytest.raises(ValueError):
        driver.stream_id(*(np.asarray([0, a]) for a in args))


def test_with_attempt_rejects_attempt_256():
    with pytest.raises(ValueError):
        driver.with_attempt(driver.stream_id(1, np.arange(3)), 256)


def test_ids_travel_with_the_graphs_through_pack_subset_and_shard():
    mols = _mols(5)
    confs = driver.num_confs("2x")
    packed = driver.pack_batch(mols, confs)
    ids = packed["stream_ids"]
    assert ids.dtype == np.int64 and ids.shape == (packed["num_graphs"],)
    want = np.concatenate([driver.stream_id(m["index"], np.arange(confs(m["num_refs"]))) for m in mols])
    assert np.array_equal(ids, want)
    # every node's graph carries the id of (its molecule, its conformer)
    for m, (off, n, g) in zip(mols, packed["spans"]):
        for c in range(g):
            assert ids[packed["batch"][off + c * n]] == driver.stream_id(m["index"], c)
    sub = driver.subset_batch(packed, [3, 1])
    ref = np.concatenate([driver.stream_id(mols[k]["index"], np.arange(confs(mols[k]["num_refs"]))) for k in (3, 1)])
    assert np.array_equal(sub["stream_ids"], ref) and sub["stream_ids"].shape == (sub["num_graphs"],)
    seen = []
    for rank in range(3):
        part, (g0, g1), (lo, hi) = shard_of(sub, rank, 3)
        assert part is not None and np.array_equal(part["stream_ids"], sub["stream_ids"][g0:g1])
        assert part["stream_ids"].shape == (part["num_graphs"],)
        seen.append(part["stream_ids"])
    assert np.array_equal(np.concatenate(seen), sub["stream_ids"])
    # molecules without an index (hand-made lists): no ids, and counter noise is refused instead of inventing some
    bare = [{k: v for k, v in m.items() if k != "index"} for m in mols[:2]]
    p2 = driver.pack_batch(bare, confs)
    assert "stream_ids" not in p2 and "stream_ids" not in driver.subset_batch(p2, [1])
    with pytest.raises(ValueError):
        driver.sample_batch(object(), p2, "cpu", {}, counter_seed=1)


def test_two_plans_of_the_same_job_give_every_conformer_the_same_id():
    """--max-atoms changes which molecules share a batch and where a conformer's graph sits in it, never its id."""
    mols = _mols(6)
    confs = driver.num_confs("2x")

    def ids_of(max_atoms):
        out, shapes = {}, []
        for bm in driver.plan_batches(mols, confs, max_atoms):
            p = driver.pack_batch(bm, confs)
            shapes.append(tuple(m["index"] for m in bm))
            g0 = 0
            for m, (_, _, g) in zip(bm, p["spans"]):
                for c in range(g):
                    out[(m["index"], c)] = int(p["stream_ids"][g0 + c])
                g0 += g
        return out, shapes
    a, plan_a = ids_of(10 ** 6)
    b, plan_b = ids_of(120)
    assert plan_a != plan_b and len(plan_b) > len(plan_a) == 1
    assert a == b and len(a) == sum(confs(m["num_refs"]) for m in mols)
    assert all(v == driver.stream_id(k[0], k[1]) for k, v in a.items())
    # a resumed job plans over the molecules still missing: the ids stay
    rest = [m for m in mols if m["index"] not in (10, 16)]
    for bm in driver.plan_batches(rest, confs, 120):
        p = driver.pack_batch(bm, confs)
        g0 = 0
        for m, (_, _, g) in zip(bm, p["spans"]):
            assert [int(x) for x in p["stream_ids"][g0:g0 + g]] == [a[(m["index"], k)] for k in range(g)]
            g0 += g


def test_run_job_and_sample_batch_argument_checks():
    with pytest.raises(ValueError):
        driver.run_job(object(), [], "unused", driver.num_confs("1"), 10, {}, "cpu", noise="philox")

    class _Stub:                                     # a model without begin_sampling / counter_normals
        def langevin_dynamics_sample_diffusion(self, **kw):
            raise AssertionError("not reached")
    packed = driver.pack_batch(_mols(2), driver.num_confs("1"))
    with pytest.raises(ValueError):
        driver.sample_batch(_Stub(), packed, "cpu", {}, counter_seed=3)


def test_abi_exports_the_counter_noise_entry_point():
    import ctypes
    assert _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    assert _lib.EXPORTS["agdiff_counter_noise"] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int32,
                                                    ctypes.c_void_p, ctypes.c_void_p]
    lib = _lib.load()
    assert lib.agdiff_abi_version() == 48 and lib.agdiff_counter_noise.argtypes[2] is ctypes.c_uint64
    # argument checks run on the host, before any launch
    topo = _lib.Topo()
    assert lib.agdiff_counter_noise(None, None, 0, None, 1, None, None) == -1
    assert lib.agdiff_counter_noise(ctypes.byref(topo), ctypes.c_void_p(8), 0, ctypes.c_void_p(8), -1, ctypes.c_void_p(8), None) == -1
    assert lib.agdiff_counter_noise(ctypes.byref(topo), ctypes.c_void_p(8), 0, ctypes.c_void_p(8), 0, ctypes.c_void_p(8), None) == 0
    topo.num_nodes, topo.num_graphs = 4, 1          # (graph_ptr still null)
    assert lib.agdiff_counter_noise(ctypes.byref(topo), ctypes.c_void_p(8), 0, ctypes.c_void_p(8), 1, ctypes.c_void_p(8), None) == -1
