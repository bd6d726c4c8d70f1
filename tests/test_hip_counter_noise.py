"""GPU (MI355X): the counter-based noise mode.  agdiff_counter_noise against the numpy restatement of the generator
(tests/counter_noise_ref.py), its statistics, and what the mode is for: a conformer's draws -- and with them its sample -- do
not depend on the batch it is packed into, on how the batch is sharded, on --max-atoms, on a resume or on a neighbour's retry."""
import os
import socket

import numpy as np
import pytest
import torch

import counter_noise_ref as R
from helpers import check_close, t

pytestmark = pytest.mark.gpu

PREC = "f16x3"          # the default arithmetic mode: what tests/helpers.check_close gates the positions in
SEED = 0x9E3779B97F4A7C15        # (a key with both 32-bit halves in use)


def _model(T=8, **cfg_kw):
    from agdiff_amd import get_model, qm9_model_config, synth
    m = get_model(qm9_model_config(num_diffusion_timesteps=T, **cfg_kw))
    m.load_state_dict(synth.synth_state_dict(m.state_dict()))
    return m.to("cuda:0").eval()


def _mols(sizes, refs, first_index=0, seed=5):
    from agdiff_amd import synth
    rng = np.random.default_rng(seed)
    out = []
    for i, (n, g) in enumerate(zip(sizes, refs)):
        at, r, c, ty = synth.random_molecule(rng, n)
        out.append(dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=ty, num_refs=g, name="mol%d" % i, index=first_index + i))
    return out


CONFS = lambda num_refs: num_refs          # conformers per molecule = its num_refs field


def _run_counter(m, part, seed, n_steps=8, **kw):
    """One counter-mode run over `part` (a packed batch, or a graph range of one, with its stream_ids): (pos_init, noise rows
    [steps, N, 3], final pos, variant_log word, the run)."""
    a = [t(part[k]).cuda() for k in ("atom_type", "bond_index", "bond_type", "batch")]
    p0 = m.counter_normals(part["batch"], part["stream_ids"], seed, [-1])[0]
    run = m.begin_sampling(a[0], p0, a[1], a[2], a[3], part["num_graphs"], False, n_steps=n_steps, w_global=1.0, clip=1000.0,
                           noise_mode="counter", noise_seed=seed, stream_ids=part["stream_ids"], **kw)
    run.advance(run.remaining())
    pos, _ = run.finish()
    assert run.global_steps == n_steps                      # the global branch ran on every step
    assert run._nz.shape[0] == n_steps and run._nz_base == 0
    return p0.cpu(), run._nz.cpu(), pos.cpu(), int(run.ws.variant_log.item()), run


def _compare_positions(name, got, ref):
    same = bool(torch.equal(got, ref))
    print("%s: positions bitwise equal: %s (max |diff| %.3e)" % (name, same, float((got - ref).abs().max())))
    check_close(name, got, ref, PREC)
    return same


# ------------------------------------------------------------------------------------------------ 1. kernel against restatement
def test_kernel_matches_the_float64_restatement():
    """Graphs of unequal size (one atom, one past the 512-atom small path), ids with a set high word and the largest
    non-negative one, steps 0, T - 1 and -1 (pos_init): every value within 1e-5 of the float64 restatement -- fp32 log, sqrt and
    sincos at r <= 5.9 leave ~1e-6; a wrong counter word or key half is an O(1) error -- and a second call gives the same bits."""
    from agdiff_amd import driver
    from agdiff_amd.topology import BatchTopology
    m = _model()
    T = 5000
    sizes = [5, 1, 300, 17, 600, 64]
    ids = [0, 3, (1 << 32) + 5, 2 ** 63 - 1, driver.stream_id(123456, 77, 9), 123456789]
    steps = [0, T - 1, -1, 7]
    batch = np.repeat(np.arange(len(sizes)), sizes)
    ref = R.normals(SEED, ids, sizes, steps)
    got = m.counter_normals(batch, np.asarray(ids, dtype=np.int64), SEED, steps)
    assert got.shape == (len(steps), sum(sizes), 3) and got.dtype == torch.float32 and got.device.type == "cuda"
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    print("agdiff_counter_noise vs float64 restatement: max |diff| %.3e over %d values" % (err, ref.size))
    assert err < 1e-5
    again = m.counter_normals(torch.from_numpy(batch).cuda(), torch.tensor(ids, dtype=torch.int64), SEED, torch.tensor(steps))
    assert torch.equal(got, again)
    # rows are functions of their own step only: asked for alone, or in another order, the same bits
    assert torch.equal(m.counter_normals(batch, ids, SEED, [-1])[0], got[2])
    assert torch.equal(m.counter_normals(batch, ids, SEED, [7, 0]), got[[3, 0]])
    # ... and graphs of their own id only: the last three graphs alone
    tail = m.counter_normals(np.repeat(np.arange(3), sizes[3:]), ids[3:], SEED, steps)
    assert torch.equal(tail, got[:, sum(sizes[:3]):])
    # many rows in one launch (more than one row block per thread column), against the restatement again
    many = list(range(40, 40 + 21))
    got_many = m.counter_normals(batch, ids, SEED ^ 1, many).cpu().numpy().astype(np.float64)
    assert float(np.abs(got_many - R.normals(SEED ^ 1, ids, sizes, many)).max()) < 1e-5
    # a BatchTopology in place of the batch vector (what LangevinRun hands over)
    from agdiff_amd import synth
    b = synth.make_packed_batch("qm9", 3, 2, seed=7)
    topo = BatchTopology(b["atom_type"], b["bond_index"], b["bond_type"], b["batch"], num_graphs=b["num_graphs"], device="cuda:0")
    ids6 = np.arange(6, dtype=np.int64) * 1000003
    assert torch.equal(m.counter_normals(topo, ids6, 11, [3, -1]), m.counter_normals(b["batch"], ids6, 11, [3, -1]))


# ------------------------------------------------------------------------------------------------ 2. statistics
def test_statistics_of_three_million_normals():
    m = _model()
    G, n, S = 200, 50, 128
    batch = np.repeat(np.arange(G), n)
    ids = np.arange(G, dtype=np.int64) * ((1 << 32) + 1)
    z = m.counter_normals(batch, ids, 2021, list(range(S)))
    assert bool(torch.isfinite(z).all())
    cnt = z.numel()
    assert cnt >= 3_000_000
    zd = z.double()
    mean, var, top = float(zd.mean()), float(zd.var(unbiased=False)), float(z.abs().max())
    print("counter normals: n %d  mean %.3e (gate %.3e)  var - 1 %.3e (gate %.3e)  max |z| %.3f"
          % (cnt, mean, 5 / np.sqrt(cnt), var - 1.0, 5 * np.sqrt(2.0 / cnt), top))
    assert abs(mean) < 5 / np.sqrt(cnt)
    assert abs(var - 1.0) < 5 * np.sqrt(2.0 / cnt)
    assert top <= 5.9
    # per component too (x and y share a radius, z is the second pair's cosine branch)
    for c in range(3):
        k = cnt // 3
        assert abs(float(zd[..., c].mean())) < 5 / np.sqrt(k) and abs(float(zd[..., c].var(unbiased=False)) - 1.0) < 5 * np.sqrt(2.0 / k)
    # two stream ids (same step, same atoms), two steps (same id): no run of two consecutive values in common
    zc = z.cpu().numpy()

    def pairs(v):
        v = v.reshape(-1)
        return set(zip(v[:-1].tolist(), v[1:].tolist()))
    a, b, c2 = zc[5, 0:n], zc[5, n:2 * n], zc[6, 0:n]
    assert not (pairs(a) & pairs(b)) and not (pairs(a) & pairs(c2))
    assert not np.any(a == b) and not np.any(a == c2)


# ------------------------------------------------------------------------------------------------ 3. layout invariance
def test_a_conformer_draws_and_samples_the_same_alone_and_packed_after_another_molecule():
    """Molecule X x 4 conformers alone, and the same four conformers (same ids) packed after a molecule Y of another size: the
    noise rows and pos_init of X's atoms are the same bits; X's final positions agree within the mode's parity gate (both
    batches sit below every tune_* crossover, so the same kernel variants run: variant_log equal)."""
    from agdiff_amd import driver
    m = _model()
    y, x = _mols([23, 17], [3, 4], first_index=2)
    alone = driver.pack_batch([x], CONFS)
    both = driver.pack_batch([y, x], CONFS)
    off, n, g = both["spans"][1]
    assert off > 0 and g == 4 and np.array_equal(both["stream_ids"][3:], alone["stream_ids"])
    assert both["atom_type"].shape[0] < 3072                    # under BatchTopology.GROUP_MIN_NODES and every tune_* default
    p0_a, nz_a, pos_a, var_a, _ = _run_counter(m, alone, SEED)
    p0_b, nz_b, pos_b, var_b, _ = _run_counter(m, both, SEED)
    assert var_a == var_b
    assert torch.equal(p0_b[off:off + n * g], p0_a) and torch.equal(nz_b[:, off:off + n * g], nz_a)
    assert nz_a.shape == (8, n * g, 3) and float(nz_a.abs().max()) > 1.0
    _compare_positions("counter: X alone vs packed after Y", pos_b[off:off + n * g], pos_a)
    # the four conformers of X drew different numbers from each other, and Y from X
    assert not torch.equal(nz_a[:, :n], nz_a[:, n:2 * n])
    # another seed: other draws
    assert not torch.equal(_run_counter(m, alone, SEED + 1)[1], nz_a)
    # the step's counter word is the schedule index, not the loop counter: a run over the schedule's last three indices draws rows 5..7
    a = [t(alone[k]).cuda() for k in ("atom_type", "bond_index", "bond_type", "batch")]
    run = m.begin_sampling(a[0], p0_a.cuda(), a[1], a[2], a[3], alone["num_graphs"], False, step_indices=[2, 1, 0],
                           noise_mode="counter", noise_seed=SEED, stream_ids=alone["stream_ids"])
    run.advance(3)
    assert run.steps == [2, 1, 0] and torch.equal(run._nz.cpu(), nz_a[5:8])
    # an explicit noise= tensor still wins
    given = torch.zeros(8, n * g, 3)
    r2 = m.begin_sampling(a[0], p0_a.cuda(), a[1], a[2], a[3], alone["num_graphs"], False, n_steps=8, noise=given.cuda(),
                          noise_mode="counter", noise_seed=SEED, stream_ids=alone["stream_ids"])
    r2.advance(8)
    assert r2._nz is None


# ------------------------------------------------------------------------------------------------ 4. sharding invariance
def test_a_batch_cut_into_two_graph_ranges_draws_and_samples_what_the_whole_batch_does():
    from agdiff_amd import driver
    from agdiff_amd.dist import shard_of
    m = _model()
    packed = driver.pack_batch(_mols([12, 19, 15], [2, 3, 2], first_index=40, seed=8), CONFS)
    p0, nz, pos, var, _ = _run_counter(m, packed, 77)
    halves = [shard_of(packed, r, 2) for r in range(2)]
    assert all(h[0] is not None for h in halves) and halves[0][1][1] == halves[1][1][0]
    got_p0, got_nz, got_pos = [], [], []
    for part, (g0, g1), (lo, hi) in halves:
        assert np.array_equal(part["stream_ids"], packed["stream_ids"][g0:g1])
        a, b, c, v, _ = _run_counter(m, part, 77)
        assert v == var
        got_p0.append(a); got_nz.append(b); got_pos.append(c)
    assert torch.equal(torch.cat(got_p0), p0) and torch.equal(torch.cat(got_nz, dim=1), nz)
    _compare_positions("counter: two graph halves vs the whole batch", torch.cat(got_pos), pos)


def test_sample_batch_sharded_world1_draws_what_sample_batch_draws():
    import torch.distributed as dist
    from agdiff_amd import driver
    from agdiff_amd.dist import sample_batch_sharded
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        m = _model()
        packed = driver.pack_batch(_mols([12, 19, 15], [2, 3, 2], first_index=40, seed=8), CONFS)
        kw = dict(n_steps=8, step_lr=1e-6, w_global=1.0, clip=1000.0)
        a, _, oka = driver.sample_batch(m, packed, dev, kw, counter_seed=77)
        b, _, okb = sample_batch_sharded(m, packed, dev, kw, counter_seed=77)
        assert oka.all() and okb.all()
        _compare_positions("counter: sample_batch_sharded (world 1) vs sample_batch", b, a)
        # ... and both what the module API gives with the batch's ids
        _, _, pos, _, _ = _run_counter(m, packed, 77)
        _compare_positions("counter: sample_batch vs begin_sampling", a, pos)
        # the default mode is still there, and draws something else
        c, _, okc = driver.sample_batch(m, packed, dev, kw)
        assert okc.all() and not torch.equal(c, a)
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ 5. driver
def test_run_job_gives_the_same_conformers_at_two_max_atoms_and_after_a_resume(tmp_path):
    import glob
    from agdiff_amd import driver
    m = _model()
    mols = _mols([14, 22, 9, 18, 16], [3, 2, 4, 2, 3], first_index=0, seed=12)
    kw = dict(n_steps=8, step_lr=1e-6, w_global=1.0, clip=1000.0)
    need = [len(x["atom_type"]) * CONFS(x["num_refs"]) for x in mols]
    big, small = sum(need), max(need)
    plans = [[tuple(x["index"] for x in bm) for bm in driver.plan_batches(mols, CONFS, cap)] for cap in (big, small)]
    assert len(plans[0]) == 1 and len(plans[1]) >= 3 and plans[0] != plans[1]
    quiet = lambda *_: None
    one = driver.run_job(m, mols, str(tmp_path / "one"), CONFS, big, kw, "cuda:0", log=quiet, noise="counter", seed=5)
    many = driver.run_job(m, mols, str(tmp_path / "many"), CONFS, small, kw, "cuda:0", log=quiet, noise="counter", seed=5)
    bitwise = []
    for x in mols:
        k = "pos_gen_%d" % x["index"]
        assert one[k].shape == (CONFS(x["num_refs"]), len(x["atom_type"]), 3) and np.isfinite(one[k]).all()
        bitwise.append(_compare_positions("run_job counter %s: max_atoms %d vs %d" % (k, small, big), torch.from_numpy(many[k]), torch.from_numpy(one[k])))
    print("run_job counter: molecules bitwise equal across the two plans: %d of %d" % (sum(bitwise), len(bitwise)))
    # another seed names other conformers; the default mode is untouched by the new arguments
    other = driver.run_job(m, mols, str(tmp_path / "other"), CONFS, big, kw, "cuda:0", log=quiet, noise="counter", seed=6)
    assert not np.array_equal(other["pos_gen_0"], one["pos_gen_0"])
    # resume: one batch file of the second run is lost; the resumed run plans over what is missing and restores it
    files = sorted(glob.glob(str(tmp_path / "many" / "samples_[0-9]*.npz")))
    assert len(files) == len(plans[1])
    lost = [k for k in np.load(files[1]).files if k.startswith("pos_gen_")]
    os.remove(files[1])
    os.remove(str(tmp_path / "many" / "samples_all.npz"))
    again = driver.run_job(m, mols, str(tmp_path / "many"), CONFS, big, kw, "cuda:0", log=quiet, noise="counter", seed=5, resume=True)
    assert lost and sorted(k for k in again if k.startswith("pos_gen_")) == sorted(k for k in one if k.startswith("pos_gen_"))
    for x in mols:
        k = "pos_gen_%d" % x["index"]
        _compare_positions("run_job counter %s: resumed vs one batch" % k, torch.from_numpy(again[k]), torch.from_numpy(one[k]))
        if k not in lost:
            assert np.array_equal(again[k], many[k])


def test_a_retry_changes_that_molecules_draws_and_nobody_elses_result():
    """One molecule's pos_init holds a NaN: its conformers are sampled again with clip_local=20 and attempt + 1 in their stream
    ids -- fresh draws, the ones a direct run with those ids makes --, while the molecules packed with it keep their result bit
    for bit (same batch, same draws)."""
    from agdiff_amd import driver
    m = _model()
    mols = _mols([14, 22, 9], [2, 2, 3], first_index=3, seed=13)
    packed = driver.pack_batch(mols, CONFS)
    kw = dict(n_steps=8, step_lr=1e-6, w_global=1.0, clip=1000.0)
    clean, _, ok0 = driver.sample_batch(m, packed, "cuda:0", kw, counter_seed=9)
    assert ok0.all()
    p0 = m.counter_normals(packed["batch"], packed["stream_ids"], 9, [-1])[0].cpu()
    same, _, _ = driver.sample_batch(m, packed, "cuda:0", kw, counter_seed=9, pos_init=p0)
    assert torch.equal(same, clean)                         # (the injected pos_init is the one the mode draws)
    off, n, g = packed["spans"][1]
    bad = p0.clone()
    bad[off + n + 2, 0] = float("nan")
    logs = []
    pos, _, ok = driver.sample_batch(m, packed, "cuda:0", kw, counter_seed=9, pos_init=bad, log=logs.append)
    assert ok.all() and bool(torch.isfinite(pos).all()) and len(logs) == 1 and "1 of 3" in logs[0]
    keep = torch.ones(packed["atom_type"].shape[0], dtype=torch.bool)
    keep[off:off + n * g] = False
    assert torch.equal(pos[keep], clean[keep])
    assert not torch.equal(pos[~keep], clean[~keep])
    # the retried molecule = a run of it alone with attempt 1 in its ids and local clipping
    sub = driver.subset_batch(packed, [1])
    sub["stream_ids"] = driver.with_attempt(sub["stream_ids"], 1)
    assert driver.split_stream_id(sub["stream_ids"])[2].tolist() == [1] * g
    _, nz1, direct, _, _ = _run_counter(m, sub, 9, clip_local=20)
    _compare_positions("counter: retried molecule vs a direct attempt-1 run", pos[~keep], direct)
    sub0 = driver.subset_batch(packed, [1])
    assert not torch.equal(_run_counter(m, sub0, 9)[1], nz1)         # attempt 0 and attempt 1: different noise rows


# ------------------------------------------------------------------------------------------------ 6. arguments
def test_counter_mode_without_ids_or_seed_is_refused():
    from agdiff_amd import driver
    m = _model()
    packed = driver.pack_batch(_mols([10, 12], [1, 2]), CONFS)
    a = [t(packed[k]).cuda() for k in ("atom_type", "bond_index", "bond_type", "batch")]
    p0 = torch.zeros(a[0].shape[0], 3).cuda()
    ids = packed["stream_ids"]
    base = dict(n_steps=2, noise_mode="counter")
    for extra in ({}, {"noise_seed": 1}, {"stream_ids": ids}, {"noise_seed": 1, "stream_ids": ids[:-1]},
                  {"noise_seed": 1, "stream_ids": -ids - 1}, {"noise_seed": 1, "stream_ids": ids.astype(np.int32)}):
        with pytest.raises(ValueError):
            m.begin_sampling(a[0], p0, a[1], a[2], a[3], packed["num_graphs"], False, **base, **extra)
    with pytest.raises(ValueError):
        m.langevin_dynamics_sample_diffusion(a[0], p0, a[1], a[2], a[3], packed["num_graphs"], False, **base)
    with pytest.raises(ValueError):
        m.begin_sampling(a[0], p0, a[1], a[2], a[3], packed["num_graphs"], False, n_steps=2, noise_mode="philox")
    with pytest.raises(ValueError):
        m.counter_normals(packed["batch"], ids, 1, [-2])
    with pytest.raises(ValueError):
        m.counter_normals(packed["batch"][::-1].copy(), ids, 1, [0])
    with pytest.raises(ValueError):
        m.counter_normals(packed["batch"], ids[:-1], 1, [0])
    # step graphs stay with the chunked mode: a counter run on a model that asks for them launches step by step
    m.step_graphs = True
    start = m.counter_normals(packed["batch"], ids, 1, [-1])[0]
    run = m.begin_sampling(a[0], start, a[1], a[2], a[3], packed["num_graphs"], False, n_steps=4, noise_mode="counter", noise_seed=1,
                           stream_ids=ids)
    run.advance(4)
    run.finish()
    assert run.graph_steps == 0 and not run._use_graphs
