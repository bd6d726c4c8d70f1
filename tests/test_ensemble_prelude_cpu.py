"""No GPU: what prune_conformers, cluster_conformers and pick_conformers launch, in which order and with which arguments, and how
their results map back to the item's own conformer indices -- with _lib.call replaced by a recorder that fills every output with
the simplest answer its entry point can give (the leader walk keeps everything, Butina makes singletons, MaxMin picks in index
order from its start, the superposition copies its input, every matrix is zero) and everything on device="cpu".

The item: pentane's heavy atoms, five atoms and four bonds (two rotatable bonds, so the TFD path launches its dihedrals), four
conformers.  medoid_conformers checks `init.is_cuda` itself and stays with the GPU tests."""
import numpy as np
import pytest
import torch

from agdiff_amd import _lib

G, N = 4, 5
PARTIAL = np.array([True, False, True, True])
METRICS = ("rmsd", "tfd")
MASKS = (None, PARTIAL, np.zeros(G, dtype=bool))
# per metric: the entry points before the walk, the matrix entry point, and where its G, threshold, out and bits stand
MATRIX = {"rmsd": ([], "agdiff_rmsd_self", 3, 7, 9, 10), "tfd": (["agdiff_torsion_angles"], "agdiff_tfd_matrix", 5, 9, 10, 12)}


def _fill(name, a):
    if name == "agdiff_rmsd_self":
        outs = (a[9], a[10])
    elif name == "agdiff_tfd_matrix":
        outs = (a[10], a[11], a[12])
    elif name == "agdiff_torsion_angles":
        outs = (a[5],)
    elif name == "agdiff_leader_prune":              # (bits, G, keep, leader, count, n_kept): every conformer is kept
        a[2].fill_(1), a[3].copy_(torch.arange(a[1])), a[4].fill_(1), a[5].fill_(a[1])
        return
    elif name == "agdiff_butina_cluster":            # (bits, G, reorder, leader, count, rank, n_clusters): singletons
        a[3].copy_(torch.arange(a[1])), a[4].fill_(1), a[5].copy_(torch.arange(a[1])), a[6].fill_(a[1])
        return
    elif name == "agdiff_maxmin_pick":               # (dist, G, k, first, stop, picks, radius, owner, near, n_picked, cover)
        g, k, first = a[1], a[2], a[3]
        order = [first] + [i for i in range(g) if i != first]
        a[5].copy_(torch.tensor(order[:k])), a[6].fill_(0.0), a[8].fill_(0.0), a[9].fill_(k), a[10].fill_(0.0)
        a[7].copy_(torch.tensor([order.index(i) if order.index(i) < k else 0 for i in range(g)]))
        return
    elif name == "agdiff_align_conformers":          # (pos, idx, target, G, n, m, out, rmsd): the identity
        a[6].copy_(a[0]), a[7].fill_(0.0)
        return
    else:
        raise AssertionError("an entry point this test does not know: %s" % name)
    for t in outs:
        if t is not None:
            t.zero_()


@pytest.fixture
def trace(monkeypatch):
    calls = []

    def call(name, *args):
        calls.append((name, args))
        _fill(name, args)
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(_lib, "require_device_conformers", lambda pos: None)
    monkeypatch.setattr(_lib, "require_device_table", lambda t, what: None)
    return calls


def _item():
    rng = np.random.default_rng(3)
    pos = torch.from_numpy(rng.normal(size=(G, N, 3)).astype(np.float32))
    bonds = np.array([[0, 1, 2, 3], [1, 2, 3, 4]])
    return {"atom_type": np.array([6, 6, 6, 6, 6]), "bond_index": bonds, "bond_type": np.ones(4, dtype=np.int64), "pos_gen": pos}


def _check_matrix_call(calls, metric, usable, threshold, out_null, bits_null):
    before, name, g, thr, out, bits = MATRIX[metric]
    k = len(before)
    assert [c[0] for c in calls[:k + 1]] == before + [name]
    args = calls[k][1]
    assert args[g] == usable and args[thr] == threshold
    assert (args[out] is None) == out_null and (args[bits] is None) == bits_null
    if metric == "tfd":
        assert args[4] == usable and args[11] is None                     # R = G, and no mirror matrix
        assert tuple(calls[0][1][0].shape) == (usable, N, 3)              # the dihedrals of the usable conformers only
    else:
        assert tuple(args[0].shape) == (usable, N, 3)
    return k + 1


def _own(mask):
    """the usable conformers' indices in the item's own numbering"""
    return np.arange(G) if mask is None else np.nonzero(mask)[0]


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("mask", MASKS, ids=["all", "partial", "none"])
@pytest.mark.parametrize("metric", METRICS)
def test_prune_conformers_launches(trace, metric, mask, align):
    from agdiff_amd.ensemble import prune_conformers
    item = _item()
    before = item["pos_gen"].clone()
    res = prune_conformers(item, 0.25, align=align, device="cpu", metric=metric, valid=mask)
    assert torch.equal(item["pos_gen"], before)
    own = _own(mask)
    if own.size == 0:
        assert trace == []
        assert res["kept"].shape == (0,) and res["count"].shape == (0,) and res["pos"].shape == (0, N, 3)
        assert res["leader"].tolist() == [-1] * G and res["leader"].dtype == torch.int32
        return
    k = _check_matrix_call(trace, metric, own.size, 0.25, out_null=True, bits_null=False)
    assert [c[0] for c in trace[k:]] == ["agdiff_leader_prune"] + (["agdiff_align_conformers"] if align else [])
    assert trace[k][1][1] == own.size
    if align:
        assert trace[k + 1][1][3] == own.size and trace[k + 1][1][5] == N
    want = np.full(G, -1)
    want[own] = own
    assert res["kept"].tolist() == own.tolist() and res["leader"].tolist() == want.tolist() and res["count"].tolist() == [1] * own.size
    assert all(res[key].dtype == torch.int32 for key in ("kept", "leader", "count"))
    assert torch.equal(res["pos"], before[own])
    assert set(res) == {"kept", "leader", "count", "pos"}


@pytest.mark.parametrize("distances", [False, True])
@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("mask", MASKS, ids=["all", "partial", "none"])
@pytest.mark.parametrize("metric", METRICS)
def test_cluster_conformers_launches(trace, metric, mask, align, distances):
    from agdiff_amd.clusters import cluster_conformers
    item = _item()
    before = item["pos_gen"].clone()
    res = cluster_conformers(item, 0.25, metric=metric, align=align, device="cpu", valid=mask, distances=distances)
    assert torch.equal(item["pos_gen"], before)
    assert set(res) == {"centroids", "leader", "cluster", "count", "population", "pos"} | ({"dist"} if distances else set())
    own = _own(mask)
    if own.size == 0:
        assert trace == []
        assert all(res[key].shape == (0,) for key in ("centroids", "count", "population")) and res["pos"].shape == (0, N, 3)
        assert res["leader"].tolist() == [-1] * G and res["cluster"].tolist() == [-1] * G
        assert not distances or (res["dist"].shape == (G,) and bool(torch.isnan(res["dist"]).all()))
        return
    k = _check_matrix_call(trace, metric, own.size, 0.25, out_null=not distances, bits_null=False)
    assert [c[0] for c in trace[k:]] == ["agdiff_butina_cluster"] + (["agdiff_align_conformers"] if align else [])
    assert trace[k][1][1] == own.size and trace[k][1][2] == 1
    lead, clus = np.full(G, -1), np.full(G, -1)
    lead[own], clus[own] = own, np.arange(own.size)
    assert res["centroids"].tolist() == own.tolist() and res["leader"].tolist() == lead.tolist() and res["cluster"].tolist() == clus.tolist()
    assert res["count"].tolist() == [1] * own.size and res["population"].tolist() == [float(np.float32(1) / np.float32(own.size))] * own.size
    assert all(res[key].dtype == torch.int32 for key in ("centroids", "leader", "cluster", "count"))
    assert torch.equal(res["pos"], before[own])
    if distances:
        usable = np.zeros(G, dtype=bool)
        usable[own] = True
        assert res["dist"].dtype == torch.float32 and np.array_equal(torch.isnan(res["dist"]).numpy(), ~usable)
        assert (res["dist"][torch.from_numpy(usable)] == 0).all()


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("mask", MASKS, ids=["all", "partial", "none"])
@pytest.mark.parametrize("metric", METRICS)
def test_pick_conformers_launches(trace, metric, mask, align):
    from agdiff_amd.picks import pick_conformers
    item = _item()
    before = item["pos_gen"].clone()
    first = 2 if mask is PARTIAL else None
    res = pick_conformers(item, k=2, metric=metric, first=first, align=align, device="cpu", valid=mask)
    assert torch.equal(item["pos_gen"], before)
    assert set(res) == {"picks", "radius", "owner", "near", "count", "cover", "pos"}
    own = _own(mask)
    if own.size == 0:
        assert trace == []
        assert all(res[key].shape == (0,) for key in ("picks", "radius", "count")) and res["pos"].shape == (0, N, 3)
        assert res["owner"].tolist() == [-1] * G and bool(torch.isnan(res["near"]).all()) and res["cover"] == 0.0
        return
    k = _check_matrix_call(trace, metric, own.size, 0.0, out_null=False, bits_null=True)     # the float matrix, no threshold
    assert [c[0] for c in trace[k:]] == ["agdiff_maxmin_pick"] + (["agdiff_align_conformers"] if align else [])
    start = 0 if first is None else 1                                     # conformer 2 is the second usable one
    assert trace[k][1][1:5] == (own.size, 2, start, -1.0)
    order = [start] + [i for i in range(own.size) if i != start]
    owner = np.full(G, -1)
    owner[own] = [order.index(i) if order.index(i) < 2 else 0 for i in range(own.size)]
    assert res["picks"].tolist() == own[order[:2]].tolist() and res["owner"].tolist() == owner.tolist()
    assert res["picks"].dtype == torch.int32 and res["owner"].dtype == torch.int32
    assert res["count"].tolist() == np.bincount(owner[own], minlength=2).tolist()
    assert np.array_equal(torch.isnan(res["near"]).numpy(), owner < 0)
    assert torch.equal(res["pos"], before[own[order[:2]]])


def test_fixes_leave_the_callers_tensor_alone_and_reach_every_result(trace, monkeypatch):
    """the handedness fix writes its tensor in place: it must be a copy, on every path, the all-masked one included"""
    from agdiff_amd import clusters, ensemble, picks

    def fix(item, gen):
        gen.neg_()
        return torch.full((gen.shape[0],), -1, dtype=torch.int32)
    for module in (ensemble, clusters):              # (wherever a module binds the fix under this name)
        if hasattr(module, "_fix_handedness"):
            monkeypatch.setattr(module, "_fix_handedness", fix)
    for mask in MASKS:
        own = _own(mask)
        for run in (lambda it: ensemble.prune_conformers(it, 0.25, device="cpu", valid=mask, fix_handedness=True),
                    lambda it: clusters.cluster_conformers(it, 0.25, device="cpu", valid=mask, fix_handedness=True),
                    lambda it: picks.pick_conformers(it, k=G, device="cpu", valid=mask, fix_handedness=True)):
            item = _item()
            before = item["pos_gen"].clone()
            res = run(item)
            assert torch.equal(item["pos_gen"], before)
            assert res["hand"].tolist() == [-1] * G and "ez_state" not in res
            assert torch.equal(res["pos"], -before[own])
