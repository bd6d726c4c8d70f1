"""CPU: host logic of the torsion restraints (agdiff_amd/torsion_restraints.py, epsnet.LangevinRun's torsion_* keywords): the
export and its declaration, the side rules, the refusals of the keyword checks, the test set's `tors_*_<i>` fields, packing, the
scan grid and the command line's defaults.  Nothing here computes on a GPU."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from agdiff_amd import _lib, driver, epsnet, restraints, synth
from agdiff_amd import torsion_restraints as TR

PI = np.pi


def test_export_argtypes_and_header():
    lib = _lib.load()
    assert hasattr(lib, "agdiff_restrain_torsions")
    P, I, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    want = [P] * 10 + [I, I, I, I, F, I, P, P, P, P]
    assert _lib.EXPORTS["agdiff_restrain_torsions"] == want
    assert list(lib.agdiff_restrain_torsions.argtypes) == want and lib.agdiff_restrain_torsions.restype is ctypes.c_int
    src = open(_lib.HEADER).read()
    assert "int agdiff_restrain_torsions(float* pos /* [N][3], in place */, const int32_t* graph_ptr /* [G + 1] */" in src
    assert "e = Delta - sign(Delta) half" in src and "theta' = theta - w e" in src          # the rule is stated in the header
    # a pure addition: the ABI version and the neighbours are what they were
    assert lib.agdiff_abi_version() == _lib.DEFINES["AGDIFF_ABI_VERSION"] == 48
    assert len(_lib.EXPORTS["agdiff_restrain_pairs"]) == 17 and ctypes.sizeof(_lib.StepArgs) == 72


def test_argument_errors_of_the_entry_point_need_no_gpu():
    lib = _lib.load()
    bufs = [(ctypes.c_float * 64)() for _ in range(10)]
    p, gp, tp, q, ce, ha, sr, sp, si, vi = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
    null = ctypes.c_void_p(0)

    def call(pos=p, graph_ptr=gp, tr_ptr=tp, quads=q, centre=ce, half=ha, side_row=sr, side_ptr=sp, G=1, N=4, T=1, S=1, w=1.0, copy_out=null,
             viol=vi):
        return lib.agdiff_restrain_torsions(pos, graph_ptr, tr_ptr, quads, centre, half, side_row, side_ptr, si, null, G, N, T, S, w, 1,
                                            copy_out, null, viol, null)

    for bad in (dict(pos=null), dict(graph_ptr=null), dict(tr_ptr=null), dict(quads=null), dict(centre=null), dict(half=null),
                dict(side_row=null), dict(side_ptr=null), dict(viol=null), dict(G=-1), dict(N=0), dict(T=-1), dict(S=-1), dict(copy_out=p)):
        assert call(**bad) == -1, bad
    for w in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert call(w=w) == -1, w
    assert call(G=0) == 0 and call(G=0, T=0, S=0, quads=null, centre=null, half=null, side_row=null, side_ptr=null) == 0


# a molecule for the side rules:   0 - 1 - 2 - 3 - 4 - 5   with 6 on 1, 7 and 8 on 4, and the ring 9 - 10 - 11 on 5
def _chain():
    bonds = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (1, 6), (4, 7), (4, 8), (5, 9), (9, 10), (10, 11), (11, 5)]
    bi = np.array(bonds + [(b, a) for a, b in bonds]).T
    return 12, bi, np.ones(bi.shape[1], dtype=np.int64)


def test_torsion_sides_rules():
    n, bi, bt = _chain()
    q, sp, si = TR.torsion_sides(n, bi, bt, [[1, 2, 3, 4], [2, 3, 4, 5]])
    # bond 2 - 3: u's side {0, 1, 2, 6} (4 atoms) is smaller than v's (8 atoms): the quad comes back reversed, its row is u's side
    # bond 3 - 4: (0, 1, 2, 3, 6) against (4, 5, 7 .. 11): 5 < 7, reversed as well
    assert q.dtype == np.int32 and q.tolist() == [[4, 3, 2, 1], [5, 4, 3, 2]] and sp.dtype == si.dtype == np.int32
    assert sp.tolist() == [0, 4, 9] and si.tolist() == [0, 1, 2, 6, 0, 1, 2, 3, 6]
    # the larger side is u's: the quad stays, the row is v's side with v itself in it
    q, sp, si = TR.torsion_sides(n, bi, bt, [[5, 4, 3, 2]])
    assert q.tolist() == [[5, 4, 3, 2]] and si.tolist() == [0, 1, 2, 3, 6]
    # a tie goes to v
    bonds = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    b6 = np.array(bonds + [(b, a) for a, b in bonds]).T
    q, sp, si = TR.torsion_sides(6, b6, np.ones(10), [[1, 2, 3, 4]])
    assert q.tolist() == [[1, 2, 3, 4]] and si.tolist() == [3, 4, 5]
    # frozen: the side without a frozen atom, whatever its size; both sides frozen: an empty row, the quad as given
    fz = np.zeros(n, dtype=bool)
    fz[0] = True
    q, sp, si = TR.torsion_sides(n, bi, bt, [[1, 2, 3, 4]], frozen=fz)
    assert q.tolist() == [[1, 2, 3, 4]] and si.tolist() == [3, 4, 5, 7, 8, 9, 10, 11]
    fz[10] = True
    q, sp, si = TR.torsion_sides(n, bi, bt, [[1, 2, 3, 4]], frozen=fz)
    assert q.tolist() == [[1, 2, 3, 4]] and sp.tolist() == [0, 0] and si.size == 0
    fz[0] = False
    q, sp, si = TR.torsion_sides(n, bi, bt, [[1, 2, 3, 4]], frozen=fz)
    assert q.tolist() == [[4, 3, 2, 1]] and si.tolist() == [0, 1, 2, 6]
    empty = TR.torsion_sides(n, bi, bt, np.zeros((0, 4), dtype=np.int32))
    assert empty[0].shape == (0, 4) and empty[1].tolist() == [0]


def test_torsion_sides_value_errors():
    n, bi, bt = _chain()
    for bad in ([[1, 2, 4, 5]],                   # 2 - 4 is no bond
                [[0, 2, 3, 4]], [[1, 2, 3, 5]],   # a not bonded to u, b not bonded to v
                [[3, 2, 3, 4]], [[1, 2, 3, 2]],   # a == v, b == u
                [[4, 5, 9, 10]],                  # a ring bond
                [[1, 2, 3, 4], [4, 3, 2, 1]],     # two restraints on one bond
                [[1, 2, 3, 12]], [[-1, 2, 3, 4]], [[1, 2, 3]]):
        with pytest.raises(ValueError):
            TR.torsion_sides(n, bi, bt, bad)
    with pytest.raises(ValueError):
        TR.torsion_sides(n, bi, bt, [[1, 2, 3, 4]], frozen=np.zeros(5))


def _batch3():
    """Three conformers of the chain molecule."""
    n, bi, bt = _chain()
    at, r, c, t, b = synth.repeat_molecule(np.full(n, 6), bi[0], bi[1], bt, 3)
    return 3 * n, np.stack([r, c]), t, b


def test_restraint_arguments_value_errors():
    N, bi, bt, batch = _batch3()
    ok = dict(quads=[[1, 2, 3, 4], [13, 14, 15, 16]], target=[1.0, -2.0], tol=[0.1, 0.0])
    ra = lambda **kw: TR.restraint_arguments(N, *(kw.pop(k, ok[k]) for k in ("quads", "target", "tol")), kw.pop("batch", batch), **kw)
    bad = [dict(target=[1.0]), dict(tol=[0.1]), dict(target=None), dict(tol=None),
           dict(quads=[[1, 2, 3]], target=[1.0], tol=[0.1]), dict(quads=[1, 2, 3, 4, 5], target=[1.0], tol=[0.1]),     # not [T, 4]
           dict(quads=[[1.0, 2.0, 3.0, 4.5]], target=[1.0], tol=[0.1]),                                                  # not indices
           dict(target=[1.0, np.nan]), dict(tol=[np.nan, 0.0]), dict(target=[3.2, 0.0]), dict(target=[0.0, -3.2]),
           dict(tol=[-0.1, 0.0]), dict(tol=[0.1, 3.2]), dict(tol=[0.1, np.inf]),
           dict(quads=[[1, 2, 3, 4], [13, 14, 15, 36]]), dict(quads=[[1, 2, 3, 4], [-1, 14, 15, 16]]),
           dict(quads=[[1, 2, 3, 4], [11, 12, 13, 14]]),                                                               # across two graphs
           dict(quads=[[13, 14, 15, 16], [1, 2, 3, 4]]),                                                               # not graph by graph
           dict(batch=None), dict(batch=batch[:-1]),
           dict(weight=0.0), dict(weight=1.0001), dict(weight=-1.0), dict(weight=float("nan")), dict(start_sigma=float("nan")),
           dict(sides=([0, 1], [0, 2])), dict(sides=([0], [0, 2, 4], [2, 3, 2, 3])), dict(sides=([0, 2], [0, 2, 4], [2, 3, 2, 3])),
           dict(sides=([0, 1], [0, 2, 5], [2, 3, 2, 3])), dict(sides=([0, 1], [0, 2, 4], [2, 3, -2, 3])),
           dict(bond_index=bi, bond_type=bt, quads=[[4, 5, 9, 10]], target=[0.0], tol=[0.1])]                        # a ring bond
    for kw in bad:
        with pytest.raises(ValueError):
            ra(**dict(kw))
    with pytest.raises(ValueError):
        TR.restraint_arguments(N, None, [1.0], [0.1], batch)               # targets without quads
    assert TR.restraint_arguments(N, None, None, None, batch) is None
    assert TR.restraint_arguments(N, np.zeros((0, 4), dtype=np.int64), [], [], batch) is None
    assert TR.restraint_arguments(N, [], [], [], None) is None
    # fp32's pi is a legal target and tolerance
    assert ra(target=np.array([np.pi, -np.pi], dtype=np.float32), tol=np.array([np.pi, 0.0], dtype=np.float32)) is not None
    tr_ptr, q, tg, tl, table, w, start = ra(weight=0.25, start_sigma=0.7)
    assert tr_ptr.dtype == np.int32 and tr_ptr.tolist() == [0, 1, 2, 2] and q.dtype == np.int32 and tg.dtype == tl.dtype == np.float32
    assert table is None and (w, start) == (0.25, 0.7)                     # checked, no bonds: no sides
    # with the bonds: one row of the table for the two conformers (one topology, one local quad), the quads reversed
    tr_ptr, q, tg, tl, (row, sp, si), w, start = ra(quads=[[1, 2, 3, 4], [13, 14, 15, 16], [25, 26, 27, 28]], target=[0.0] * 3, tol=[0.1] * 3,
                                                    bond_index=bi, bond_type=bt)
    assert q.tolist() == [[4, 3, 2, 1], [16, 15, 14, 13], [28, 27, 26, 25]] and row.tolist() == [0, 0, 0]
    assert sp.tolist() == [0, 4] and si.tolist() == [0, 1, 2, 6]
    # a frozen atom in one conformer only: that graph is another topology
    fz = np.zeros(N, dtype=bool)
    fz[12] = True
    _, q, _, _, (row, sp, si), _, _ = ra(quads=[[1, 2, 3, 4], [13, 14, 15, 16]], bond_index=bi, bond_type=bt, frozen=fz)
    assert q.tolist() == [[4, 3, 2, 1], [13, 14, 15, 16]] and row.tolist() == [0, 1] and sp.tolist() == [0, 4, 12]
    # torsion_sides runs once per distinct topology, not per conformer
    calls, real = [], TR.torsion_sides
    TR.torsion_sides = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        ra(quads=[[1, 2, 3, 4], [13, 14, 15, 16], [25, 26, 27, 28]], target=[0.0] * 3, tol=[0.1] * 3, bond_index=bi, bond_type=bt)
    finally:
        TR.torsion_sides = real
    assert len(calls) == 1


def test_the_six_keywords_are_real_parameters():
    params = inspect.signature(epsnet.LangevinRun.__init__).parameters
    for name, default in (("torsion_quads", None), ("torsion_target", None), ("torsion_tol", None), ("torsion_sides", None),
                          ("torsion_weight", 1.0), ("torsion_start_sigma", float("inf"))):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default
    assert TR.SAMPLER_KEYWORDS == ("torsion_quads", "torsion_target", "torsion_tol", "torsion_sides", "torsion_weight", "torsion_start_sigma")
    assert restraints.SAMPLER_KEYWORDS == ("restraint_pairs", "restraint_lo", "restraint_hi", "restraint_weight", "restraint_start_sigma",
                                           "restraint_sweeps")


class _NoGpu:
    """A model on which touching the device is an error: the keyword checks come first."""

    def _device(self):
        raise AssertionError("the run reached the device")

    def _require_gpu(self):
        raise AssertionError("the run reached the device")


def test_sampler_keyword_checks():
    N, bi, bt, batch = _batch3()
    at, batch_t = torch.full((N,), 6), torch.from_numpy(batch)
    quads, target, tol = [[1, 2, 3, 4], [13, 14, 15, 16]], [1.0, -2.0], [0.1, 0.0]
    good = dict(torsion_quads=quads, torsion_target=target, torsion_tol=tol)
    bad = [dict(torsion_quads=quads), dict(torsion_quads=quads, torsion_target=target), dict(torsion_target=target, torsion_tol=tol),
           dict(good, torsion_target=[1.0]), dict(good, torsion_target=[4.0, 0.0]), dict(good, torsion_tol=[-1.0, 0.0]),
           dict(good, torsion_tol=[0.1, float("nan")]), dict(good, torsion_quads=[[1, 2, 3, 4], [13, 14, 15, 36]]),
           dict(good, torsion_quads=[[1, 2, 3, 4], [11, 14, 15, 16]]), dict(good, torsion_weight=0.0), dict(good, torsion_weight=1.5),
           dict(good, torsion_weight=float("nan")), dict(good, torsion_start_sigma=float("nan")), dict(torsion_weight=2.0),
           dict(good, torsion_sides=([0], [0, 2], [2, 3])), dict(torsion_sides=([0], [0, 2], [2, 3]))]
    for kw in bad:
        with pytest.raises(ValueError):
            epsnet.LangevinRun(_NoGpu(), at, None, None, None, batch_t, 3, False, 2, 1e-6, 1000.0, None, None, 0.5, 1.0, **kw)
        with pytest.raises(ValueError):
            epsnet.DualEncoderEpsNetwork.begin_sampling(_NoGpu(), at, None, None, None, batch_t, 3, False, **kw)
    # what needs the bonds is refused before the device as well: a ring bond, two restraints on one bond
    for kw in (dict(torsion_quads=[[4, 5, 9, 10]], torsion_target=[0.0], torsion_tol=[0.1]),
               dict(torsion_quads=[[1, 2, 3, 4], [4, 3, 2, 1]], torsion_target=[0.0, 0.0], torsion_tol=[0.1, 0.1])):
        with pytest.raises(ValueError):
            epsnet.DualEncoderEpsNetwork.begin_sampling(_NoGpu(), at, None, torch.from_numpy(bi), torch.from_numpy(bt), batch_t, 3, False, **kw)
        with pytest.raises(ValueError):
            epsnet.LangevinRun(_NoGpu(), at, None, torch.from_numpy(bi), torch.from_numpy(bt), batch_t, 3, False, 2, 1e-6, 1000.0, None, None,
                               0.5, 1.0, **kw)
    with pytest.raises(ValueError, match="bonds"):                        # neither bonds nor sides: nothing says what turns
        epsnet.LangevinRun(_NoGpu(), at, None, None, None, batch_t, 3, False, 2, 1e-6, 1000.0, None, None, 0.5, 1.0, **good)
    with pytest.raises(AssertionError, match="reached the device"):      # good keywords pass the checks and go on
        epsnet.DualEncoderEpsNetwork.begin_sampling(_NoGpu(), at, None, torch.from_numpy(bi), torch.from_numpy(bt), batch_t, 3, False, **good)
    with pytest.raises(AssertionError, match="reached the device"):
        epsnet.LangevinRun(_NoGpu(), at, None, torch.from_numpy(bi), torch.from_numpy(bt), batch_t, 3, False, 2, 1e-6, 1000.0, None, None, 0.5,
                           1.0, **good)


def _mols(k=3):
    rng = np.random.default_rng(11)
    out = []
    for i in range(k):
        n = int(rng.integers(6, 14))
        at, r, c, t = synth.random_molecule(rng, n)
        out.append(dict(atom_type=at, edge_index=np.stack([r, c]), edge_type=t, num_refs=1 + i, name="m%d" % i, index=i))
    return out


def usable_bridges(mol):
    """Quads (a, u, v, b) over the molecule's bridges with a neighbour on both ends, lowest-index neighbours, sorted by (u, v)."""
    from agdiff_amd.molecule import bonded_neighbours, bridges
    n = mol["atom_type"].shape[0]
    nbrs = [sorted(a) for a in bonded_neighbours(n, mol["edge_index"], mol["edge_type"])]
    out = []
    for u, v in sorted(bridges(nbrs)):
        a, b = [k for k in nbrs[u] if k != v], [k for k in nbrs[v] if k != u]
        if a and b:
            out.append((a[0], u, v, b[0]))
    return out


def test_round_trip_through_the_testset(tmp_path):
    mols = _mols()
    plain, with_t = str(tmp_path / "t.npz"), str(tmp_path / "r.npz")
    driver.save_testset(plain, mols)
    q0, q2 = usable_bridges(mols[0]), usable_bridges(mols[2])
    assert len(q0) >= 2 and len(q2) >= 1
    for m in mols:                                                         # the module lists the same bonds
        assert TR.bridge_quads(m["atom_type"].shape[0], m["edge_index"], m["edge_type"]).tolist() == [list(q) for q in usable_bridges(m)]
    grid = TR.scan_grid(-PI, PI, PI / 2)
    given = {0: (q0[:2], [1.0, -2.0], [0.1, 0.0]), 2: (np.array(q2[:1]), grid, [0.05])}
    TR.add_torsion_restraints(plain, with_t, given)
    z = np.load(with_t)
    assert z["tors_quads_0"].dtype == np.int32 and z["tors_quads_0"].shape == (2, 4) and z["tors_target_0"].dtype == np.float32
    assert z["tors_target_0"].shape == (2,) and z["tors_target_2"].shape == (4, 1) and z["tors_tol_2"].dtype == np.float32
    assert "tors_quads_1" not in z.files
    back = TR.load_torsion_restraints(with_t)
    assert sorted(back) == [0, 2] and TR.load_torsion_restraints(plain) == {}
    for i, (q, tg, tl) in given.items():
        assert np.array_equal(back[i][0], np.asarray(q, dtype=np.int32)) and np.array_equal(back[i][1], np.asarray(tg, dtype=np.float32))
        assert np.array_equal(back[i][2], np.asarray(tl, dtype=np.float32))
    # every other field is kept, the driver's loader reads the file as before, and distance restraints go on top
    z0 = np.load(plain)
    assert all(np.array_equal(z[k], z0[k]) for k in z0.files)
    again = driver.load_testset(with_t)
    assert [m["name"] for m in again] == ["m0", "m1", "m2"] and np.array_equal(again[2]["atom_type"], mols[2]["atom_type"])
    both = str(tmp_path / "b.npz")
    restraints.add_restraints(with_t, both, {0: ([[0, 1]], [0.5], [3.0])})
    assert sorted(TR.load_torsion_restraints(both)) == [0, 2] and sorted(restraints.load_restraints(both)) == [0]
    a, u, v, b = q0[0]
    for bad in ({3: (q0[:1], [0.0], [0.1])}, {1: ([[0, 1, 2, 99]], [0.0], [0.1])}, {0: (q0[:1], [4.0], [0.1])}, {0: (q0[:1], [0.0], [-0.1])},
                {0: ([q0[0], q0[0]], [0.0, 0.0], [0.1, 0.1])}, {0: ([(a, u, v, u)], [0.0], [0.1])}, {0: (q0[:2], grid, [0.1, 0.1])}):
        with pytest.raises(ValueError):
            TR.add_torsion_restraints(plain, str(tmp_path / "bad.npz"), bad)


@pytest.mark.parametrize("spec", ["2x", "3"])
def test_pack_shifts_by_the_spans_and_takes_target_rows_c_mod_k(spec):
    mols = _mols()
    packed = driver.pack_batch(mols, driver.num_confs(spec))
    q0, q2 = usable_bridges(mols[0]), usable_bridges(mols[2])
    table = np.array([[0.1, -0.1], [0.2, -0.2]], dtype=np.float32)        # K = 2 rows for molecule 0
    per = [(q0[:2], table, [0.1, 0.0]), None, (q2[:1], [1.5], [0.05])]
    q, tg, tl, (row, sp, si) = TR.pack_torsion_restraints(packed, per)
    assert q.dtype == np.int32 and tg.dtype == np.float32 and tl.dtype == np.float32 and row.dtype == sp.dtype == si.dtype == np.int32
    want_tg, k = [], 0
    for m, r, (off, n, g) in zip(mols, per, packed["spans"]):
        if r is None:
            continue
        oq, msp, msi = TR.torsion_sides(n, m["edge_index"], m["edge_type"], r[0])
        for c in range(g):
            for t in range(len(r[0])):
                assert q[k].tolist() == (oq[t] + off + c * n).tolist()
                assert si[sp[row[k]]:sp[row[k] + 1]].tolist() == msi[msp[t]:msp[t + 1]].tolist()      # offsets inside the molecule
                want_tg.append(np.asarray(r[1], dtype=np.float32).reshape(-1, len(r[0]))[c % np.asarray(r[1]).reshape(-1, len(r[0])).shape[0], t])
                k += 1
    assert k == q.shape[0] == 2 * packed["spans"][0][2] + packed["spans"][2][2] and tg.tolist() == [float(x) for x in want_tg]
    assert sp.shape[0] - 1 == 3                                           # the table holds each molecule's rows once
    g0 = packed["spans"][0][2]
    assert tg[:2 * g0].reshape(g0, 2)[:, 0].tolist() == [np.float32(0.1), np.float32(0.2)] * (g0 // 2) + [np.float32(0.1)] * (g0 % 2)
    # the packed restraints pass the sampler's checks on the packed batch, and the bonds give the same table
    N = packed["atom_type"].shape[0]
    got = TR.restraint_arguments(N, q, tg, tl, packed["batch"], (row, sp, si))
    assert got[0][-1] == q.shape[0] and np.array_equal(got[1], q)
    from_bonds = TR.restraint_arguments(N, q, tg, tl, packed["batch"], bond_index=packed["bond_index"], bond_type=packed["bond_type"])
    assert np.array_equal(from_bonds[1], q) and all(np.array_equal(a, b) for a, b in zip(from_bonds[4], (row, sp, si)))
    empty = TR.pack_torsion_restraints(packed, [None, None, None])
    assert empty[0].shape == (0, 4) and TR.restraint_arguments(N, *empty[:3], packed["batch"], empty[3]) is None
    with pytest.raises(ValueError):
        TR.pack_torsion_restraints(packed, per[:2])
    with pytest.raises(ValueError):
        TR.pack_torsion_restraints(packed, [([[0, 1, 2, 99]], [0.0], [0.1]), None, None])
    # a held core: the side without a core atom
    fz = np.zeros(N, dtype=np.uint8)
    off, n, g = packed["spans"][2]
    a, u, v, b = q2[0]
    oq, _, msi = TR.torsion_sides(n, mols[2]["edge_index"], mols[2]["edge_type"], q2[:1])
    held = int(msi[-1])                                                    # an atom of the side that would turn
    fz[off + held + n * np.arange(g)] = 1
    q_f, _, _, (row_f, sp_f, si_f) = TR.pack_torsion_restraints(dict(packed, core_select=fz), [None, None, per[2]])
    assert held not in si_f.tolist() and q_f[0].tolist() == (oq[0][::-1] + off).tolist()


def test_scan_grid():
    g = TR.scan_grid(-PI, PI, PI / 6)
    assert g.dtype == np.float32 and g.shape == (12, 1) and abs(float(g[0, 0]) - PI) < 1e-6 and abs(float(g[1, 0]) + 5 * PI / 6) < 1e-6
    assert (np.abs(g) <= np.float32(PI)).all()
    g = TR.scan_grid(0.0, 2 * PI, PI / 2)                                  # 0, 90, 180, 270 -> -90 degrees
    assert np.allclose(g[:, 0], [0.0, PI / 2, PI, -PI / 2], atol=1e-6)
    assert TR.scan_grid(0.0, 1.0, 0.4).shape == (3, 1) and TR.scan_grid(0.0, 1.2, 0.4).shape == (3, 1)
    for bad in ((0.0, 0.0, 0.1), (1.0, 0.0, 0.1), (0.0, 1.0, 0.0), (0.0, 1.0, -0.1), (0.0, float("inf"), 0.1)):
        with pytest.raises(ValueError):
            TR.scan_grid(*bad)


def test_parser_defaults():
    ap = TR.build_parser()
    a = ap.parse_args(["--ckpt", "c.pt", "--testset", "t.npz", "--out", "o"])
    assert (a.num_confs, a.n_steps, a.w_global, a.global_start_sigma, a.clip) == ("2x", 5000, 1.0, 0.5, 1000.0)
    assert (a.weight, a.start_sigma, a.seed, a.noise, a.precision) == (1.0, float("inf"), 2021, "default", None)
    assert (a.start_idx, a.end_idx, a.trust_ckpt, a.report, a.samples) == (0, 200, False, False, None) and not hasattr(a, "sweeps")
    r = ap.parse_args(["--report", "--samples", "s.npz", "--testset", "t.npz", "--out", "v.npz"])
    assert r.report and r.samples == "s.npz" and r.ckpt is None
    with pytest.raises(SystemExit):
        ap.parse_args(["--ckpt", "c.pt", "--testset", "t.npz", "--out", "o", "--noise", "other"])
    # the distance restraints' parser is what it was
    d = restraints.build_parser().parse_args(["--testset", "t.npz", "--out", "o"])
    assert (d.weight, d.start_sigma, d.sweeps) == (1.0, float("inf"), 1)
