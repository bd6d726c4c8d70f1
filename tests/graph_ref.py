"""Plain NumPy restatement of the per-step graph build (csrc/graph.hip: k_graph, k_lg_*; the graph phase of k_sampler_front,
csrc/front.hip) for one packed batch, and the inputs that take the rule to its limits.  tests/test_graph_ref_cpu.py anchors both on
the CPU, tests/test_hip_graph_kernels.py runs every entry point against them on the GPU, bit for bit.

The rule (header of oracle/agdiff_oracle.py): d2 = (dx*dx + dy*dy) + dz*dz in float32 without FMA; source j is a candidate of
target i when d2 < r2, r2 = cutoff * cutoff in float32; the first 33 candidates in ascending index are kept, self included and
then dropped; the static local edges (type > 0) are always present; a kept pair that is no local edge is a radius edge (type 0).
Lengths are sqrt of the float32 d2 taken in float64 and rounded once (csrc/graph.hip: ag_sqrt_rn).

Independent of oracle.radius_graph (a dense torch evaluation): molecules and targets are walked one by one, every operation an
explicit np.float32 one.  `rule=` names the pinned rule ("rule") or one of the wrong ones a kernel could implement instead; the
inputs below are chosen so that each wrong one gives another edge list (asserted in tests/test_graph_ref_cpu.py).

Test infrastructure only."""
import functools

import numpy as np

from agdiff_amd import _lib, synth

CAP = _lib.RADIUS_CAP                            # 33: max_num_neighbors + 1, self included
RS = _lib.DEFINES["AGDIFF_RAD_STRIDE"]
TW = _lib.TILE
RULES = ("rule", "reordered", "fma", "float64", "le", "cap32", "cap34", "self_excluded_first")
f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------- the rule
def r2_of(cutoff, rule="rule"):
    """cutoff * cutoff in float32, as the launchers compute it; "float64": the exact square of the float32 cutoff."""
    c = f32(cutoff)
    return f64(c) * f64(c) if rule == "float64" else f32(c * c)


def d2_of(a, b, rule="rule"):
    """d2 between the positions a [..., 3] and b [..., 3] (float32, a - b), under `rule`'s arithmetic."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == f32 and b.dtype == f32
    if rule == "float64":
        d = a.astype(f64) - b.astype(f64)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d = a - b                    # float32 - float32
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    assert dx.dtype == f32
    if rule == "fma":            # fmaf(dz, dz, fmaf(dy, dy, dx * dx)): every product exact (float64 holds it), one rounding per accumulate
        x, y, z = dx.astype(f64), dy.astype(f64), dz.astype(f64)
        acc = (x * x).astype(f32)
        acc = (y * y + acc.astype(f64)).astype(f32)
        return (z * z + acc.astype(f64)).astype(f32)
    xx, yy, zz = dx * dx, dy * dy, dz * dz
    if rule == "reordered":
        return xx + (yy + zz)
    return (xx + yy) + zz


def d2_row(p, i, rule="rule"):
    """d2(i, j) for every atom j of the molecule p [n, 3] (float32)."""
    return d2_of(p[i][None, :], p, rule)


def in_range(d2, cutoff, rule="rule"):
    r2 = r2_of(cutoff, rule)
    return d2 <= r2 if rule == "le" else d2 < r2


ARITHMETIC = ("reordered", "fma", "float64")


def length_of(d2):
    """(float)sqrt((double)d2): correctly rounded for every float32 d2."""
    return np.sqrt(np.asarray(d2, dtype=f32).astype(f64)).astype(f32)


def kept_sources(p, i, cutoff, rule="rule"):
    """(kept sources of target i in ascending order with self dropped, all candidates) inside the molecule p."""
    within = in_range(d2_row(p, i, rule if rule in ARITHMETIC else "rule"), cutoff, rule)
    if rule == "self_excluded_first":
        within[i] = False
    cand = np.nonzero(within)[0]
    kept = cand[:{"cap32": 32, "cap34": 34}.get(rule, CAP)]
    return kept[kept != i], cand


# ------------------------------------------------------------------------------------------------- the static local edges
def local_edges(b):
    """The coalesced local edge list (models/common.py:215-231): sorted by (src, dst), types of duplicates summed."""
    assert not b.get("extend_order", False)
    N = b["atom_type"].shape[0]
    bi = np.asarray(b["bond_index"], dtype=np.int64).reshape(2, -1)
    uniq, inv = np.unique(bi[0] * N + bi[1], return_inverse=True)
    typ = np.zeros(uniq.shape[0], dtype=np.int64)
    np.add.at(typ, inv.reshape(-1), np.asarray(b["bond_type"], dtype=np.int64))
    return uniq // N, uniq % N, typ


def local_rows(src, dst, typ, batch):
    """Row of every local edge in the canonical local list (agdiff_topo_t.loc_row): one entry per pair of mirror edges of one type
    (the one with src < dst) and one per edge without such a mirror, in order of (molecule, type, source, list position)."""
    at = {(int(s), int(d)): k for k, (s, d) in enumerate(zip(src, dst))}
    mirror = np.asarray([at.get((int(d), int(s)), -1) for s, d in zip(src, dst)], dtype=np.int64)
    has = (mirror >= 0) & (typ[np.maximum(mirror, 0)] == typ)
    canon = np.nonzero(~has | (src < dst))[0]
    canon = np.asarray(sorted(canon, key=lambda k: (batch[src[k]], typ[k], src[k], k)), dtype=np.int64)
    row = np.full(src.shape[0], -1, dtype=np.int64)
    row[canon] = np.arange(canon.shape[0])
    paired = has[canon]
    row[mirror[canon[paired]]] = np.nonzero(paired)[0]
    return row


# ------------------------------------------------------------------------------------------------- the build
def build(b, pos=None, cutoff=None, rule="rule"):
    """Everything a build of batch `b` writes, as int64 / float32 arrays (dict):
      num_edges, e_src, e_dst, e_type, e_len, e_loc  (destination order: targets ascending, sources ascending inside a target)
      in_ptr [N + 1], out_ptr [N + 1], ref2dst (position in that list of the k-th edge in (src, dst) order)
      graph_edge_cnt [G], graph_edge_ptr [G + 1]
      canon[0] (every edge) / canon[1] (canon_radius_only): num_canon, c_src, c_dst, c_type, c_len, c_pos, c_mir, graph_canon_cnt,
        graph_canon_ptr; canon[1] also row_pos / row_mir: c_pos / c_mir as radius-row indices target * RS + rank (the front's form)
      rad_cnt [N], rad_src [N, RS], rad_len [N, RS] (-1 / NaN past a target's count)
      l_len [L]: the length of every local edge of local_edges(b)
      n_within [N], thr [N], self_rank [N]: candidates of a target (self included), index inside the molecule of its 33rd
        candidate (-1: none) and the number of candidates below the target itself -- the reference's own intermediate counts"""
    pos = np.ascontiguousarray(b["pos"] if pos is None else pos, dtype=f32)
    cutoff = b["cutoff"] if cutoff is None else cutoff
    batch, G = np.asarray(b["batch"], dtype=np.int64), int(b["num_graphs"])
    N = batch.shape[0]
    gptr = np.concatenate([[0], np.cumsum(np.bincount(batch, minlength=G))]).astype(np.int64)
    ls, ld, lt = local_edges(b)
    lrow = local_rows(ls, ld, lt, batch)
    lgraph = batch[ls] if ls.size else np.zeros(0, dtype=np.int64)
    lptr = np.searchsorted(lgraph, np.arange(G + 1))          # (the list is sorted by source, hence by molecule)
    e = {k: [] for k in ("e_src", "e_dst", "e_type", "e_len", "e_loc", "ref2dst")}
    canon = [{k: [] for k in ("c_src", "c_dst", "c_type", "c_len", "c_pos", "c_mir", "row_pos", "row_mir")} for _ in range(2)]
    in_ptr, out_ptr = np.zeros(N + 1, dtype=np.int64), np.zeros(N + 1, dtype=np.int64)
    ecnt, ccnt = np.zeros(G, dtype=np.int64), np.zeros((2, G), dtype=np.int64)
    rad_cnt = np.zeros(N, dtype=np.int64)
    rad_src, rad_len = np.full((N, RS), -1, dtype=np.int64), np.full((N, RS), np.nan, dtype=f32)
    l_len = np.zeros(ls.shape[0], dtype=f32)
    n_within, thr, self_rank = np.zeros(N, dtype=np.int64), np.full(N, -1, dtype=np.int64), np.zeros(N, dtype=np.int64)
    ebase = 0
    for g in range(G):
        g0, n = int(gptr[g]), int(gptr[g + 1] - gptr[g])
        p = pos[g0:g0 + n]
        k0, k1 = int(lptr[g]), int(lptr[g + 1])
        L = np.zeros((n, n), dtype=bool)                      # [i, j]: local edge j -> i
        T = np.zeros((n, n), dtype=np.int64)
        EID = np.full((n, n), -1, dtype=np.int64)
        L[ld[k0:k1] - g0, ls[k0:k1] - g0] = True
        T[ld[k0:k1] - g0, ls[k0:k1] - g0] = lt[k0:k1]
        EID[ld[k0:k1] - g0, ls[k0:k1] - g0] = np.arange(k0, k1)
        A = L.copy()                                          # [i, j]: edge j -> i
        D2 = np.zeros((n, n), dtype=f32)
        for i in range(n):
            kept, cand = kept_sources(p, i, cutoff, rule)
            A[i, kept] = True
            D2[i] = d2_row(p, i)
            n_within[g0 + i] = cand.size
            self_rank[g0 + i] = int(np.searchsorted(cand, i))
            if cand.size >= CAP:
                thr[g0 + i] = cand[CAP - 1]
        LEN = length_of(D2)
        l_len[k0:k1] = LEN[ld[k0:k1] - g0, ls[k0:k1] - g0]
        ii, jj = np.nonzero(A)                                # row-major: targets ascending, sources ascending
        P = np.full((n, n), -1, dtype=np.int64)
        P[ii, jj] = ebase + np.arange(ii.size)
        e["e_src"].append(g0 + jj); e["e_dst"].append(g0 + ii); e["e_type"].append(T[ii, jj]); e["e_len"].append(LEN[ii, jj])
        e["e_loc"].append(np.concatenate([lrow, [-1]])[EID[ii, jj]])          # (EID = -1: a radius edge, no row)
        sj, si = np.nonzero(A.T)                              # sources ascending, targets ascending: the (src, dst) order
        e["ref2dst"].append(P[si, sj])
        in_ptr[g0:g0 + n] = ebase + np.cumsum(A.sum(axis=1)) - A.sum(axis=1)
        out_ptr[g0:g0 + n] = ebase + np.cumsum(A.sum(axis=0)) - A.sum(axis=0)
        ecnt[g] = ii.size
        lower = np.tri(n, k=-1, dtype=bool)                   # [i, j]: j < i
        R = A & ~L                                            # radius edges
        RK = np.cumsum(R, axis=1) - 1                         # rank of a radius source inside its target's rows
        ROW = (g0 + np.arange(n))[:, None] * RS + RK
        for mode in (0, 1):
            # mirrors: both directions exist with one type (mode 0) / both are radius edges (mode 1); canonical: the direction with
            # src < dst, and every edge without a mirror
            M = A & A.T & (L == L.T) & (T == T.T) if mode == 0 else R & R.T
            C = (A if mode == 0 else R) & (lower | ~M)
            ci, cj = np.nonzero(C)
            c = canon[mode]
            c["c_src"].append(g0 + cj); c["c_dst"].append(g0 + ci); c["c_type"].append(T[ci, cj]); c["c_len"].append(LEN[ci, cj])
            c["c_pos"].append(P[ci, cj]); c["c_mir"].append(np.where(M[ci, cj], P[cj, ci], -1))
            c["row_pos"].append(ROW[ci, cj]); c["row_mir"].append(np.where(M[ci, cj], ROW[cj, ci], -1))
            ccnt[mode, g] = ci.size
        for i in range(n):
            s = np.nonzero(R[i])[0]
            rad_cnt[g0 + i] = s.size
            rad_src[g0 + i, :s.size] = g0 + s
            rad_len[g0 + i, :s.size] = LEN[i, s]
        ebase += ii.size
    in_ptr[N] = out_ptr[N] = ebase
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    out = {k: cat(v, f32 if k == "e_len" else np.int64) for k, v in e.items()}
    ptr = lambda cnt: np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    out.update(num_edges=ebase, in_ptr=in_ptr, out_ptr=out_ptr, graph_edge_cnt=ecnt, graph_edge_ptr=ptr(ecnt), rad_cnt=rad_cnt,
               rad_src=rad_src, rad_len=rad_len, l_len=l_len, n_within=n_within, thr=thr, self_rank=self_rank, graph_ptr=gptr,
               loc=(ls, ld, lt), loc_row=lrow, canon=[])
    for mode in (0, 1):
        c = {k: cat(v, f32 if k == "c_len" else np.int64) for k, v in canon[mode].items()}
        c.update(num_canon=int(ccnt[mode].sum()), graph_canon_cnt=ccnt[mode], graph_canon_ptr=ptr(ccnt[mode]))
        out["canon"].append(c)
    return out


def edge_keys(ref, N):
    """src * N + dst of every edge of a build: the final list as a set."""
    return ref["e_src"] * N + ref["e_dst"]


def only_in(a, b, N):
    """Edges of build `a` that build `b` of the same batch lacks (keys src * N + dst)."""
    return np.setdiff1d(edge_keys(a, N), edge_keys(b, N))


# ------------------------------------------------------------------------------------------------- input builders
def _bond_graph(rng, n):
    """(atom_type, row, col, type): the order-3 extended bond graph of a random tree with ring closures over n atoms, the builders
    of tests/step_ref.py (dense extension) and tests/large_mols.py (sparse, the same lists) by size."""
    import step_ref
    from large_mols import large_molecule
    return step_ref._molecule(rng, n, False) if n <= 64 else large_molecule(rng, n)


def _pack(mols, cutoff, empty_after=()):
    """mols: (atom_type, row, col, type, pos) per molecule with indices inside the molecule.  empty_after: an empty molecule
    (no atom) follows the molecule with that index."""
    ats, rs, cs, ts, bs, ps, sizes, off, g = [], [], [], [], [], [], [], 0, 0
    for k, (at, r, c, t, p) in enumerate(mols):
        n = at.shape[0]
        assert p.shape == (n, 3) and p.dtype == f32
        ats.append(at); rs.append(np.asarray(r, dtype=np.int64) + off); cs.append(np.asarray(c, dtype=np.int64) + off)
        ts.append(np.asarray(t, dtype=np.int64)); bs.append(np.full(n, g, dtype=np.int64)); ps.append(p); sizes.append(n)
        off += n
        g += 1
        if k in empty_after:
            sizes.append(0)
            g += 1
    return dict(atom_type=np.concatenate(ats).astype(np.int64), bond_index=np.stack([np.concatenate(rs), np.concatenate(cs)]),
                bond_type=np.concatenate(ts), batch=np.concatenate(bs), num_graphs=g, sizes=tuple(sizes), extend_order=False,
                pos=np.concatenate(ps), cutoff=float(cutoff))


def _gauss(rng, n, scale):
    return (rng.standard_normal((n, 3)) * scale).astype(f32)


def _tail(rng, scale=3.0):
    return [_bond_graph(rng, n) + (_gauss(rng, n, scale),) for n in (1, 2, 23)]


SHELL_CUTOFFS = (10.0, 3.7)      # 3.7 * 3.7 is inexact in float32: r2 itself is a rounded number
SHELL_SIZES = (40, 77, 130, 200)
SHELL_CORE = 12
SHELL_SEEDS = {10.0: 1, 3.7: 1}  # fixed draws; tests/test_graph_ref_cpu.py asserts the conditions they have to meet


def shell_batch(cutoff, seed=None):
    """Molecules whose first SHELL_CORE atoms form a compact core; every other atom sits at cutoff * u (u a random unit vector)
    from a core atom, rounded to float32: d2 of that pair lands within a few ulp of r2, on either side or on it.  The core has the
    lowest indices, so the edge core atom -> shell atom is never cut by the cap, and the two are no bond-graph neighbours (local
    edges reach ~20 indices): what the comparison decides is what the final list shows."""
    rng = np.random.default_rng(7000 + (SHELL_SEEDS[cutoff] if seed is None else seed))
    mols = []
    for n in SHELL_SIZES:
        p = np.zeros((n, 3), dtype=f32)
        p[:SHELL_CORE] = _gauss(rng, SHELL_CORE, 0.12 * cutoff)
        for s in range(SHELL_CORE, n):
            u = rng.standard_normal(3)
            u /= np.sqrt((u * u).sum())
            p[s] = (p[rng.integers(0, SHELL_CORE)].astype(f64) + f64(f32(cutoff)) * u).astype(f32)
        mols.append(_bond_graph(rng, n) + (p,))
    return _pack(mols + _tail(rng, 0.3 * cutoff), cutoff)


# |v|^2 = 100 (ties: the strict < rejects them), 99 and 101
LATTICE_100 = ((6, 8, 0), (10, 0, 0), (0, 6, 8), (8, 0, 6), (0, 10, 0), (0, 0, 10), (-8, 6, 0), (0, -8, 6), (6, 0, -8))
LATTICE_99 = ((7, 7, 1), (9, 3, 3), (-7, 1, 7), (5, -5, 7), (3, 9, -3))
LATTICE_101 = ((10, 1, 0), (6, 8, 1), (9, -4, 2), (0, 1, -10), (-8, 6, 1), (2, 4, 9))


def _lattice_molecule(origin, order):
    """Atoms 0 and 1 at `origin` (coincident AND bonded), then one atom per offset of the three tables (order: a permutation), then
    a second atom at the first offset (coincident with it, no bond).  Bonds 0-1, 2-3, 3-4, type 1, both directions."""
    off = np.asarray(LATTICE_100 + LATTICE_99 + LATTICE_101, dtype=np.int64)[order]
    xyz = np.concatenate([np.zeros((2, 3), dtype=np.int64), off, off[:1]]) + np.asarray(origin, dtype=np.int64)
    a, b = np.asarray([0, 2, 3]), np.asarray([1, 3, 4])
    n = xyz.shape[0]
    assert n <= CAP                               # the cap never cuts: every in-range pair is an edge
    return np.full(n, 6, dtype=np.int64), np.concatenate([a, b]), np.concatenate([b, a]), np.ones(6, dtype=np.int64), xyz.astype(f32)


def lattice_batch():
    """Integer coordinates (every d2 exact) at cutoff 10: a molecule at the origin, the same offsets in another order far from the
    origin (coordinates of a few thousand: still exact), two unbonded atoms exactly 10 apart (no edge at all) and two coincident
    unbonded atoms."""
    k = len(LATTICE_100 + LATTICE_99 + LATTICE_101)
    six = np.full(2, 6, dtype=np.int64)
    none = np.zeros(0, dtype=np.int64)
    mols = [_lattice_molecule((0, 0, 0), np.arange(k)), _lattice_molecule((4096, -2048, 1000), np.random.default_rng(5).permutation(k)),
            (six, none, none, none, np.asarray([[0, 0, 0], [10, 0, 0]], dtype=f32)),
            (six, none, none, none, np.asarray([[3, -4, 5], [3, -4, 5]], dtype=f32))]
    return _pack(mols, 10.0)


CLUSTER_SPACING = 30.0           # between cluster centres, along x: three cutoffs
CLUSTER_RADIUS = 1.0             # every atom within this of its centre (per axis): all pairs of a cluster inside the cutoff


def _cluster_molecule(rng, n, cluster_of, bonds=None, centres=None):
    """n atoms, atom k in cluster cluster_of[k]; cluster c at x = CLUSTER_SPACING c (or centres[c])."""
    cluster_of = np.asarray(cluster_of, dtype=np.int64)
    assert cluster_of.shape == (n,)
    x = CLUSTER_SPACING * cluster_of if centres is None else np.asarray(centres, dtype=f64)[cluster_of]
    p = rng.uniform(-CLUSTER_RADIUS, CLUSTER_RADIUS, size=(n, 3))
    p[:, 0] += x
    return (_bond_graph(rng, n) if bonds is None else bonds) + (p.astype(f32),)


def _cap_at(index, n, extra=3):
    """cluster_of for a molecule of n atoms whose cluster 0 has its 33rd member (ascending) at `index`: 31 atoms at every second
    index from index - 63 to index - 3, then index - 1, `index` itself, and `extra` members beyond it (index + 1, + 3, ...).  All
    other atoms form cluster 1."""
    first = list(range(index - 1 - 2 * ((CAP - 2)), index - 1, 2)) + [index - 1]
    assert len(first) == CAP - 1 and first[0] >= 0
    members = first + [index] + [index + 1 + 2 * k for k in range(extra)]
    assert members[-1] < n
    c = np.ones(n, dtype=np.int64)
    c[members] = 0
    return c


CAP_INDICES = (63, 64, 127, 128)  # the 33rd candidate on either side of a 64-lane ballot boundary
SIZES_PATTERN = np.concatenate([np.arange(128) % 4, [1, 2, 2, 3, 3, 3]])      # clusters of exactly 32, 33, 34, 35 atoms
ONE_WAY = dict(n=100, block=35, i=60, j=90)


def _dendrimer():
    import step_ref
    at, r, c, t = step_ref.dendrimer()
    return (at,) + synth.extend_graph_order_np(at.shape[0], r, c, t, order=3)


def clusters_batch():
    """Molecules whose atoms sit in clusters more than a cutoff apart: the candidates of a target are exactly its cluster.
      0     clusters of 32, 33, 34, 35 atoms (index k in cluster k % 4, six more atoms at the end)
      1..4  the 33rd candidate of cluster 0 at index 63, 64, 127, 128; three more members behind it
      5     the dendrimer of tests/step_ref.py in one cluster: the centre's 33 kept candidates are itself and 32 of its 52 local
            sources -- no radius row
      6     ONE_WAY: atoms 0..34 at x = 0, atom j = 90 at x = 8, atom i = 60 at x = 16, the others far away: j -> i is an edge
            (i has two candidates), i -> j is not (35 candidates of j come first): an unpaired radius edge with src > dst; the
            last two members of every cluster of more than 33 atoms receive unpaired edges with src < dst
      then molecules of 1, 2 and 23 atoms."""
    rng = np.random.default_rng(7100)
    mols = [_cluster_molecule(rng, SIZES_PATTERN.shape[0], SIZES_PATTERN)]
    for idx in CAP_INDICES:
        n = 80 if idx < 100 else 144
        mols.append(_cluster_molecule(rng, n, _cap_at(idx, n)))
    mols.append(_cluster_molecule(rng, 53, np.zeros(53, dtype=np.int64), bonds=_dendrimer()))
    w = ONE_WAY
    c = np.full(w["n"], 3, dtype=np.int64)
    c[:w["block"]] = 0
    c[w["j"]], c[w["i"]] = 1, 2
    mols.append(_cluster_molecule(rng, w["n"], c, centres=(0.0, 8.0, 16.0, 4 * CLUSTER_SPACING)))
    return _pack(mols + _tail(rng), 10.0)


def clusters_large_batch():
    """A molecule of 520 atoms (past AGDIFF_MAX_ATOMS_PER_GRAPH: the entry points take the large path by themselves), atom k in
    cluster k % 13 -- 13 clusters of 40, every target at the cap, the 33rd candidate at index 416 + k % 13 --, next to molecules of
    1, 2 and 23 atoms."""
    rng = np.random.default_rng(7200)
    return _pack([_cluster_molecule(rng, 520, np.arange(520) % 13)] + _tail(rng), 10.0)


SHAPE_MAX = (1, 2, 63, 64, 65, 128, 129, 384, 385, 512)
SHAPE_GRAPHS = (511, 512, 1024, 1025, 2050)
EMPTY_IN = 1025                  # this batch has an empty molecule (graph 700)


def shapes_batch(name):
    """"maxN": the largest molecule has N atoms, next to molecules of 1, 2 and 23 atoms (those that are not larger than N); Gaussian
    positions x 3 (odd N) or x 4.5 (even N: part of a larger molecule beyond the cutoff of the rest).
    "graphsG": G molecules of 1, 2 and 3 atoms, single atoms in between, every fifth without bonds (an unbonded pair inside the
    cutoff is a radius edge), raw tree bonds of types 1, 2 (a 3-atom tree leaves one pair unbonded); graphs1025 has an empty
    molecule."""
    rng = np.random.default_rng(7300 + sum(map(ord, name)))
    if name.startswith("max"):
        n = int(name[3:])
        sizes = [n] + [k for k in (1, 2, 23) if k <= n and n > 1] if n > 2 else ([1, 1, 1] if n == 1 else [2, 1, 2, 1])
        return _pack([_bond_graph(rng, k) + (_gauss(rng, k, 3.0 if n % 2 else 4.5),) for k in sizes], 10.0)
    from cfconv_ref import _tree
    G = int(name[6:])
    real = G - (G == EMPTY_IN)
    mols = []
    none = np.zeros(0, dtype=np.int64)
    for k in range(real):
        n = (1, 2, 3, 1, 3, 2, 1)[k % 7]
        r, c, t = _tree(rng, n, (1, 2), 0) if (n > 1 and k % 5 != 3) else (none, none, none)
        mols.append((np.full(n, 6, dtype=np.int64), r, c, t, _gauss(rng, n, 3.0 if k % 3 else 7.0)))
    b = _pack(mols, 10.0, empty_after=(699,) if G == EMPTY_IN else ())
    assert b["num_graphs"] == G
    return b


BATCHES = (["shell10", "shell3.7", "lattice", "clusters", "clusters520"] + ["max%d" % n for n in SHAPE_MAX] +
           ["graphs%d" % g for g in SHAPE_GRAPHS])


@functools.lru_cache(maxsize=None)
def make_batch(name):
    """dict: atom_type, bond_index, bond_type, batch, num_graphs, sizes, extend_order (False), pos float32 [N, 3], cutoff."""
    if name.startswith("shell"):
        return shell_batch(float(name[5:]))
    if name.startswith(("max", "graphs")):
        return shapes_batch(name)
    return {"lattice": lattice_batch, "clusters": clusters_batch, "clusters520": clusters_large_batch}[name]()


@functools.lru_cache(maxsize=None)
def reference(name, rule="rule"):
    """build(make_batch(name)) under `rule`, computed once and shared (the arrays are not modified)."""
    return build(make_batch(name), rule=rule)


def launch_shape(b):
    """(threads per molecule, 32-bit words per mask row, dynamic LDS bytes, workgroup rounds of the scan over the graphs) of the
    LDS build for batch `b`, by the launcher's rule (csrc/graph.hip: graph_build_impl, k_scan_graphs)."""
    mx, G = max(b["sizes"]), b["num_graphs"]
    words = 2 * ((mx + 63) // 64)
    nmax = 32 * words
    return (512 if G >= 512 else 1024), words, (6 * nmax + 2 * nmax * words) * 4, (G + 1023) // 1024
