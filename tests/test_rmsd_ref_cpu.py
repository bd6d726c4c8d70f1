"""CPU: the float64 restatement of the RMSD recipe (tests/rmsd_ref.py) and the gate derived from it are anchored before
tests/test_hip_rmsd_kernels.py holds the kernels to them: the restatement against oracle.covmat_oracle (SVD Kabsch), the
twelve-sweep Jacobi against eigvalsh inside the 64 units the gate reserves for it, what the gate catches that the old 2e-5 bar
does not (a solver stopped after three sweeps), the LDS sizes on their stated sides of 48 KiB and 64 KiB, and the case generator."""
import functools

import numpy as np
import pytest

import rmsd_ref as RM
from oracle import covmat_oracle as CO

SMALL = (1, 2, 3, 12)                                    # m = 1: S = 0; 2: always collinear; 3: always planar
SEEDS = (0, 1, 2, 3)                                      # conformer sets per shape in the sensitivity test
SIZES = SMALL + tuple(sorted(set(RM.SHAPES["matrix"] + RM.SHAPES["self"])))


@functools.lru_cache(maxsize=None)
def _case(m, seed=0):
    """(molecule, stored centred ref [R, m, 3], stored centred gen [G, m, 3]) -- computed once, read-only"""
    mol = RM.molecule(m, seed)
    cref, cgen = RM.stored_centres(mol["ref"], mol["heavy"]), RM.stored_centres(mol["gen"], mol["heavy"])
    cref.setflags(write=False)
    cgen.setflags(write=False)
    return mol, cref, cgen


@functools.lru_cache(maxsize=None)
def _solved(m, sweeps, seed=0):
    """[(kind, j, i, msd, mirror, delta, gsum)] of every named pair of _case(m, seed) over the mappings `maps`: sweeps = 0 is eigvalsh,
    else jacobi4 with that many (None: jacobi4's default)"""
    mol, cref, cgen = _case(m, seed)
    eig = np.linalg.eigvalsh if sweeps == 0 else RM.jacobi_eig(*(() if sweeps is None else (sweeps,)))
    out = []
    for kind, j, i in RM.kinds_of(mol):
        msd, mir, delta = RM.pair_msd(cgen[i], cref[j], mol["maps"], eig=eig)
        out.append((kind, j, i, float(msd), float(mir), float(delta), float(delta) / ((4 * m + 64) * RM.U) * m))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("m", SIZES)
def test_the_restatement_matches_the_oracle(m):
    """centre -> one rounding to fp32 -> pair_msd -> sqrt, against kabsch_rmsd / best_rmsd of the fp32 inputs (float64 SVD, centred
    in float64 and never rounded), and against the oracle on the point-inverted conformer for the mirror value.  The RMSD is
    1-Lipschitz in the RMS displacement of either conformer and each centred coordinate moves by at most half an ulp, 2^-24 of
    itself: sqrt(3) 2^-24 max|coordinate| per conformer, two conformers."""
    mol, cref, cgen = _case(m)
    heavy, perms = mol["heavy"], mol["maps"]
    worst = 0.0
    seen = set()
    for kind, j, i, msd, mir, delta, _ in _solved(m, 0):
        gen, ref = mol["gen"][i], mol["ref"][j]
        bound = 2.0 * np.sqrt(3.0) * 2.0 ** -24 * max(np.abs(cref[j]).max(), np.abs(cgen[i]).max())
        want = CO.best_rmsd(gen, ref, heavy, perms)
        inverted = gen.astype(np.float64).copy()
        inverted[heavy] = 2.0 * inverted[heavy].mean(0) - inverted[heavy]
        want_mirror = CO.best_rmsd(inverted, ref, heavy, perms)
        e = max(abs(np.sqrt(max(msd, 0.0)) - want), abs(np.sqrt(max(mir, 0.0)) - want_mirror))
        assert e <= bound, (kind, j, i, e, bound)
        worst = max(worst, e / bound) if bound > 0 else worst
        seen.add(kind)
    print("m = %d: largest |restatement - oracle| / bound = %.3f over %d pairs" % (m, worst, len(_solved(m, 0))))
    assert seen >= set(RM.KINDS) and (m < 5 or seen >= {"twin", "mirror"})
    # kabsch_rmsd directly, identity mapping: the unrelated pair
    j, i = mol["pairs"]["unrelated"][0]
    msd = RM.pair_msd(cgen[i], cref[j])[0]
    assert abs(np.sqrt(msd) - CO.kabsch_rmsd(mol["gen"][i][heavy], mol["ref"][j][heavy])) <= 2.0 * np.sqrt(3.0) * 2.0 ** -24 * max(
        np.abs(cref[j]).max(), np.abs(cgen[i]).max())


# ------------------------------------------------------------------------------------------------ 2. the solver
@pytest.mark.parametrize("m", SIZES)
def test_twelve_jacobi_sweeps_are_within_the_64_units_of_eigvalsh(m):
    worst, kinds = 0.0, set()
    for a, b in zip(_solved(m, 0), _solved(m, None)):
        kind, j, i, msd, mir, delta, gsum = a
        unit = RM.U * gsum / m
        for x, y in ((msd, b[3]), (mir, b[4])):
            assert abs(x - y) <= 64 * unit, (kind, j, i, abs(x - y) / unit if unit else abs(x - y))
            worst = max(worst, abs(x - y) / unit) if unit > 0 else worst
        kinds.add(kind)
    print("m = %d: twelve sweeps differ from eigvalsh by at most %.1f units of 2^-53 gsum / m" % (m, worst))
    assert kinds >= set(RM.KINDS)          # S = 0 at m = 1, rank 1 (collinear), rank 2 (planar) and x = y (identical) among them


def test_the_degenerate_key_matrices_are_what_they_are_said_to_be():
    mol, cref, cgen = _case(1)
    assert not cref.any() and not cgen.any()                                     # m = 1: centred coordinates 0, S = 0, msd = 0
    assert RM.pair_msd(cgen[0], cref[0])[0] == 0.0 and RM.pair_msd(cgen[0], cref[0], eig=RM.jacobi_eig())[0] == 0.0
    mol, cref, cgen = _case(128)
    rank = lambda j, i: int(np.linalg.matrix_rank(cgen[i].astype(np.float64).T @ cref[j].astype(np.float64), tol=1e-9))
    assert rank(*mol["pairs"]["collinear"][0]) == 1 and rank(*mol["pairs"]["planar"][0]) == 2
    j, i = mol["pairs"]["identical"][0]
    assert np.array_equal(cref[j], cgen[i])
    msd, _, delta = RM.pair_msd(cgen[i], cref[j], eig=RM.jacobi_eig())
    assert abs(msd) <= delta


# ------------------------------------------------------------------------------------------------ 3. sensitivity
@pytest.mark.parametrize("m", sorted(set(RM.SHAPES["matrix"] + RM.SHAPES["self"])))
def test_the_gate_rejects_a_solver_cut_to_three_sweeps_that_the_old_bar_accepts(m):
    """The value a kernel would store is float32(sqrt(msd)) of its solver, for the proper and for the mirror value of every noise
    and unrelated pair.  With jacobi4 as it stands every such value is inside the gate.  Cut to three sweeps, at least one value of
    every shape is within the old 2e-5 Angstrom of the truth -- tests/test_hip_eval.py and test_hip_ensemble.py would pass it --
    and outside the gate; nothing the old bar rejects gets through the gate either.  Asserted for the conformer set the GPU tests
    use (seed 0) and for at least one more of the independent sets of SEEDS."""
    per_seed = []
    for seed in SEEDS:
        exact, full, cut = _solved(m, 0, seed), _solved(m, None, seed), _solved(m, 3, seed)
        caught_by_gate_alone = caught_by_both = values = 0
        for e, f, c in zip(exact, full, cut):
            if e[0] not in ("noise", "unrelated"):
                continue
            for col in (3, 4):                                                   # proper, mirror
                stored_full = np.float32(np.sqrt(max(f[col], 0.0)))
                stored_cut = np.float32(np.sqrt(max(c[col], 0.0)))
                assert RM.in_gate(stored_full, e[col], e[5]), (seed, e[:3], col)
                old_accepts = abs(float(stored_cut) - np.sqrt(e[col])) < RM.OLD_BAR
                new_accepts = bool(RM.in_gate(stored_cut, e[col], e[5]))
                assert old_accepts or not new_accepts, (seed, e[:3], col)
                caught_by_gate_alone += int(old_accepts and not new_accepts)
                caught_by_both += int(not old_accepts)
                values += 1
        print("m = %d seed %d: of %d three-sweep values the gate alone rejects %d, gate and 2e-5 bar both %d"
              % (m, seed, values, caught_by_gate_alone, caught_by_both))
        per_seed.append(caught_by_gate_alone)
    assert per_seed[0] >= 1                                  # the molecule the GPU tests use
    assert sum(c >= 1 for c in per_seed) >= 2                # and in another, independent set: not by the luck of one seeded pair


def test_the_gate_is_one_fp32_value_wide_away_from_zero_and_a_micro_angstrom_at_zero():
    mol, cref, cgen = _case(256)
    for kind, j, i, msd, mir, delta, _ in _solved(256, 0):
        lo, hi = RM.gate(msd, delta)
        if msd > 1e-6:                                                           # RMSD above 1e-3 Angstrom
            assert hi == lo or hi == np.nextafter(lo, np.float32(np.inf)), (kind, j, i)
        else:
            assert lo == 0.0 and hi <= 2e-6, (kind, j, i, hi)
    assert not RM.in_gate(np.float32(np.nextafter(RM.gate(1.0, 1e-14)[1], np.float32(2))), 1.0, 1e-14)
    assert RM.in_gate(np.float32(1.0), 1.0, 1e-14) and RM.in_gate(np.float32(0.0), 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ 4. LDS sizes
def test_lds_sizes_sit_on_their_stated_sides_of_48_and_64_kib():
    from agdiff_amd import _lib
    M, Q = _lib.DEFINES["AGDIFF_RMSD_MAX_ATOMS"], _lib.DEFINES["AGDIFF_TFD_MAX_COLUMNS"]
    assert (M, Q) == (256, 512)
    k48, k64 = 48 * 1024, 64 * 1024
    for kernel in ("matrix", "self", "tfd"):
        below48, first48, below64, first64 = RM.SHAPES[kernel][:4] if kernel != "tfd" else RM.SHAPES[kernel][:2] + (511, 512)
        assert RM.lds_bytes(kernel, below48) <= k48 < RM.lds_bytes(kernel, first48), kernel
        assert RM.lds_bytes(kernel, below64) <= k64 < RM.lds_bytes(kernel, first64), kernel
        assert RM.SHAPES[kernel][-1] == (Q if kernel == "tfd" else M)
    assert RM.lds_bytes("self", 122) == k48                                      # exactly 48 KiB: still the first path
    assert RM.lds_bytes("matrix", M) == 98432 and RM.lds_bytes("self", M) == 100608
    assert RM.lds_bytes("tfd", Q) == 65664 and RM.lds_bytes("tfd_terms", Q, Q) == 73856
    assert RM.lds_bytes("tfd", 383) == RM.lds_bytes("tfd", 382) == k48 - 128 and RM.lds_bytes("tfd", 384) == k48 + 128      # the pitch is odd
    assert RM.lds_bytes("tfd_terms", 383, 383) > k48                             # the terms kernel at T = Q is past 48 KiB at every Q here


# ------------------------------------------------------------------------------------------------ 5. the case generator
@pytest.mark.parametrize("m", SIZES)
def test_the_molecule_has_exactly_m_heavy_atoms_and_its_twins_match_under_one_mapping(m):
    mol, cref, cgen = _case(m)
    at, heavy = mol["atom_type"], mol["heavy"]
    assert int((at != 1).sum()) == m == heavy.shape[0] and np.array_equal(heavy, np.nonzero(at != 1)[0])
    assert mol["ref"].dtype == mol["gen"].dtype == np.float32 and mol["ref"].shape == (5, mol["n"], 3) and mol["gen"].shape == (18, mol["n"], 3)
    if m >= 12:
        assert mol["n"] > m and not np.array_equal(np.diff(heavy), np.full(m - 1, np.diff(heavy)[0]))      # hydrogens, irregularly
    if m < 5:
        assert mol["perms"] is None and mol["maps"] is None and mol["self_twin"] is None
        return
    perms = mol["perms"]
    assert perms.shape == (6, m) and all(np.array_equal(np.sort(p), np.arange(m)) for p in perms)
    table = {tuple(p) for p in perms}
    assert all(tuple(a[b]) in table for a in perms for b in perms)               # closed: a group
    for name, (j, i), which, col in (("twin", mol["pairs"]["twin"][0], 1, 0), ("mirror", mol["pairs"]["mirror"][0], 4, 1)):
        per_map = [np.sqrt(max(float(RM.pair_msd(cgen[i], cref[j], [p])[col]), 0.0)) for p in perms]
        assert per_map[which] < 5e-6 and all(v > 1e-2 for k, v in enumerate(per_map) if k != which), (name, per_map)
        other = np.sqrt(float(RM.pair_msd(cgen[i], cref[j], [perms[which]])[1 - col]))
        assert m < 12 or other > 1e-2, (name, other)                              # chiral: the other hand does not superpose
    a, b = mol["self_twin"]
    per_map = [np.sqrt(max(float(RM.pair_msd(cgen[a], cgen[b], [p])[0]), 0.0)) for p in perms]
    assert per_map[1] < 5e-6 and all(v > 1e-2 for k, v in enumerate(per_map) if k != 1)      # gen 9 = gen 0 by c c: x = conformer 0 needs c
    # the one-way set of a reference x generated matrix holds c and c s without their inverses: the direction of a mapping shows
    maps = mol["maps"]
    assert np.array_equal(maps, perms[[0, 1, 3, 4]]) and not np.array_equal(perms[1][perms[1]], perms[0])
    have = {tuple(p) for p in maps}
    assert tuple(np.argsort(perms[1])) not in have and tuple(np.argsort(perms[4])) not in have
    for (j, i), col in ((mol["pairs"]["twin"][0], 0), (mol["pairs"]["mirror"][0], 1)):
        right = RM.pair_msd(cgen[i], cref[j], maps)[col]
        inverse = RM.pair_msd(cgen[i], cref[j], [np.argsort(p) for p in maps])[col]          # a kernel that applied the inverse mappings
        swapped = RM.pair_msd(cref[j], cgen[i], maps)[col]                                   # or mapped the other conformer's atoms
        assert np.sqrt(max(right, 0.0)) < 5e-6 and np.sqrt(inverse) > 1e-2 and np.sqrt(swapped) > 1e-2
    # the sets of another size grow by noise conformers only: the named pairs stay where they are
    big = RM.molecule(m, R=17, G=33)
    assert big["ref"].shape[0] == 17 and big["gen"].shape[0] == 33 and big["pairs"]["twin"] == mol["pairs"]["twin"]

