"""The molecules and conformers the E/Z tests share (tests/test_ezbonds_cpu.py, tests/test_hip_ezbonds.py): chains with double
bonds laid out as a planar zigzag (folded into rows, so that 600 atoms stay within 32 A of their centroid and an fp32 ulp stays below 2e-6), with
hydrogens and other substituents hung on them, and seeded conformers of those: the skeleton, about half of the flippable bonds
turned over (an exact float64 rotation of the side row), 0.1 A of noise, a random rigid frame, rounded to float32.
"""
import functools

import numpy as np

import ez_ref as ER
import planarity_ref as PR
from agdiff_amd.ezbonds import flip_sides, stereo_double_bonds

ROW = 28            # backbone atoms per row of the folded zigzag


def chain(m, doubles, extras=(), order=3):
    """A backbone of m carbons 0 .. m - 1 (bond k - (k + 1) of type 2 for k in doubles, else 1) plus extras (parent, atomic number,
    offset [3]), numbered from m on in their order, each bonded to its parent (a backbone atom or an earlier extra) by a single bond.
    Returns (mol = (atom_type, edge_index, edge_type) with the 2- / 3-hop entries of the data sets, skeleton float64 [n, 3])."""
    k = np.arange(m)
    row, col = k // ROW, k % ROW
    col = np.where(row % 2 == 0, col, ROW - 1 - col)
    pos = np.stack([1.25 * col, 2.0 * row + 0.35 * (-1.0) ** k, np.zeros(m)], axis=1)
    atoms = [6] * m
    bonds = [(i, i + 1, 2 if i in doubles else 1) for i in range(m - 1)]
    pos = list(pos)
    for parent, z, off in extras:
        bonds.append((parent, len(atoms), 1))
        atoms.append(z)
        pos.append(pos[parent] + np.asarray(off, dtype=np.float64))
    pos = np.stack(pos)
    return PR.graph(atoms, bonds, order=order), pos - pos.mean(0)


def hyd(k):
    """a hydrogen on backbone atom k, pointing out of the zigzag, in its plane"""
    return (k, 1, (0.0, 1.05 * (-1.0) ** k, 0.0))


def _chain_with_side(length):
    """a - i = j - (a tail of length - 1 atoms): the row of j's side has `length` atoms; frozen = {a} makes flip_sides choose it"""
    return chain(2 + length, {1}), np.arange(2 + length) == 0


#: name -> (mol, skeleton, frozen or None, expected number of stereogenic double bonds)
@functools.lru_cache(maxsize=None)
def molecule(name):
    frozen = None
    if name == "c6":                      # 2-butene's carbons and the two vinyl hydrogens: n = 6, D = 1
        mol, pos = chain(4, {1}, [hyd(1), hyd(2)])
    elif name == "c10":                   # two double bonds three bonds apart: n = 10, D = 2, disjoint sides
        mol, pos = chain(8, {1, 5}, [hyd(1), hyd(6)])
    elif name == "c14":                   # a conjugated triene: n = 14, D = 3, nested sides
        mol, pos = chain(8, {1, 3, 5}, [hyd(k) for k in range(1, 7)])
    elif name.startswith("side"):         # side rows of 2, 63, 64, 65 and 130 atoms: the edges of the lanes' stride
        (mol, pos), frozen = _chain_with_side(int(name[4:]))
    elif name == "big600":                # past the 512 atoms of the LDS graph build; rows of 101, 299 and 99 atoms
        mol, pos = chain(600, {100, 300, 500})
    elif name == "centre":                # a four-neighbour centre (C3: C2, F, Cl, Br) on the side that turns; frozen: atom 0
        mol, pos = chain(4, {1}, [hyd(1), hyd(2), (3, 9, (0.9, -0.5, 0.8)), (3, 17, (0.9, -0.5, -0.9)), (3, 35, (0.3, 1.2, 0.2))])
        frozen = np.arange(9) == 0
    else:
        raise KeyError(name)
    return mol, pos, frozen


def butene(twist_degrees=0.0):
    """(mol, pos float64 [12, 3]): (E)-2-butene with real bond lengths and angles, planar in z = 0 -- C0 - C1 = C2 - C3, H4 on C1, H5
    on C2, methyl hydrogens 6 .. 8 on C0 and 9 .. 11 on C3 -- with C2's side turned about the double bond by twist_degrees, so the
    dihedral C0 - C1 = C2 - C3 is 180 + twist_degrees."""
    import flatten_ref as FR
    ang = lambda deg, r: r * np.array([np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg)), 0.0])
    up = np.array([0.0, 0.0, 1.0])
    c1, c2 = np.zeros(3), np.array([1.34, 0.0, 0.0])
    c0, h4, c3, h5 = c1 + ang(120, 1.50), c1 + ang(240, 1.09), c2 + ang(-60, 1.50), c2 + ang(60, 1.09)
    pos = np.stack([c0, c1, c2, c3, h4, h5] + FR._methyl(c0, c0 - c1, up) + FR._methyl(c3, c3 - c2, up))
    side = [3, 5, 9, 10, 11]
    pos[side] = PR.rotate_about(pos[side], c1, c2, twist_degrees)
    bonds = [(0, 1, 1), (1, 2, 2), (2, 3, 1), (1, 4, 1), (2, 5, 1)] + [(0, k, 1) for k in (6, 7, 8)] + [(3, k, 1) for k in (9, 10, 11)]
    return PR.graph([6] * 4 + [1] * 8, bonds), pos - pos.mean(0)


def signed_dihedral(p, quad):
    """degrees in (-180, 180] of one quad in one conformer"""
    a, i, j, d = (int(x) for x in quad)
    b1, b2, b3 = p[i] - p[a], p[j] - p[i], p[d] - p[j]
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    return float(np.degrees(np.arctan2(np.cross(n1, n2) @ b2 / np.linalg.norm(b2), n1 @ n2)))


EXPECT_D = {"c6": 1, "c10": 2, "c14": 3, "side2": 1, "side63": 1, "side64": 1, "side65": 1, "side130": 1, "big600": 3, "centre": 1}
NAMES = tuple(EXPECT_D)


@functools.lru_cache(maxsize=None)
def tables(name):
    """(quads [D, 4], target int8 [D], side_ptr, side_idx) of a molecule: the target is the skeleton's own parity"""
    mol, pos, frozen = molecule(name)
    quads, in_ring = stereo_double_bonds(*mol)
    assert quads.shape[0] == EXPECT_D[name] and not in_ring.any()
    target = ER.states(pos[None], quads, np.ones(quads.shape[0], dtype=np.int8))[0]
    assert (target != 0).all()
    side_ptr, side_idx = flip_sides(pos.shape[0], mol[1], mol[2], quads, frozen=frozen)
    assert (np.diff(side_ptr) > 0).all()
    return quads, target, side_ptr, side_idx


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@functools.lru_cache(maxsize=None)
def conformers(name, G, seed=0):
    """float32 [G, n, 3] (read-only): per conformer each bond turned over with probability 1 / 2, then 0.1 A of uniform noise on
    every coordinate, a random rotation and a shift of up to 1 A"""
    _, skeleton, _ = molecule(name)
    quads, _, side_ptr, side_idx = tables(name)
    rng = np.random.default_rng([seed, G, len(name), skeleton.shape[0]])
    out = np.empty((G,) + skeleton.shape, dtype=np.float32)
    for g in range(G):
        p = skeleton.copy()
        for c in range(quads.shape[0]):
            if rng.random() < 0.5:
                ER.rotate_side(p, int(quads[c, 1]), int(quads[c, 2]), side_idx[side_ptr[c]:side_ptr[c + 1]])
        p += rng.uniform(-0.1, 0.1, size=p.shape)
        out[g] = (p @ random_rotation(rng).T + rng.uniform(-1.0, 1.0, size=3)).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, G):
    """(pos_out float32, state, flipped, pos_exact float64) of ez_ref.flip on conformers(name, G): computed once, read-only"""
    pos = conformers(name, G)
    quads, target, side_ptr, side_idx = tables(name)
    out, state, flipped = ER.flip(pos, quads, target, side_ptr, side_idx)
    exact, state_x, _ = ER.flip(pos, quads, target, side_ptr, side_idx, exact=True)
    assert np.array_equal(state, state_x)
    for a in (out, state, flipped, exact):
        a.setflags(write=False)
    return out, state, flipped, exact


def moves(name, state):
    """int [G, n]: how many flips moved each atom of each conformer, from a state table (the end atoms of a row do not count)"""
    quads, _, side_ptr, side_idx = tables(name)
    n = molecule(name)[1].shape[0]
    count = np.zeros((state.shape[0], n), dtype=np.int64)
    for c in range(quads.shape[0]):
        row = np.setdiff1d(side_idx[side_ptr[c]:side_ptr[c + 1]], quads[c, 1:3])
        count[np.ix_(state[:, c] < 0, row)] += 1
    return count


SHAPES = tuple((name, G) for name in NAMES for G in (1, 3, 65))

#: max |ez_ref rounding - ez_ref exact| over the atoms moved by two or more flips in SHAPES, in Angstrom, as measured when this was
#: written (1986 entries; the worst ones are big600's, 30 A from an axis whose end atom the first flip had rounded to fp32: one ulp
#: of 1.9e-6 A across a 1.4 A bond tilts the axis by 1.4e-6 rad).  The tests use the live value, nested_deviation(); this record is
#: what tests/test_ezbonds_cpu.py holds it against, within a factor of two.
NESTED_MEASURED = 4.9e-5


@functools.lru_cache(maxsize=None)
def nested_deviation():
    """the live value NESTED_MEASURED records, and the number of (conformer, atom) entries it was taken over"""
    worst, entries = 0.0, 0
    for name, G in SHAPES:
        out, state, _, exact = reference(name, G)
        many = moves(name, state) >= 2
        if many.any():
            worst = max(worst, float(np.abs(out.astype(np.float64) - exact)[many].max()))
            entries += int(many.sum())
    return worst, entries
