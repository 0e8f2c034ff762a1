"""NumPy statement of the voxel-occupancy counts (include/pccm.h, pccm_voxel_occupancy) -- the yardstick of the occupancy tests --
and the planted families those tests run on, each with the triple (nA, nB, nAB) it was BUILT to have: derived from how the family
is made (or, for the boundary families, from exact rational arithmetic), not from ``occupancy`` below.

A row's voxel is ``np.floor(x / v) + 0.0`` per component: the correctly rounded fp64 quotient, floored, -0.0 folded onto 0.0."""
import fractions
import functools
import math

import numpy as np


def occupancy(a, b, v):
    ka = np.unique(np.floor(np.asarray(a, np.float64) / v) + 0.0, axis=0)
    kb = np.unique(np.floor(np.asarray(b, np.float64) / v) + 0.0, axis=0)
    both = len(ka) + len(kb) - len(np.unique(np.vstack([ka, kb]), axis=0))
    return len(ka), len(kb), both


def occupancy_by_reciprocal(a, b, v):
    """What a kernel that multiplies by 1 / v instead of dividing would count (the boundary families tell the two apart)."""
    r = np.float64(1.0) / np.float64(v)
    ka = np.unique(np.floor(np.asarray(a, np.float64) * r) + 0.0, axis=0)
    kb = np.unique(np.floor(np.asarray(b, np.float64) * r) + 0.0, axis=0)
    both = len(ka) + len(kb) - len(np.unique(np.vstack([ka, kb]), axis=0))
    return len(ka), len(kb), both


def exact_voxel(x: float, v: float) -> int:
    """floor of the correctly rounded fp64 quotient x / v, without a floating-point division: the exact rational quotient of the
    two doubles, rounded to the nearest double by Fraction.__float__ (integer arithmetic), then floored."""
    return math.floor(float(fractions.Fraction(x) / fractions.Fraction(v)))


def exact_occupancy(a, b, v):
    """The triple by exact rational arithmetic and Python sets (slow: for the planted families only)."""
    def keys(pts):
        return {tuple(exact_voxel(float(c), float(v)) for c in row) for row in np.asarray(pts, dtype=np.float64)}
    ka, kb = keys(a), keys(b)
    return len(ka), len(kb), len(ka & kb)


def rows(triple, voxel):
    """The report rows of one voxel size from its triple, keyed as the metrics key them, in report order."""
    n_a, n_b, n_ab = (int(c) for c in triple)
    v = float(voxel)
    return {
        ("OccupiedVoxels", True, v): np.float64(n_a),
        ("OccupiedVoxels", False, v): np.float64(n_b),
        ("VoxelCoverage", True, v): np.float64(n_ab) / np.float64(n_a),
        ("VoxelCoverage", False, v): np.float64(n_ab) / np.float64(n_b),
        ("VoxelIoU", v): np.float64(n_ab) / np.float64(n_a + n_b - n_ab),
    }


def _lattice(nx, ny, nz, x0=0):
    g = np.stack(np.meshgrid(np.arange(x0, x0 + nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1)
    return g.reshape(-1, 3).astype(np.float64)


@functools.lru_cache(maxsize=None)
def planted(name):
    """-> (a, b, voxel, (nA, nB, nAB) by construction)."""
    rng = np.random.default_rng(31)
    if name == "one_voxel":
        # every point of both clouds strictly inside the voxel [3, 4) x [-2, -1) x [0, 1): the contended slot
        lo = np.array([3.0, -2.0, 0.0])
        a = lo + 0.001 + 0.998 * rng.random((1000, 3))
        b = lo + 0.001 + 0.998 * rng.random((1000, 3))
        return a, b, 1.0, (1, 1, 1)
    if name == "subset":
        # every point its own voxel: A is a 5 x 5 x 5 block of the 7 x 6 x 5 block B, both shuffled
        a, b = _lattice(5, 5, 5), _lattice(7, 6, 5)
        return a[rng.permutation(len(a))], b[rng.permutation(len(b))], 1.0, (125, 210, 125)
    if name == "disjoint":
        a, b = _lattice(5, 5, 5), _lattice(5, 5, 5, x0=10) * np.array([1.0, -1.0, 1.0]) - np.array([0.0, 1.0, 0.0])
        return a[rng.permutation(125)], b[rng.permutation(125)], 1.0, (125, 125, 0)
    if name == "multiplicities":
        # the same 6 x 5 x 4 voxels in both clouds, three points in each in A and one to five in B, anywhere inside the voxel
        cells = _lattice(6, 5, 4) - 3.0
        a = np.repeat(cells, 3, axis=0)
        b = np.repeat(cells, rng.integers(1, 6, len(cells)), axis=0)
        a, b = a + 0.9375 * rng.random(a.shape), b + 0.9375 * rng.random(b.shape)
        return a[rng.permutation(len(a))], b[rng.permutation(len(b))], 1.0, (120, 120, 120)
    if name == "boundary_tenths":
        # x = k * 0.1 in A and x = k / 10 in B, k = -200..200, on voxels of 0.1: the two roundings of "k tenths" fall on
        # different sides of some voxel faces, and so would x * (1 / 0.1); y and z hold both zeros
        k = np.arange(-200, 201, dtype=np.float64)
        a = np.stack([k * 0.1, np.where(k % 2 == 0, -0.0, 0.0), np.zeros_like(k)], axis=1)
        b = np.stack([k / 10.0, np.zeros_like(k), np.where(k % 3 == 0, -0.0, 0.0)], axis=1)
        return a, b, 0.1, exact_occupancy(a, b, 0.1)
    if name == "boundary_far":
        # coordinates near +-1e9 on voxels of 1e-3: voxel indices near 1e12 (no int32 holds them), built by two roundings
        k = np.arange(0, 201, dtype=np.float64)
        sign = np.where(np.arange(201) % 2 == 0, 1.0, -1.0)
        a = np.stack([sign * (1.0e9 + k * 1e-3), k * 1e-3, -k * 1e-3], axis=1)
        b = np.stack([sign * (1.0e9 + k / 1000.0), k / 1000.0, -(k / 1000.0)], axis=1)
        return a, b, 1e-3, exact_occupancy(a, b, 1e-3)
    raise KeyError(name)


PLANTED = ("one_voxel", "subset", "disjoint", "multiplicities", "boundary_tenths", "boundary_far")
BOUNDARY = ("boundary_tenths", "boundary_far")

RAGGED = ((1, 1), (63, 65), (64, 64), (300, 200), (1000, 777))


@functools.lru_cache(maxsize=None)
def ragged(n1, n2, dtype="float32"):
    """Uniform random clouds in the unit cube and a voxel size that gives about as many voxels as points: every row mostly its own
    table entry, at the table's fullest (cap is the power of two >= 2 (n1 + n2), 64 for the tiny cases), with probe chains."""
    rng = np.random.default_rng(1000 * n1 + n2)
    a = rng.random((n1, 3)).astype(dtype)
    near = a[: min(n1 // 3, n2)].astype(np.float64) + 1e-4              # a third of A again, a hair away: mostly shared voxels
    b = np.concatenate([near, rng.random((n2 - len(near), 3))]).astype(dtype)
    voxel = 0.05 if n1 + n2 > 100 else 0.3
    return a, b, voxel
