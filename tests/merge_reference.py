"""NumPy restatement of merged duplicate points (include/pccm.h, pccm_merge_duplicates) -- the yardstick of the merge tests.

Rows whose fp64 coordinates are equal (``==`` per component: ``-0.0`` equals ``+0.0``) form a group ``i_1 < ... < i_m`` with
representative ``i_1``.  The merged cloud has one row per group in ascending order of representative, with the representative's
coordinates and normal bit for bit and -- ``mode`` "drop" -- its colour, or -- "average" -- per component
``(((c[i_1] + c[i_2]) + ...) + c[i_m]) / m``: a plain Python left-to-right loop over ascending rows, every add rounded
separately, one division.  ``map[i]`` is the merged row of original row ``i``."""
import numpy as np


def groups(points):
    """-> (inverse [n]: the group of every row, numbered in ascending order of representative; representatives [n'])."""
    pts = np.asarray(points).astype(np.float64) + 0.0                  # (-0.0 + 0.0 = +0.0: one key for both zeros)
    _, inverse = np.unique(pts, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    first = np.full(int(inverse.max()) + 1, len(pts), dtype=np.int64)
    np.minimum.at(first, inverse, np.arange(len(pts), dtype=np.int64))
    order = np.argsort(first)                                          # groups by ascending representative
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return rank[inverse], first[order]


def _merged(points, normals, colours, mode, reverse):
    if mode not in ("drop", "average"):
        raise ValueError(mode)
    pts = np.asarray(points).astype(np.float64)
    mapping, reps = groups(pts)
    out_p = pts[reps].copy()
    out_n = None if normals is None else np.asarray(normals).astype(np.float64)[reps].copy()
    out_c = None
    if colours is not None:
        col = np.asarray(colours).astype(np.float64)
        out_c = col[reps].copy()
        if mode == "average":
            members = [[] for _ in reps]
            for i, g in enumerate(mapping.tolist()):                   # ascending rows
                members[g].append(i)
            for g, rows in enumerate(members):
                if len(rows) == 1:
                    continue                                           # (m = 1: the input bits)
                rows = rows[::-1] if reverse else rows
                for a in range(3):
                    s = float(col[rows[0], a])
                    for r in rows[1:]:
                        s = s + float(col[r, a])
                    out_c[g, a] = s / float(len(rows))
    return out_p, out_n, out_c, mapping.astype(np.int32)


def merged(points, normals, colours, mode):
    """-> (points', normals' or None, colours' or None, map) as the library must hold them."""
    return _merged(points, normals, colours, mode, False)


def merged_reversed(points, normals, colours, mode):
    """The same with every group's colours summed in DESCENDING row order: what a kernel that ignored the order could produce."""
    return _merged(points, normals, colours, mode, True)


def drawn_20000():
    """The summation-order family: 20000 rows over 12000 fp32 positions, colours of mixed magnitude."""
    rng = np.random.default_rng(0)
    keys = rng.random((12000, 3), dtype=np.float32)
    pts = keys[rng.integers(0, 12000, 20000)]
    n = len(pts)
    colours = rng.random((n, 3)) * 10.0 ** rng.uniform(-6, 0, (n, 1))
    return pts, colours
