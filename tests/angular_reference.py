"""NumPy restatement of the plane-to-plane angular similarity (include/pccm.h, PCCM_METRIC_ANGULAR) -- the yardstick of the
angular tests.

TEST INFRASTRUCTURE.  Every operation is one NumPy element-wise op on fp64 arrays, so each is rounded separately, as the
device's __dmul_rn / __dadd_rn / __dsqrt_rn / __ddiv_rn are.  Only ``np.arccos`` and the device's ``acos`` may differ, in the last
bit.  ``angular_rows`` takes the matched rows of a direction; ``angular_tie_mean`` takes the tie sets of tests/ties_reference.py
and averages the per-neighbour values in ascending row order."""
import numpy as np

from ties_reference import tie_sets


def angular_similarity(a, b):
    """s of every row pair of a [n, 3] and b [n, 3] (fp64)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    na2 = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    nb2 = (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]
    den = np.sqrt(na2 * nb2)
    zero = den == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.minimum(np.abs(dot) / np.where(zero, 1.0, den), 1.0)
    s = 1.0 - (2.0 * np.arccos(c)) / np.pi
    return np.where(zero, 0.0, s)


def angular_rows(own_normals, other_normals, idx):
    """The pick's column: row i's normal against the normal of its matched row idx[i]."""
    other = np.asarray(other_normals, dtype=np.float64)
    return angular_similarity(own_normals, other[np.asarray(idx, dtype=np.int64)])


def angular_tie_mean(own_normals, other_normals, sets):
    """Under ties="mean": per row, (((s_j1 + s_j2) + s_j3) + ...) / k over its ascending tie set."""
    own, other = np.asarray(own_normals, dtype=np.float64), np.asarray(other_normals, dtype=np.float64)
    out = np.empty(len(sets))
    for i, rows in enumerate(sets):
        vals = angular_similarity(np.repeat(own[i:i + 1], len(rows), axis=0), other[rows])
        acc = vals[0]
        for v in vals[1:]:
            acc = acc + v
        out[i] = acc / np.float64(len(rows))
    return out


def angular_mean_column(q_points, r_points, own_normals, other_normals):
    """angular_tie_mean over the tie sets of q in r (dense enumeration: small clouds only)."""
    _, sets = tie_sets(q_points, r_points)
    return angular_tie_mean(own_normals, other_normals, sets)
