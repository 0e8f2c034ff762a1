"""A second, independent witness for the exact nearest-neighbour rule (include/pccm.h, pccm_nn): plain fp64 NumPy brute force,
d2 = ((dx*dx) + (dy*dy)) + (dz*dz) with every operation rounded on its own, exact ties to the smallest row.  Chunked over the
queries so that a 20k x 20k pair needs ~50 MB at a time.  Slow on purpose: nothing here shares code with the oracle's kd-tree."""
import numpy as np


def nn_brute(iter_pts, search_pts, *, skip_same_index=False, chunk=256):
    q = np.asarray(iter_pts, dtype=np.float64)
    r = np.asarray(search_pts, dtype=np.float64)
    n = q.shape[0]
    idx = np.empty(n, dtype=np.int64)
    d2 = np.empty(n, dtype=np.float64)
    rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        dx = q[s:e, 0:1] - rx
        dy = q[s:e, 1:2] - ry
        dz = q[s:e, 2:3] - rz
        d = (dx * dx + dy * dy) + dz * dz       # NumPy evaluates left to right: ((dx*dx) + (dy*dy)) + (dz*dz), no fused ops
        if skip_same_index:
            rows = np.arange(s, e)
            d[rows - s, rows] = np.inf
        j = np.argmin(d, axis=1)                # first occurrence of the minimum: the smallest row among exact ties
        idx[s:e] = j
        d2[s:e] = d[np.arange(e - s), j]
    return idx, d2
