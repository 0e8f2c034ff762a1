"""The stop rule of the k-NN searches of pccm_knn.hip (knn_stop_bound, pccm_knn.h), restated on the host, and the stage each query is settled in.

TEST INFRASTRUCTURE.  It does not import the product's kernels: the constants are parsed from pccm_knn.h, the grid (org, h,
dim) is the one the engine reports (Engine.grid_geometry), everything else is NumPy.  Shared by the point-to-distribution tests
(a search across the clouds) and the normal-estimation tests (a cloud against itself)."""
import os
import re

import numpy as np

import p2d_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WAVE2, WAVE3, THREAD_CAP, THREAD_RINGS, FULL = range(5)
STAGES = {WAVE2: "wave search, r = 2", WAVE3: "wave search, r = 3", THREAD_CAP: "per-thread search, more than kWCap candidates",
          THREAD_RINGS: "per-thread search, rings beyond 3", FULL: "full scan"}


def constant(name):
    src = open(os.path.join(ROOT, "open_pcc_metric_amd", "csrc", "pccm_knn.h")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))


def cells_of(p, org, h, dim):
    """ncell_coord of every row of p: floor((v - org) / h), clamped into the grid."""
    return np.clip(np.floor((p - org) / h), 0, np.asarray(dim) - 1).astype(np.int64)


def face_bound(q, c, r, org, h, dim):
    """L of the stop rule for the cube [c - r, c + r]^3: the distance from q to the nearest face of the cube that is not a face of
    the grid, less the slack; inf when the cube covers the grid."""
    slack = (np.abs(org) + (dim + 2) * h) * 2.0 ** -48
    L = np.inf
    for x in range(3):
        if c[x] - r > 0:
            L = min(L, (q[x] - (org[x] + (c[x] - r) * h[x])) - slack[x])
        if c[x] + r < dim[x] - 1:
            L = min(L, ((org[x] + (c[x] + r + 1) * h[x]) - q[x]) - slack[x])
    return L


def settles(q, b, cells_b, org, h, dim, k, rings):
    """Does the searches' stop rule settle query q within `rings` rings of the grid (org, h, dim)?  (The rule of k_knn_normals,
    restated: the k-th best distance inside the cube against the nearest face of the cube that is not a face of the grid.)"""
    c = np.clip(np.floor((q - org) / h), 0, dim - 1).astype(np.int64)
    for r in range(rings + 1):
        inside = np.all(np.abs(cells_b - c) <= r, axis=1)
        L = face_bound(q, c, r, org, h, dim)
        if L == np.inf:
            return True
        d2 = np.sort(ref.sq_dist(q[None, :], b[inside]))
        if len(d2) >= k and L > 0 and d2[k - 1] < L * L * (1.0 - 2.0 ** -30):
            return True
    return False


def classify(queries, b, org, h, dim, k, wcap=None, max_ring=None):
    """The stage (WAVE2 .. FULL) that settles each row of `queries` in a k-NN search over the cloud b on the grid (org, h, dim),
    following estimate_normals' chain: k_knn_cov_wave tries the cubes r = 2 and r = 3 and gives up on more than kWCap
    candidates; k_knn_normals walks the rings 0 .. kKnnMaxRing; k_knn_normals_full takes what is still open."""
    wcap = constant("kWCap") if wcap is None else wcap
    max_ring = constant("kKnnMaxRing") if max_ring is None else max_ring
    org, h = np.asarray(org, dtype=np.float64), np.asarray(h, dtype=np.float64)
    dim = np.asarray(dim).astype(np.int64)
    queries, b = np.asarray(queries, dtype=np.float64), np.asarray(b, dtype=np.float64)
    cells_b = cells_of(b, org, h, dim)
    out = np.empty(len(queries), dtype=np.int64)
    for i, q in enumerate(queries):
        c = cells_of(q, org, h, dim)
        cheb = np.max(np.abs(cells_b - c), axis=1)
        d2 = ref.sq_dist(q[None, :], b)

        def closed(r):
            """the rule of one cube: (settled, candidates)"""
            inside = cheb <= r
            T = int(np.count_nonzero(inside))
            L = face_bound(q, c, r, org, h, dim)
            if L == np.inf:
                return True, T
            if T < k or not L > 0:
                return False, T
            return bool(np.partition(d2[inside], k - 1)[k - 1] < L * L * (1.0 - 2.0 ** -30)), T

        stage, handed_for_cap = None, False
        for r, name in ((2, WAVE2), (3, WAVE3)):
            ok, T = closed(r)
            if T > wcap:
                handed_for_cap = True
                break
            if ok:
                stage = name
                break
        if stage is None:
            done = any(closed(r)[0] for r in range(max_ring + 1))
            stage = FULL if not done else (THREAD_CAP if handed_for_cap else THREAD_RINGS)
        out[i] = stage
    return out


def blocked_rows(p, q, k, block=1024, extra=8):
    """[len(p), k] rows of q nearest to each row of p in ascending (d2, row) order, for clouds too large for knn_rows: every
    (query, candidate) distance is formed block by block on the GPU through torch, one element-wise op at a time; the k + extra
    smallest per query go to the host, where the order is decided in NumPy by the exact (d2, row) and the cut below the
    candidates is checked to be strict."""
    import torch
    qt = torch.from_numpy(q).to("cuda")
    out = np.empty((len(p), k), dtype=np.int64)
    for s in range(0, len(p), block):
        pt = torch.from_numpy(p[s:s + block]).to("cuda")
        d2 = None
        for x in range(3):
            d = pt[:, None, x] - qt[None, :, x]
            d = d * d
            d2 = d if d2 is None else d2 + d
        cand = torch.topk(d2, k + extra, dim=1, largest=False).indices.cpu().numpy()
        cd2 = ref.sq_dist(p[s:s + block, None, :], q[cand])
        order = np.lexsort((cand, cd2), axis=-1)
        cd2 = np.take_along_axis(cd2, order, axis=-1)
        assert np.all(cd2[:, k - 1] < cd2[:, -1])                # nothing outside the candidates can belong to the first k
        out[s:s + block] = np.take_along_axis(cand, order, axis=-1)[:, :k]
    return out
