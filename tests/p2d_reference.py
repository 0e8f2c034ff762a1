"""NumPy restatement of the point-to-distribution metric ("Point-to-distribution"; include/pccm.h,
pccm_p2d_build / PCCM_METRIC_P2D) -- the yardstick of the point-to-distribution tests -- and the clouds those tests run on.

TEST INFRASTRUCTURE.  It does not import the product's kernels.  Every operation is one NumPy element-wise op on fp64 arrays, so
each is rounded separately, as the device's __dadd_rn / __dmul_rn / __dsub_rn / __ddiv_rn / __dsqrt_rn are; the moment sums start
from 0.0 and run left to right over the neighbourhood, one addition per neighbour.  The device's column must therefore equal
mahalanobis() bit for bit.  The neighbourhoods are brute force: every (query, candidate) distance, np.lexsort((rows, d2))."""
import numpy as np

RIDGE = 2.0 ** -10


def sq_dist(p, q):
    """d2 = ((dx*dx) + (dy*dy)) + dz*dz with d = p - q, broadcast over the leading axes."""
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _first_rows(d2, kk):
    """Per row of d2 [m, n]: the kk columns first in ascending (d2, column) order.  Columns beyond the kk-th smallest value
    cannot enter, so the lexsort runs over the others only (padded to the widest row)."""
    m, n = d2.shape
    kth = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
    qi, cj = np.nonzero(d2 <= kth[:, None])                  # row-major: per query, candidate rows ascending
    counts = np.bincount(qi, minlength=m)
    width = int(counts.max())
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    slot = np.arange(len(qi)) - start[qi]
    cand = np.full((m, width), n, dtype=np.int64)            # padding: row n at distance inf, behind everything
    cd2 = np.full((m, width), np.inf)
    cand[qi, slot] = cj
    cd2[qi, slot] = d2[qi, cj]
    order = np.lexsort((cand, cd2), axis=-1)[:, :kk]
    return np.take_along_axis(cand, order, axis=-1)


def knn_rows(a, b, k, chunk=256):
    """[n_a, min(k, n_b)] rows of b: per point of a, the points of b first in ascending (d2, row) order (exact, brute force)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    kk = min(int(k), len(b))
    out = np.empty((len(a), kk), dtype=np.int64)
    for s in range(0, len(a), chunk):
        out[s:s + chunk] = _first_rows(sq_dist(a[s:s + chunk, None, :], b[None, :, :]), kk)
    return out


def moments(a, b, nbr):
    """(m [n, 3], c: the six entries 00 01 02 11 12 22 of the RIDGED covariance [n, 6], t [n]) of each point's neighbourhood."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n, kk = nbr.shape
    s1 = [np.zeros(n) for _ in range(3)]
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    s2 = [np.zeros(n) for _ in pairs]
    for j in range(kk):
        e = b[nbr[:, j]] - a
        for x in range(3):
            s1[x] = s1[x] + e[:, x]
        for i, (x, y) in enumerate(pairs):
            s2[i] = s2[i] + e[:, x] * e[:, y]
    kkf = np.float64(kk)
    m = [s / kkf for s in s1]
    cov = [s2[i] / kkf - m[x] * m[y] for i, (x, y) in enumerate(pairs)]
    t = (cov[0] + cov[3]) + cov[5]
    lam = t * RIDGE
    c = [cov[0] + lam, cov[1], cov[2], cov[3] + lam, cov[4], cov[5] + lam]
    return np.column_stack(m), np.column_stack(c), t


def mahalanobis(a, b, k, nbr=None, return_parts=False):
    """The column of direction a -> b: M(p) for every point p of a against its k nearest points of b."""
    nbr = knn_rows(a, b, k) if nbr is None else np.asarray(nbr, dtype=np.int64)
    m, c, t = moments(a, b, nbr)
    m0, m1, m2 = m.T
    c00, c01, c02, c11, c12, c22 = c.T
    f00 = c11 * c22 - c12 * c12
    f01 = c02 * c12 - c01 * c22
    f02 = c01 * c12 - c02 * c11
    f11 = c00 * c22 - c02 * c02
    f12 = c01 * c02 - c00 * c12
    f22 = c00 * c11 - c01 * c01
    det = (c00 * f00 + c01 * f01) + c02 * f02
    v0 = (f00 * m0 + f01 * m1) + f02 * m2
    v1 = (f01 * m0 + f11 * m1) + f12 * m2
    v2 = (f02 * m0 + f12 * m1) + f22 * m2
    quad = (m0 * v0 + m1 * v1) + m2 * v2
    degenerate = ~(t > 0) | ~(det > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = quad / np.where(degenerate, 1.0, det)
    r = np.where(r > 0, r, 0.0)                              # max(quad / det, 0)
    out = np.sqrt(r)
    at_mean = (m0 == 0) & (m1 == 0) & (m2 == 0)
    out = np.where(degenerate, np.where(at_mean, 0.0, np.inf), out)
    if return_parts:
        return out, m, c, degenerate
    return out


def solved(m, c):
    """sqrt(m^T c^-1 m) by np.linalg.solve on the ridged matrices (the check on the closed form; not bit-pinned)."""
    mat = np.empty((len(m), 3, 3))
    mat[:, 0, 0], mat[:, 0, 1], mat[:, 0, 2] = c[:, 0], c[:, 1], c[:, 2]
    mat[:, 1, 0], mat[:, 1, 1], mat[:, 1, 2] = c[:, 1], c[:, 3], c[:, 4]
    mat[:, 2, 0], mat[:, 2, 1], mat[:, 2, 2] = c[:, 2], c[:, 4], c[:, 5]
    x = np.linalg.solve(mat, m[:, :, None])[:, :, 0]
    return np.sqrt(np.maximum(np.einsum("ni,ni->n", m, x), 0.0))


# ---- the clouds of the tests (plain [n, 3] float64 arrays) ---------------------------------------------------------------------
def uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32).astype(np.float64)


def surface(n, seed, noise=0.01):
    rng = np.random.default_rng(seed)
    uv = rng.random((n, 2))
    z = 0.1 * np.sin(6.0 * uv[:, 0]) * np.cos(4.0 * uv[:, 1]) + rng.normal(0, noise, n)
    return np.column_stack([uv, z]).astype(np.float32).astype(np.float64)


def duplicates(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3), dtype=np.float32).astype(np.float64)
    p = np.concatenate([p, p[rng.integers(0, n, n // 10)]])
    return p[rng.permutation(len(p))]


def lattice(side, count, seed):
    rng = np.random.default_rng(seed)
    p = np.unique(rng.integers(0, side, (count, 3)), axis=0).astype(np.float64)
    return p[rng.permutation(len(p))]


def planes(side, count, seed, z):
    """Points of two parallel integer planes z = z[0], z[1]: neighbourhoods inside one plane have a singular covariance."""
    rng = np.random.default_rng(seed)
    xy = np.unique(rng.integers(0, side, (count, 2)), axis=0)
    p = np.column_stack([xy, np.asarray(z)[rng.integers(0, 2, len(xy))]]).astype(np.float64)
    return p[rng.permutation(len(p))]


def line(n, seed):
    """Points on a straight line (rank-1 covariance)."""
    t = np.random.default_rng(seed).random(n)
    return np.column_stack([t, 2.0 * t, -t]).astype(np.float32).astype(np.float64)


def georeferenced(n, seed):
    """fp64 coordinates that do not survive fp32: a small cloud far from the origin."""
    rng = np.random.default_rng(seed)
    return np.array([4.5e5, 5.4e6, 120.0]) + rng.random((n, 3)) * np.array([40.0, 40.0, 8.0])


def staged(seed, clump=700, isolated=24):
    """(a, b) that send queries down the whole chain of searches.  b: uniform points and a clump of `clump` points inside a ball of
    radius 1e-4 -- more than the wave search stages (kWCap) for every query whose first cubes reach it: the per-thread stage; a:
    uniform points, queries next to the clump, and `isolated` queries far to one side of everything -- further than kKnnMaxRing
    rings of cells from any point of b: the full scan."""
    rng = np.random.default_rng(seed)
    centre = np.array([0.5, 0.5, 0.5])
    ball = rng.normal(0, 1, (clump, 3))
    ball = ball / np.linalg.norm(ball, axis=1)[:, None] * (1e-4 * rng.random((clump, 1)))
    b = np.concatenate([rng.random((5000, 3)), centre + ball])
    near = centre + rng.normal(0, 2e-4, (40, 3))
    far = np.array([0.5, 0.5, 6.0]) + rng.random((isolated, 3)) * 0.05
    a = np.concatenate([rng.random((4000, 3)), near, far])
    return a[rng.permutation(len(a))], b[rng.permutation(len(b))]


FAMILIES = {
    "uniform": lambda: (uniform(3000, 1), uniform(2500, 2)),
    "surface": lambda: (surface(3000, 3), surface(2800, 4)),
    "duplicates": lambda: (duplicates(2500, 5), duplicates(2000, 6)),
    "lattice": lambda: (lattice(14, 2400, 7), lattice(14, 2200, 8)),
    "planes": lambda: (planes(40, 2000, 9, (3, 4)), planes(40, 1800, 10, (3, 5))),
    "georeferenced": lambda: (georeferenced(2400, 11), georeferenced(2000, 12)),
    "b_smaller_than_k": lambda: (uniform(900, 13), uniform(3, 14)),
    "a_large": lambda: (uniform(5000, 15), uniform(1500, 16)),            # A more than twice B: B gets cells of its own
    "b_large": lambda: (uniform(1500, 17), uniform(5000, 18)),            # ... and the reverse
    "overlap": lambda: (uniform(3000, 19), uniform(3000, 20) + np.array([0.75, 0.0, 0.0])),
    "staged": lambda: staged(21),
}
