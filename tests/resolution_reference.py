"""NumPy restatement of the point spacings and the intrinsic resolution (include/pccm.h, pccm_resolution_build; INTEGRATION.md,
"Resolution-adaptive PSNR").

TEST INFRASTRUCTURE.  Brute force: every squared distance of the cloud to itself, d2 = ((dx*dx) + (dy*dy)) + dz*dz in fp64 on the
coordinates as given, np.sort per row, entries 1 .. m - 1 of the m = min(K + 1, n) smallest (entry 0 is the point itself, or a
duplicate of it: distance 0 either way), their square roots summed from 0.0 left to right -- a Python loop over j, one rounded
add per entry -- and one division by m - 1.  The value depends only on the sorted distances, so np.sort (which orders equal
distances arbitrarily) decides nothing."""
import numpy as np


def sq_dist(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def spacings(x, K, block=1024):
    """r[n]: the mean distance of every row of x to its K nearest other rows (all n - 1 of them when n <= K); 0 when n < 2."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    m = min(int(K) + 1, n)
    r = np.zeros(n, dtype=np.float64)
    if m < 2:
        return r
    for s in range(0, n, block):
        d2 = np.sort(sq_dist(x[s:s + block, None, :], x[None, :, :]), axis=1)[:, :m]
        root = np.sqrt(d2)
        total = np.zeros(len(root), dtype=np.float64)
        for j in range(1, m):
            total = total + root[:, j]
        r[s:s + block] = total / np.float64(m - 1)
    return r


def resolution(x, K):
    """R: np.sum(r) / n, NumPy's pairwise sum."""
    r = spacings(x, K)
    return np.sum(r) / len(r)


def psnr(peak, distortion):
    return 10 * np.log10(peak ** 2 / distortion)
