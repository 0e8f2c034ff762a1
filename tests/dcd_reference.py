"""NumPy restatement of the density-aware Chamfer rows (CalculateOptions(dcd=..., dcd_squared=...); INTEGRATION.md, "Density-aware
Chamfer distance"), for the tests.

``d2`` is a direction's D1 column (squared nearest-neighbour distances), ``idx`` its matched rows (ties: the smallest row), ``n`` its
length and ``n_searched`` the rows of the searched cloud; every operation is the fp64 NumPy one, in this order:

    m                          = np.bincount(idx, minlength=n_searched)
    s                          = d2 if squared else np.sqrt(d2)
    t                          = 1.0 - np.exp(-alpha * s) / m[idx].astype(np.float64)
    GeoDensityAwareDistance    = np.sum(t) / n
    GeoDensityAwareChamfer     = (L + R) / np.float64(2)

Every operation but ``exp`` is correctly rounded here and on the device, so alpha = 0 (exp(-0.0 * s) == 1.0) and alpha = 1e300
(exp == 0.0 where s > 0, 1.0 where s == 0) compare on bits, and any other alpha to within what two exp implementations differ by
(ATOL)."""
import numpy as np

SIDE, BOTH = "GeoDensityAwareDistance", "GeoDensityAwareChamfer"

# The only inexact comparison.  The terms lie in [0, 1] and the two sides differ only through exp: the device's fp64 exp and
# NumPy's are each documented to about 1 ulp, a difference of k ulps of a value <= 1 per term moves the mean by at most
# k * 2^-53, and the two roundings of the identical summation tree add at most 2 * (20 + log2 n) * 2^-53 -- about 8e-15 at
# n = 1e5.  2^-40 (9e-13) is two orders above that bound and far below what one wrong count does at the alphas the tests
# choose (about 0.37 * |1/m - 1/m'| / n >= 1e-7).
ATOL = 2.0 ** -40


def counts(idx, n_searched) -> np.ndarray:
    return np.bincount(np.asarray(idx), minlength=int(n_searched)).astype(np.uint32)


def terms(d2, idx, n_searched, alpha, squared=False) -> np.ndarray:
    d2 = np.asarray(d2, dtype=np.float64)
    idx = np.asarray(idx)
    m = counts(idx, n_searched)
    s = d2 if squared else np.sqrt(d2)
    return 1.0 - np.exp(-np.float64(alpha) * s) / m[idx].astype(np.float64)


def totals(d2, idx, n_searched, alpha, squared=False):
    """(np.sum, np.min, np.max) of the terms: what pccm_reduce_density_total_many answers."""
    t = terms(d2, idx, n_searched, alpha, squared)
    return np.sum(t), np.min(t), np.max(t)


def side(d2, idx, n_searched, alpha, squared=False) -> np.float64:
    return np.sum(terms(d2, idx, n_searched, alpha, squared)) / len(d2)


def huge_alpha_side(d2, idx, n_searched) -> np.float64:
    """The row at alpha = 1e300 without any exp: 1 where the distance is positive, 1 - 1 / m where it is zero."""
    d2 = np.asarray(d2, dtype=np.float64)
    m = counts(idx, n_searched)
    return np.sum(np.where(d2 > 0, 1.0, 1.0 - 1.0 / m[np.asarray(idx)].astype(np.float64))) / len(d2)


def alphas_of(values):
    """The option as the report sees it: distinct floats in ascending order."""
    return tuple(sorted({float(a) + 0.0 for a in (values or ())}))


def rows(left_d2, right_d2, left_idx, right_idx, n0, n1, alphas, squared=False):
    """The expected report rows, keyed as the report keys them, in row order.  Left iterates cloud 0 (n0 rows) and searches
    cloud 1 (n1 rows); right the other way round."""
    squared = bool(squared)
    out = {}
    for a in alphas_of(alphas):
        va = side(left_d2, left_idx, n1, a, squared)
        vb = side(right_d2, right_idx, n0, a, squared)
        out[(SIDE, True, a, squared)] = va
        out[(SIDE, False, a, squared)] = vb
        out[(BOTH, a, squared)] = (va + vb) / np.float64(2)
    return out
