"""NumPy restatement of the Chamfer and truncated-distance rows (CalculateOptions(chamfer=..., truncate=...); INTEGRATION.md,
"Chamfer and truncated distances"), for the tests.

``v`` is a direction's D1 column (squared nearest-neighbour distances) or D2 column (squared projections), ``n`` its length; every
operation is the fp64 NumPy one, in this order:

    GeoMeanDistance            = np.sum(np.sqrt(v)) / n
    GeoChamferL1               = (L + R) / np.float64(2)          # D1 sides: PCN's convention
    GeoChamferL2               = GeoMSE_L + GeoMSE_R              # D1 sides
    t2                         = np.float64(tau) * np.float64(tau)
    GeoTruncatedMSE[tau]       = np.sum(np.minimum(v, t2)) / n
    GeoTruncatedMeanDistance   = np.sum(np.sqrt(np.minimum(v, t2))) / n

The symmetric rows report the larger side, the left one when they are equal."""
import numpy as np

MEAN, L1, L2, TMSE, TMEAN = "GeoMeanDistance", "GeoChamferL1", "GeoChamferL2", "GeoTruncatedMSE", "GeoTruncatedMeanDistance"
CLAMP, ROOT = 1, 2          # PCCM_MAP_CLAMP, PCCM_MAP_ROOT


def mapped(column, which: int, x=None):
    """f(column) for the map ``which``: the clamp at ``x`` first, then the root."""
    f = np.asarray(column, dtype=np.float64)
    if which & CLAMP:
        f = np.minimum(f, np.float64(x))
    if which & ROOT:
        f = np.sqrt(f)
    return f


def totals(column, which: int, x=None):
    """(np.sum, np.min, np.max) of f(column): what pccm_reduce_map_total_many answers."""
    f = mapped(column, which, x)
    return np.sum(f), np.min(f), np.max(f)


def cap(tau) -> np.float64:
    return np.float64(tau) * np.float64(tau)


def mse(v) -> np.float64:
    return np.sum(np.asarray(v, dtype=np.float64)) / len(v)


def mean_distance(v) -> np.float64:
    return np.sum(mapped(v, ROOT)) / len(v)


def truncated_mse(v, tau) -> np.float64:
    return np.sum(mapped(v, CLAMP, cap(tau))) / len(v)


def truncated_mean_distance(v, tau) -> np.float64:
    return np.sum(mapped(v, CLAMP | ROOT, cap(tau))) / len(v)


def thresholds(taus):
    """The option as the report sees it: distinct floats in ascending order."""
    return tuple(sorted({float(t) + 0.0 for t in (taus or ())}))


def _larger(left, right):
    return right if right > left else left


def _sym(inner, *args):
    return ("SymmetricMetric", inner, True) + args + (inner, False) + args


def rows(left, right, chamfer=True, taus=(), left_d2=None, right_d2=None):
    """The expected report rows over the two D1 columns (and, with point_to_plane, the two D2 columns), keyed as the report keys
    them, in row order."""
    out = {}
    if chamfer:
        for p2p, (a, b) in ((False, (left, right)), (True, (left_d2, right_d2))):
            if a is None:
                continue
            va, vb = mean_distance(a), mean_distance(b)
            out[(MEAN, True, p2p)] = va
            out[(MEAN, False, p2p)] = vb
            out[_sym(MEAN, p2p)] = _larger(va, vb)
        out[(L1,)] = (mean_distance(left) + mean_distance(right)) / np.float64(2)
        out[(L2,)] = mse(left) + mse(right)
    for t in thresholds(taus):
        for name, fn in ((TMSE, truncated_mse), (TMEAN, truncated_mean_distance)) if chamfer else ((TMSE, truncated_mse),):
            va, vb = fn(left, t), fn(right, t)
            out[(name, True, t)] = va
            out[(name, False, t)] = vb
            out[_sym(name, t)] = _larger(va, vb)
    return out
