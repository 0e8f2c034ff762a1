"""NumPy restatement of the F-score rows (CalculateOptions(fscore=...); INTEGRATION.md, "F-score"), for the tests.

A point of one cloud lies within tau of the other cloud when its squared nearest-neighbour distance is <= tau * tau, the product
formed in fp64.  Left (origin -> processed) is the recall, right the precision; the F-score is their harmonic mean, 0 when both
are 0, evaluated in fp64 as ((2 P) R) / (P + R)."""
import numpy as np

RATIO, FSCORE = "GeoInlierRatio", "GeoFScore"


def count_le(column, x) -> int:
    """The number of elements of ``column`` that are <= x (IEEE comparison: 0.0 <= -0.0 holds, NaN is never counted)."""
    return int(np.count_nonzero(np.asarray(column, dtype=np.float64) <= np.float64(x)))


def inlier_ratio(column, tau) -> np.float64:
    t2 = np.float64(tau) * np.float64(tau)
    return np.float64(count_le(column, t2)) / np.float64(len(column))


def fscore(p, r) -> np.float64:
    p, r = np.float64(p), np.float64(r)
    if p + r == 0.0:
        return np.float64(0.0)
    return ((2.0 * p) * r) / (p + r)


def thresholds(taus):
    """The option as the report sees it: distinct floats in ascending order."""
    return tuple(sorted({float(t) + 0.0 for t in taus}))


def keys(taus):
    """The report keys the option adds, in row order."""
    out = []
    for t in thresholds(taus):
        out += [(RATIO, True, t), (RATIO, False, t), (FSCORE, t)]
    return out


def rows(cols_left, cols_right, taus):
    """The expected report rows over the two D1 columns (squared distances), keyed as the report keys them, in row order."""
    out = {}
    for t in thresholds(taus):
        recall, precision = inlier_ratio(cols_left, t), inlier_ratio(cols_right, t)
        out[(RATIO, True, t)] = recall
        out[(RATIO, False, t)] = precision
        out[(FSCORE, t)] = fscore(precision, recall)
    return out
