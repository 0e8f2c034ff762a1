"""NumPy restatement of the ranked (generalized) Hausdorff rows ("Ranked Hausdorff"): the nearest-rank index
of a rank r in (0, 1] over n points, and the k-th smallest element of a column.  Nothing here imports the package."""
import fractions
import math

import numpy as np


def rank_index(r, n):
    """k = max(1, ceil(R * n)), R the decimal number repr(float(r)) spells, taken as an exact fraction."""
    big_r = fractions.Fraction(repr(float(r)))
    return max(1, math.ceil(big_r * int(n)))


def ranked(col, r):
    """The rank_index(r, len(col))-th smallest element of col (1-based; equal elements count separately)."""
    col = np.asarray(col, dtype=np.float64)
    k = rank_index(r, col.shape[0])
    return np.partition(col, k - 1)[k - 1]


def ranked_psnr(peak, value):
    """GeoHausdorffDistancePSNR's expression (metric.py:384-386) with the ranked value."""
    return 10 * np.log10(peak ** 2 / value)
