"""NumPy restatement of the reflectance rows (include/pccm.h, PCCM_METRIC_REFLECTANCE; INTEGRATION.md, "Reflectance") -- the
yardstick of the reflectance tests.

Per row ``i`` of the iterating cloud ``a``: ``nn(i)`` = the exact nearest row of the searched cloud ``b``, the smallest row on ties
(tests/nn_reference.py), ``d = ra[i] - rb[nn(i)]`` and ``d * d`` in fp64 on the values as given.  NumPy's element-wise subtract
and power round each operation on its own, as the kernel's two instructions do.  Rows: ``np.sum(col) / n``, ``np.max(col)`` and
``_psnr`` of metric.py against the peak; the symmetric rows follow metric.py's SymmetricMetric like every other symmetric row of
the report: the sides are compared by ``np.linalg.norm`` -- for a scalar its absolute value --, an error row takes the side with
the larger key and a PSNR row the one with the smaller, the left one on ties.  ``merged`` restates the duplicate rule of
pccm_merge_duplicates for a scalar column over the groups of tests/merge_reference.py."""
import numpy as np

from merge_reference import groups
from nn_reference import nn_brute

DEFAULT_PEAK = 65535.0


def column(a, b, ra, rb):
    """-> the per-point column of the direction that iterates ``a`` and searches ``b``."""
    nn, _ = nn_brute(a, b)
    return (np.asarray(ra).astype(np.float64) - np.asarray(rb).astype(np.float64)[nn]) ** 2


def _psnr(peak, distortion):
    with np.errstate(divide="ignore"):
        return 10 * np.log10(np.float64(peak) ** 2 / np.float64(distortion))


def rows(a, b, ra, rb, *, hausdorff=False, peak=DEFAULT_PEAK):
    """-> {as_dict key: value} of every reflectance row of the report, in report order."""
    peak = float(peak)
    cols = {True: column(a, b, ra, rb), False: column(b, a, rb, ra)}
    out = {}

    def block(err_name, psnr_name, reduce):
        err = {side: reduce(cols[side]) for side in (True, False)}
        psnr = {side: _psnr(peak, err[side]) for side in (True, False)}
        for side in (True, False):
            out[(err_name, side)] = err[side]
        out[("SymmetricMetric", err_name, True, err_name, False)] = err[False] if abs(err[False]) > abs(err[True]) else err[True]
        for side in (True, False):
            out[(psnr_name, side, peak)] = psnr[side]
        out[("SymmetricMetric", psnr_name, True, peak, psnr_name, False, peak)] = \
            psnr[False] if abs(psnr[False]) < abs(psnr[True]) else psnr[True]

    block("ReflectanceMSE", "ReflectancePSNR", lambda c: np.sum(c) / c.shape[0])
    if hausdorff:
        block("ReflectanceHausdorffDistance", "ReflectanceHausdorffDistancePSNR", np.max)
    return out


def _merged(x, r, mode, reverse):
    if mode not in ("drop", "average"):
        raise ValueError(mode)
    r = np.asarray(r).astype(np.float64)
    mapping, reps = groups(x)
    out = r[reps].copy()
    if mode == "average":
        members = [[] for _ in reps]
        for i, g in enumerate(mapping.tolist()):                       # ascending rows
            members[g].append(i)
        for g, grp in enumerate(members):
            if len(grp) == 1:
                continue                                               # (m = 1: the input bits)
            grp = grp[::-1] if reverse else grp
            s = float(r[grp[0]])
            for i in grp[1:]:
                s = s + float(r[i])
            out[g] = s / float(len(grp))
    return out


def merged(x, r, mode):
    """-> the reflectance column of the merged cloud: "drop" the representative's value, "average" the group's values summed in
    ascending row order, every add rounded, then one division by the count."""
    return _merged(x, r, mode, False)


def merged_descending(x, r, mode):
    """The same with every group summed in DESCENDING row order: what a kernel that ignored the order could produce."""
    return _merged(x, r, mode, True)


def merged_points(x):
    """-> the merged cloud's points (the representatives' rows, ascending)."""
    _, reps = groups(x)
    return np.asarray(x).astype(np.float64)[reps].copy()
