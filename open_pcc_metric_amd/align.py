"""Rigid registration of the processed cloud onto the original, on the GPU (``CloudPair(transform=..., align="icp")``).

Two things move cloud 1 before the pair searches, estimates normals and reports: an explicit rigid ``transform`` the caller already
knows, and point-to-point ICP.  Both act on the RESIDENT cloud (pccm_transform_cloud): no file is written, nothing is uploaded again,
and file normals of the cloud are rotated with it.  The original cloud never moves.

ICP, per iteration: one exact nearest-neighbour search of direction RIGHT (cloud 1 in cloud 0, ties to the smallest row), the
inlier count ``m = #(d2 <= tau2)`` (pccm_count_many), sixteen sums over the inliers relative to the pivot ``c``, the centre of the
original's bounding box (pccm_reduce_moment_total_many, two calls of eight): ``sp = sum p - c``, ``sq = sum q - c``,
``S[a][b] = sum (p - c)_a (q - c)_b`` and ``sum d2``, p a point of cloud 1 and q its match.  Every one of them equals ``np.sum`` bit
for bit, so the loop below is reproducible on any host from the same numbers.  The Kabsch step is 3 x 3 and runs on the host.
The stopping rule is Open3D's ``registration_icp`` default (relative fitness and relative RMSE both below the tolerance).

Out of scope: scale estimation, point-to-plane ICP, global registration without an initial pose, moving cloud 0, sharded pairs,
matching under ``ties="mean"`` (alignment always matches under "pick"; the pair's policy applies to the report afterwards).
"""
import math
import typing

import numpy as np

from . import _native as nat

ALIGN_METHODS = ("icp",)
MAX_ALIGN_ITERATIONS = 1000
RIGID_TOLERANCE = 1e-9          # max |A^T A - I| of a transform= that counts as a rotation


class Alignment(typing.NamedTuple):
    """What moved cloud 1 (``pair.alignment``).  ``transformation``: the 4 x 4 matrix applied to the given cloud in all -- an explicit
    ``transform`` included; ``iterations``: searches ICP ran (0: no ICP); ``fitness``: inliers / points of cloud 1 and
    ``inlier_rmse``: their root mean squared distance, both at the last search (None without ICP); ``converged``: the stopping rule
    was met before ``align_iterations`` ran out."""
    transformation: np.ndarray
    iterations: int
    fitness: typing.Optional[float]
    inlier_rmse: typing.Optional[float]
    converged: bool


def check_transform(transform) -> typing.Optional[np.ndarray]:
    """``transform=`` as a 4 x 4 float64 matrix, or None; ValueError unless it is rigid: a 3 x 4 or 4 x 4 array of finite numbers,
    ``max |A^T A - I| <= 1e-9``, ``det A > 0`` and, where given, the last row ``0 0 0 1``."""
    if transform is None:
        return None
    try:
        m = np.array(transform, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("transform: a 4 x 4 or 3 x 4 array of numbers expected") from None
    if m.shape not in ((3, 4), (4, 4)):
        raise ValueError(f"transform: a 4 x 4 or 3 x 4 array expected, not shape {m.shape}")
    if not np.all(np.isfinite(m)):
        raise ValueError("transform: every entry must be finite")
    if m.shape == (4, 4) and not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError("transform: the last row of a 4 x 4 matrix must be 0 0 0 1")
    a = m[:3, :3]
    if not np.max(np.abs(a.T @ a - np.eye(3))) <= RIGID_TOLERANCE:
        raise ValueError("transform: only rigid motions are supported (the 3 x 3 block is not orthogonal to 1e-9)")
    if not np.linalg.det(a) > 0.0:
        raise ValueError("transform: only rigid motions are supported (the 3 x 3 block is a reflection)")
    out = np.eye(4)
    out[:3, :] = m[:3, :]
    return out


def check_align(align, align_distance=None, align_iterations=30, align_tolerance=1e-6, *, transform=None, group=None):
    """Validate the alignment settings before any GPU work -> ``(transform 4 x 4 or None, align, tau2, iterations, tolerance)``;
    ValueError otherwise."""
    t = check_transform(transform)
    if align is not None and (not isinstance(align, str) or align not in ALIGN_METHODS):
        raise ValueError('align must be None or "icp"')
    if align_distance is not None:
        if isinstance(align_distance, bool) or not isinstance(align_distance, (int, float, np.integer, np.floating)):
            raise ValueError("align_distance must be None or a finite number > 0")
        if not (math.isfinite(float(align_distance)) and float(align_distance) > 0.0):
            raise ValueError("align_distance must be None or a finite number > 0")
    if isinstance(align_iterations, bool) or not isinstance(align_iterations, (int, np.integer)) \
            or not 1 <= int(align_iterations) <= MAX_ALIGN_ITERATIONS:
        raise ValueError(f"align_iterations must be an integer in 1..{MAX_ALIGN_ITERATIONS}")
    if isinstance(align_tolerance, bool) or not isinstance(align_tolerance, (int, float, np.integer, np.floating)) \
            or not (math.isfinite(float(align_tolerance)) and float(align_tolerance) >= 0.0):
        raise ValueError("align_tolerance must be a finite number >= 0")
    if (t is not None or align is not None) and group is not None:
        raise ValueError("transform= and align= are not available for sharded pairs (group=)")
    tau2 = math.inf if align_distance is None else float(np.float64(align_distance) * np.float64(align_distance))
    return t, align, tau2, int(align_iterations), float(align_tolerance)


def read_transform_file(path) -> np.ndarray:
    """``--transform FILE``: 12 or 16 whitespace-separated numbers, row-major -> a checked 4 x 4 matrix (ValueError otherwise)."""
    with open(path, "r") as f:
        words = f.read().split()
    try:
        values = [float(w) for w in words]
    except ValueError:
        raise ValueError(f"{path}: not a number among the entries") from None
    if len(values) not in (12, 16):
        raise ValueError(f"{path}: 12 or 16 numbers expected, found {len(values)}")
    return check_transform(np.array(values, dtype=np.float64).reshape(-1, 4))


def write_transform_file(path, matrix) -> None:
    """``--align-out FILE``: the 4 x 4 matrix, one row per line, 17 significant digits (every float64 survives the round trip)."""
    with open(path, "w") as f:
        for row in np.asarray(matrix, dtype=np.float64).reshape(-1, 4):       # (a list of matrices: one after the other)
            f.write(" ".join("%.17g" % v for v in row) + "\n")


def bounding_box_centre(points) -> np.ndarray:
    """The pivot of the moments: the centre of the cloud's bounding box, ``(min + max) / 2`` per axis in fp64."""
    p = np.asarray(points)
    return centre_of(np.min(p, axis=0), np.max(p, axis=0))


def centre_of(lo, hi) -> np.ndarray:
    return (np.asarray(lo, dtype=np.float64) + np.asarray(hi, dtype=np.float64)) / 2.0


def kabsch_step(sums, m: int, c: np.ndarray):
    """The rigid motion ``(R, t)`` that best maps the inliers of cloud 1 onto their matches, from the sixteen moment sums
    (kinds 0..15, relative to the pivot ``c``) over ``m`` inliers."""
    s = np.asarray(sums, dtype=np.float64)
    sp, sq, big = s[0:3], s[3:6], s[6:15].reshape(3, 3)
    h = np.empty((3, 3))
    for a in range(3):
        for b in range(3):
            h[a][b] = big[a][b] - sp[a] * sq[b] / m
    u, _s, vt = np.linalg.svd(h)
    d = np.sign(np.linalg.det(vt.T @ u.T))
    r = vt.T @ np.diag([1.0, 1.0, d]) @ u.T
    t = (sq / m + c) - r @ (sp / m + c)
    return r, t


def _moment_sums(eng, tau2: float, c) -> list:
    requests = [(nat.DIR_RIGHT, kind, tau2) for kind in range(nat.MOMENT_KINDS)]
    out = eng.reduce_moment_total_many(requests[:8], c) + eng.reduce_moment_total_many(requests[8:], c)
    return [float(v[0]) for v in out]


def icp(eng, n1: int, c, tau2: float, iterations: int, tolerance: float, nn_engine: str = "auto", start=None) -> Alignment:
    """Point-to-point ICP of resident cloud 1 onto resident cloud 0 on engine ``eng`` (module docstring).  ``start``: the 4 x 4
    motion cloud 1 has already been given, which the result's ``transformation`` continues.  ValueError when fewer than three
    points of cloud 1 lie within the distance."""
    total = np.eye(4) if start is None else np.array(start, dtype=np.float64)
    prev = None
    k = 0
    while True:
        k += 1
        eng.nn(nat.DIR_RIGHT, nn_engine)
        m = int(eng.count_many([(nat.DIR_RIGHT, nat.METRIC_D1, tau2)])[0])
        if m < 3:
            raise ValueError(f"align: only {m} of the processed cloud's points lie within align_distance of the original "
                             "(a rigid motion needs three): the clouds need a better initial pose (transform=) or a larger distance")
        sums = _moment_sums(eng, tau2, c)
        fitness = m / n1
        rmse = math.sqrt(sums[15] / m)
        if prev is not None and abs(fitness - prev[0]) < tolerance and abs(rmse - prev[1]) < tolerance:
            return Alignment(total, k, fitness, rmse, True)
        if k >= iterations:
            return Alignment(total, k, fitness, rmse, False)
        prev = (fitness, rmse)
        r, t = kabsch_step(sums, m, np.asarray(c, dtype=np.float64))
        step = np.eye(4)
        step[:3, :3] = r
        step[:3, 3] = t
        eng.transform_cloud(1, step)
        total = step @ total
