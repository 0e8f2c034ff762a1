"""NumPy restatement of the alignment feature (``CloudPair(transform=..., align="icp")``; INTEGRATION.md, "Alignment"), for the
tests: the move of a cloud, the sixteen alignment moments and the ICP loop, over the oracle's exact nearest-neighbour search.
Written from the feature's definition, not from the product's align.py.  Every operation is the fp64 NumPy one, in this order.

Move, per row (x, y, z) of the cloud and the row-major 3 x 4 matrix [A | t]:

    x' = ((a00 * x + a01 * y) + a02 * z) + t0          likewise y', z'
    n' = (a00 * nx + a01 * ny) + a02 * nz              per component of a normal, no translation

Moments of a direction, for row i, its matched row j (ties: the smallest row), d2 its D1 value, w = (d2 <= cap) and a pivot c:

    u_a = x_it[i][a] - c[a]        v_b = x_se[j][b] - c[b]
    kind 0..2: where(w, u_a, 0.0)    3..5: where(w, v_b, 0.0)    6 + 3 a + b: where(w, u_a * v_b, 0.0)    15: where(w, d2, 0.0)

ICP (c: the centre of the original's bounding box; tau2 = align_distance ** 2 or +inf), for k = 1, 2, ...: search cloud 1 in cloud
0; m = count(d2 <= tau2) (fewer than 3: ValueError); fitness = m / n1, rmse = sqrt(S15 / m); stop converged when k > 1 and both
moved by less than the tolerance, stop unconverged when k reached the iterations; H[a][b] = S[a][b] - sp[a] * sq[b] / m;
U, s, Vt = svd(H); R = Vt.T diag(1, 1, sign(det(Vt.T U.T))) U.T; t = (sq / m + c) - R (sp / m + c); move cloud 1 by [R | t] and
compose T <- [R | t] T."""
import math

import numpy as np

from oracle import oracle as orc

KINDS = 16


def move_points(x, m):
    x = np.asarray(x, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)[:3, :4]
    out = np.empty_like(x)
    for a in range(3):
        out[:, a] = ((m[a, 0] * x[:, 0] + m[a, 1] * x[:, 1]) + m[a, 2] * x[:, 2]) + m[a, 3]
    return out


def move_normals(n, m):
    n = np.asarray(n, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)[:3, :4]
    out = np.empty_like(n)
    for a in range(3):
        out[:, a] = (m[a, 0] * n[:, 0] + m[a, 1] * n[:, 1]) + m[a, 2] * n[:, 2]
    return out


def moment_column(kind, x_it, x_se, idx, d2, cap, pivot):
    """The term column of one kind (module docstring)."""
    x_it, x_se = np.asarray(x_it, dtype=np.float64), np.asarray(x_se, dtype=np.float64)
    idx, d2 = np.asarray(idx), np.asarray(d2, dtype=np.float64)
    c = np.asarray(pivot, dtype=np.float64)
    w = d2 <= np.float64(cap)
    if kind < 3:
        term = x_it[:, kind] - c[kind]
    elif kind < 6:
        term = x_se[idx, kind - 3] - c[kind - 3]
    elif kind < 15:
        a, b = divmod(kind - 6, 3)
        term = (x_it[:, a] - c[a]) * (x_se[idx, b] - c[b])
    else:
        term = d2
    return np.where(w, term, 0.0)


def moment_totals(kind, x_it, x_se, idx, d2, cap, pivot):
    """(np.sum, np.min, np.max) of the term column: what pccm_reduce_moment_total_many answers."""
    t = moment_column(kind, x_it, x_se, idx, d2, cap, pivot)
    return np.sum(t), ordered_min(t), ordered_max(t)


# np.min / np.max compare -0.0 and 0.0 equal, so which of the two they answer for a column that holds both depends on where the
# values stand (and on the width of NumPy's vector loop): not a function of the column's values.  A product column holds both as
# soon as a point has a coordinate of the pivot.  The device orders them, -0.0 below 0.0 (fmin / fmax, as for the signed
# projection columns); the reference states the same order explicitly and is compared on bits like everything else.
def ordered_min(t):
    m = np.min(t)
    return np.float64(-0.0) if m == 0 and np.any(np.signbit(t[t == 0])) else m


def ordered_max(t):
    m = np.max(t)
    if m != 0:
        return m
    return np.float64(0.0) if np.any(~np.signbit(t[t == 0])) else np.float64(-0.0)


def box_centre(points):
    p = np.asarray(points, dtype=np.float64)
    return (np.min(p, axis=0) + np.max(p, axis=0)) / 2.0


def icp(origin, processed, align_distance=None, iterations=30, tolerance=1e-6, start=None, trace=None, steps=None):
    """-> dict(transformation, iterations, fitness, inlier_rmse, converged, points): the loop of the module docstring.  ``start``:
    a 4 x 4 motion applied first (``transform=``).  ``trace``: a list that receives the matched rows of every search; ``steps``: one that
    receives every motion [R | t] applied."""
    p0 = np.ascontiguousarray(np.asarray(origin, dtype=np.float64))
    p1 = np.ascontiguousarray(np.asarray(processed, dtype=np.float64))
    total = np.eye(4)
    if start is not None:
        total = np.array(start, dtype=np.float64)
        p1 = move_points(p1, total)
    c = box_centre(p0)
    tau2 = math.inf if align_distance is None else float(np.float64(align_distance) * np.float64(align_distance))
    n1 = len(p1)
    prev = None
    k = 0
    while True:
        k += 1
        idx, d2 = orc.nn(p1, p0)
        if trace is not None:
            trace.append(np.asarray(idx).copy())
        m = int(np.count_nonzero(d2 <= tau2))
        if m < 3:
            raise ValueError("fewer than three inliers")
        s = [np.sum(moment_column(kind, p1, p0, idx, d2, tau2, c)) for kind in range(KINDS)]
        fitness = m / n1
        rmse = math.sqrt(s[15] / m)
        if k > 1 and abs(fitness - prev[0]) < tolerance and abs(rmse - prev[1]) < tolerance:
            converged = True
            break
        if k >= iterations:
            converged = False
            break
        prev = (fitness, rmse)
        sp, sq = np.array(s[0:3]), np.array(s[3:6])
        big = np.array(s[6:15]).reshape(3, 3)
        h = np.empty((3, 3))
        for a in range(3):
            for b in range(3):
                h[a][b] = big[a][b] - sp[a] * sq[b] / m
        u, _, vt = np.linalg.svd(h)
        r = vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(vt.T @ u.T))]) @ u.T
        t = (sq / m + c) - r @ (sp / m + c)
        step = np.eye(4)
        step[:3, :3] = r
        step[:3, 3] = t
        if steps is not None:
            steps.append(step)
        p1 = move_points(p1, step)
        total = step @ total
    return dict(transformation=total, iterations=k, fitness=fitness, inlier_rmse=rmse, converged=converged, points=p1)


# ---- planted cases ------------------------------------------------------------------------------------------------------------
def rotation(axis, degrees):
    """Rodrigues' formula."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.sqrt(np.sum(a * a))
    th = math.radians(degrees)
    kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(th) * kx + (1.0 - math.cos(th)) * (kx @ kx)


def rigid(axis, degrees, shift):
    m = np.eye(4)
    m[:3, :3] = rotation(axis, degrees)
    m[:3, 3] = shift
    return m


def lattice(seed=0, side=10, jitter=0.2):
    """A side^3 lattice of spacing 1 with every coordinate jittered by +-jitter."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float64)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return g + rng.uniform(-jitter, jitter, size=g.shape)


def planted_pair(degrees, seed=0, shift=(0.1, -0.05, 0.08)):
    """-> (origin, processed, planted 4 x 4, perm): processed[i] is origin[perm[i]] moved by ``degrees`` about (1, 2, 3) and ``shift``."""
    origin = lattice(seed)
    planted = rigid((1.0, 2.0, 3.0), degrees, shift)
    perm = np.random.default_rng(seed + 1000).permutation(len(origin))
    processed = move_points(origin, planted)[perm]
    return origin, np.ascontiguousarray(processed), planted, perm


def partial_pair(degrees=3.0, seed=0):
    """Partly overlapping clouds: the lattice's rows with x < 6.5 against its rows with x > 2.5 moved by ``degrees``."""
    full = lattice(seed)
    planted = rigid((1.0, 2.0, 3.0), degrees, (0.05, 0.02, -0.04))
    origin = np.ascontiguousarray(full[full[:, 0] < 6.5])
    processed = np.ascontiguousarray(move_points(full[full[:, 0] > 2.5], planted))
    return origin, processed, planted
