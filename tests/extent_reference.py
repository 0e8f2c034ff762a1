"""References, tolerances, inputs and kernel models for the three extent kernels of csrc/pccm_obb.hip
(k_obb_frames, k_extreme_rows, k_outside_planes behind pccm_obb_frames, pccm_extreme_rows, pccm_rows_outside).
Standard library and NumPy only.  tests/test_extent_reference_host.py holds this module to itself and to the oracle's NumPy
restatements without a GPU; tests/test_gpu_extent_kernels.py holds the kernels to it, through the same check_* helpers.

Frame reference (frame_reference)
---------------------------------
One triangle (a, b, c) and a vertex set.  Every fp64 input is a rational number; with ``fractions.Fraction`` the edge vectors
u = b - a, v0 = c - a, both cross products w = u x v0, v = w x u and every projection n_r.(x_j - a) on the UNNORMALISED axes
n_r = (u, v, w) are exact, and so are their maximum and minimum over the vertices.  What is left is one division per axis,
ext_r = (max - min) / |n_r|, taken with ``decimal`` at 50 digits.  hull_reference() is the same arithmetic for every triangle
of a hull, on integers (all inputs times one power of two -- Fractions with their common denominator taken out) and with the
exact evaluation restricted to the vertices whose fp64 projection on the correctly rounded exact axis lies within 2^-30 D of
the fp64 extreme: that projection is off by less than 2^-49 D, so no extreme vertex is screened out.

tau_frame: the tolerance on one extent, derived, not measured
-------------------------------------------------------------
eps = 2^-53 (unit roundoff of fp64), D = max_j |x_j - a|, sin = |u x v0| / (|u| |v0|).  First order in eps; an FMA contraction
removes roundings and never adds one.  All bounds are on Euclidean norms.
  * u^ = fl(b - a), v0^ = fl(c - a): |du| <= eps |u|, |dv0| <= eps |v0|.
  * w^ = fl(u^ x v0^): every component is two products and a subtraction, error <= 2 eps (|u_i v_j| + |u_j v_i|); the vector of
    these sums has norm <= sqrt(2) |u| |v0|.  With the inherited 2 eps |u| |v0|: |dw| <= (2 + 2 sqrt 2) eps |u| |v0|
    = 4.83 eps |w| / sin.
  * v^ = fl(w^ x u^), |v| = |w| |u|: |dv| <= |dw| |u| + |w| |du| + 2 sqrt(2) eps |w| |u| = (3.83 + 4.83 / sin) eps |v|.
  * normalising a row n^: the sum of three squares carries 3 eps, its root 1.5 eps + eps, the division eps: 3.5 eps.
  * one projection: d = fl(x - a) carries eps D, the three-term dot product 3 eps D.  So |l^ - l| <= e_r eps D with
    e_0 = 2 + 3.5 + 1 + 3 = 9.5  (du counted once for the direction and once for the length of the row),
    e_1 = 3.83 + 3.5 + 1 + 3 + 4.83 / sin = 11.33 + 4.83 / sin,      e_2 = 3.5 + 1 + 3 + 4.83 / sin = 7.5 + 4.83 / sin.
  * an extent is hi - lo: both ends, plus the rounding of the subtraction, eps (hi - lo) <= eps 2 D.
Hence |ext^_r - ext_r| <= 2 D eps (e_r + 1), and with the constants rounded up
        tau_frame_r = 2 D eps (c0_r + c1_r / sin),    (c0, c1) = (11, 0), (13, 5), (9, 5)  for the rows u, v, w.
The volume is the product of the three extents in two more roundings: tau_volume = prod(ext_r + tau_r) (1 + 2 eps) - prod ext_r.
The minimum over frames then lies in [min_t (vol_t - tauv_t), min_t (vol_t + tauv_t)].

tau_extreme: k_extreme_rows chooses "about the farthest" point in fp32
----------------------------------------------------------------------
Reference: the fp64 maximum of p_i.d_k.  The returned row r_k must reach it within tau_k = 6 * 2^-24 |d_k| max_i |p_i|: the cast
of the point, three products and two additions are at most 3 * 2^-24 |d_k| |p_i| on one dot product, and the comparison has two
sides.  A point that leads by more than tau_k in fp64 is therefore THE answer: planted_cloud() puts such points ("spikes" R d_k
in a bulk of radius <= R / 2) at chosen rows and asserts twice that margin for the directions it is given.

Exact data for k_outside_planes (outside_case)
----------------------------------------------
Integer coordinates below 2^20, plane coefficients that are integers over 8, a margin that is a multiple of 1/8: every product
and partial sum of n.x + off is a multiple of 1/8 below 2^40, exact in fp64 in any order and under any contraction, so the
expected rows are integer arithmetic and the comparison is set equality.

Models
------
model_obb_frames, model_extreme_rows, model_rows_outside restate the tile walks, the thread-to-data maps, the fp32 key and
the host's argmin in NumPy, each with one switchable defect (DEFECTS).  The host test shows that the check_* helpers, on the
inputs of the GPU tests, catch every one.
"""
import decimal
import functools
import math
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -53
C0 = np.array([11.0, 13.0, 9.0])
C1 = np.array([0.0, 5.0, 5.0])
_DEC = decimal.Context(prec=50)
_D = decimal.Decimal


def _prec50(fn):
    """Run fn with 50-digit Decimal arithmetic, whatever the caller's context is."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        with decimal.localcontext(_DEC):
            return fn(*args, **kwargs)
    return wrapped


# ---- exact frames -------------------------------------------------------------------------------------------------
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _axes(a, b, c):
    u = [b[k] - a[k] for k in range(3)]
    v0 = [c[k] - a[k] for k in range(3)]
    w = _cross(u, v0)
    return u, _cross(w, u), w, v0


def _dec(q):
    q = Fraction(q)
    return _DEC.divide(_D(q.numerator), _D(q.denominator))


class FrameRef:
    """ext: three Decimals (None for a degenerate triangle), vol: Decimal (Infinity), sin: float, proj: the exact projections
    on the unit axes as Decimals [3][nv] (frame_reference only)."""

    def __init__(self, ext, sin, proj=None):
        self.ext, self.sin, self.proj = ext, sin, proj
        self.vol = _D("Infinity") if ext is None else _DEC.multiply(_DEC.multiply(ext[0], ext[1]), ext[2])

    @property
    def ext64(self):
        return None if self.ext is None else np.array([float(e) for e in self.ext])


def _finish(rng, nsq, scale):
    """(max - min) of the exact projections over |n|, per axis: exact numerators, one 50-digit division each."""
    return [_DEC.divide(_dec(rng[r]), _DEC.sqrt(_dec(nsq[r]))) * scale for r in range(3)]


def _sin(u, v0, w):
    uu, vv, ww = _dot(u, u), _dot(v0, v0), _dot(w, w)
    return 0.0 if uu == 0 or vv == 0 else math.sqrt(float(Fraction(ww, uu * vv)))


@_prec50
def frame_reference(triangle, verts, keep_projections=True):
    """The frame of one triangle over ``verts`` from the exact values of the fp64 inputs (Fraction), 50-digit divisions."""
    tri = [[Fraction(float(x)) for x in p] for p in np.asarray(triangle, dtype=np.float64)]
    u, v, w, v0 = _axes(*tri)
    nsq = [_dot(n, n) for n in (u, v, w)]
    if 0 in nsq:
        return FrameRef(None, 0.0)
    a = tri[0]
    proj = [[], [], []]
    for x in np.asarray(verts, dtype=np.float64):
        d = [Fraction(float(x[k])) - a[k] for k in range(3)]
        for r, n in enumerate((u, v, w)):
            proj[r].append(_dot(n, d))
    rng = [max(p) - min(p) for p in proj]
    unit = None
    if keep_projections:
        inv = [1 / _DEC.sqrt(_dec(nsq[r])) for r in range(3)]
        unit = [[_DEC.multiply(_dec(q), inv[r]) for q in proj[r]] for r in range(3)]
    return FrameRef(_finish(rng, nsq, _D(1)), _sin(u, v0, w), unit)


def _scaled_ints(*arrays):
    """fp64 arrays -> (s, int lists) with value = int / 2^s exactly."""
    s = 0
    fr = []
    for arr in arrays:
        rows = [[Fraction(float(x)) for x in row] for row in np.asarray(arr, dtype=np.float64).reshape(-1, 3)]
        fr.append(rows)
        for row in rows:
            for q in row:
                s = max(s, q.denominator.bit_length() - 1)
    return s, [[[q.numerator * ((1 << s) // q.denominator) for q in row] for row in rows] for rows in fr]


def tau_frame(triangle, verts, sin=None):
    """Per-axis bound 2 D eps (c0 + c1 / sin) on an fp64 extent of this frame (module docstring)."""
    tri = np.asarray(triangle, dtype=np.float64)
    if sin is None:
        f = [[Fraction(float(x)) for x in p] for p in tri]
        u, _, w, v0 = _axes(*f)
        sin = _sin(u, v0, w)
    if sin == 0.0:
        return np.full(3, np.inf)
    big = float(np.max(np.linalg.norm(np.asarray(verts, dtype=np.float64) - tri[0], axis=1)))
    return 2.0 * big * EPS * (C0 + C1 / sin)


@_prec50
def tau_volume(ext, tau):
    """Bound on the product of three extents that are each within tau of ext, formed in two roundings."""
    hi = _D(1)
    for e, t in zip(ext, tau):
        hi *= e + _D(float(t))
    ref = ext[0] * ext[1] * ext[2]
    return hi * (1 + _D(2 * EPS)) - ref


@_prec50
def hull_reference(verts, triangles):
    """[(FrameRef, tau (3,), tau_volume)] for every triangle of a hull (None for a degenerate one): exact integers, and the
    exact evaluation screened to the vertices within 2^-30 D of the fp64 extreme on the rounded exact axis."""
    verts = np.ascontiguousarray(verts, dtype=np.float64)
    triangles = np.asarray(triangles, dtype=np.float64)
    s, (vi, ti) = _scaled_ints(verts, triangles)
    scale = _D(1) / _D(1 << s)
    out = []
    for t, tri in enumerate(triangles):
        a, b, c = ti[3 * t], ti[3 * t + 1], ti[3 * t + 2]
        u, v, w, v0 = _axes(a, b, c)
        nsq = [_dot(n, n) for n in (u, v, w)]
        if 0 in nsq:
            out.append(None)
            continue
        d = verts - tri[0]
        big = float(np.max(np.linalg.norm(d, axis=1)))
        rng = []
        for n in (u, v, w):
            shift = max(0, max(abs(x) for x in n).bit_length() - 900)           # (keep float(int) finite)
            unit = np.array([float(x >> shift) if x >= 0 else -float((-x) >> shift) for x in n])
            unit /= np.linalg.norm(unit)
            q = d @ unit
            ends = []
            for sign in (1, -1):
                near = np.nonzero(sign * q >= np.max(sign * q) - 2.0 ** -30 * big)[0]
                ends.append(max(sign * _dot(n, [vi[j][k] - a[k] for k in range(3)]) for j in near))
            rng.append(ends[0] + ends[1])
        ref = FrameRef(_finish(rng, nsq, scale), _sin(u, v0, w))
        tau = tau_frame(tri, verts, ref.sin)
        out.append((ref, tau, tau_volume(ref.ext, tau)))
    return out


# ---- the assertions both suites call -------------------------------------------------------------------------------
@_prec50
def check_frame(ext, vol, ref, tau, label=""):
    """One frame's extents within tau_frame of the reference, its volume within the product bound.  -> largest |err| / tau."""
    assert ref.ext is not None and ext is not None, f"{label}: no finite frame"
    ext = np.asarray(ext, dtype=np.float64)
    assert ext.shape == (3,) and np.all(np.isfinite(ext)) and np.isfinite(vol), f"{label}: {ext} {vol}"
    ratios = [float(abs(_D(float(ext[r])) - ref.ext[r]) / _D(float(tau[r]))) for r in range(3)]
    assert max(ratios) <= 1.0, f"{label}: extents {ext} against {ref.ext64}: |err| / tau_frame = {ratios}"
    tv = tau_volume(ref.ext, tau)
    assert abs(_D(float(vol)) - ref.vol) <= tv, f"{label}: volume {vol!r} against {float(ref.vol)!r} +- {float(tv)!r}"
    return max(ratios)


@_prec50
def check_hull(ext, vol, href, label=""):
    """The smallest box over a whole hull: the volume inside the bounds on the minimum, the extents within tau_frame of a
    frame whose reference volume is within its tolerance of the returned one.  -> that frame's largest |err| / tau."""
    ext = np.asarray(ext, dtype=np.float64)
    assert ext.shape == (3,) and np.all(np.isfinite(ext)) and np.isfinite(vol), f"{label}: {ext} {vol}"
    live = [f for f in href if f is not None]
    assert live, f"{label}: every frame of the reference is degenerate"
    lo, hi = min(f[0].vol - f[2] for f in live), min(f[0].vol + f[2] for f in live)
    assert lo <= _D(float(vol)) <= hi, f"{label}: volume {vol!r} outside [{float(lo)!r}, {float(hi)!r}]"
    best = None
    for ref, tau, tv in live:
        if abs(_D(float(vol)) - ref.vol) <= tv:
            ratio = max(float(abs(_D(float(ext[r])) - ref.ext[r]) / _D(float(tau[r]))) for r in range(3))
            best = ratio if best is None else min(best, ratio)
    assert best is not None and best <= 1.0, f"{label}: extents {ext} match no frame of that volume (best ratio {best})"
    return best


# ---- inputs: one frame at a time ----------------------------------------------------------------------------------
TRIANGLES = {       # hand-made, sin >= 0.1, unequal edge lengths (an unnormalised frame shows)
    4: [[0.3, -1.2, 2.5], [2.3, -0.5, 2.1], [0.8, 0.7, 3.3]],
    1023: [[-4.0, 1.5, 0.25], [-3.1, 1.9, 1.0], [-4.6, 3.0, 0.5]],
    1024: [[10.0, 20.0, -5.0], [10.5, 23.0, -4.0], [7.0, 20.5, -5.5]],
    1025: [[0.0, 0.0, 0.0], [0.0, 0.0, 3.0], [0.7, -0.2, 2.5]],             # sin = 0.28
    2049: [[1e3, -2e3, 5e2], [1e3 + 3.0, -2e3 + 1.0, 5e2 - 2.0], [1e3 - 1.0, -2e3 + 4.0, 5e2 + 1.0]],
}
FRAME_NT = (1, 256, 257, 1000)
FRAME_NV = (4, 1023, 1024, 1025, 2049)
_SIDES = [(0, 1), (1, 1), (2, -1), (0, -1), (1, -1), (2, 1)]


def frame_positions(nt):
    return sorted({t for t in (0, 63, 64, 255, 256, 257, nt - 1) if t < nt})


def special_vertices(nv):
    return sorted({j for j in (0, 1023, 1024, 2047, nv - 1) if j < nv})


@functools.lru_cache(maxsize=None)
@_prec50
def frame_case(nv):
    """-> (triangle (3, 3), verts (nv, 3), FrameRef, tau): a bulk inside the cube [-1, 1]^3 of the triangle's frame around its
    first corner, and the special vertices 2e-3 (> 1e-3 D) beyond one face each -- the unique hi or lo of one axis."""
    tri = np.array(TRIANGLES[nv], dtype=np.float64)
    u, v0 = tri[1] - tri[0], tri[2] - tri[0]
    w = np.cross(u, v0)
    frame = np.stack([n / np.linalg.norm(n) for n in (u, np.cross(w, u), w)])
    rng = np.random.default_rng(nv)
    local = rng.uniform(-1.0, 1.0, (nv, 3))
    owner = {}
    for i, j in enumerate(special_vertices(nv)):
        axis, sign = _SIDES[i % 6]
        local[j] = rng.uniform(-0.5, 0.5, 3)
        local[j, axis] = sign * 1.002
        owner[j] = (axis, sign)
    verts = np.ascontiguousarray(tri[0] + local @ frame)
    ref = frame_reference(tri, verts)
    tau = tau_frame(tri, verts, ref.sin)
    assert ref.sin >= 0.1
    for j, (axis, sign) in owner.items():           # unique extreme, by far more than the tolerance: dropping it shows
        p = [sign * q for q in ref.proj[axis]]
        assert max(range(nv), key=p.__getitem__) == j and p[j] - sorted(p)[-2] > _D(1e-3), (nv, j)
        assert float(p[j] - sorted(p)[-2]) > 1e6 * tau[axis]
    return tri, verts, ref, tau


def degenerate_triangle(i):
    """Exactly degenerate in fp64: three equal corners (even i) or three collinear ones (odd i)."""
    a = np.array([float(i % 7), -2.0, 0.5 * (i % 3)])
    return np.stack([a, a, a]) if i % 2 == 0 else np.stack([a, a + [1.0, 2.0, -0.5], a + [2.0, 4.0, -1.0]])


def isolated_batch(triangle, nt, t):
    """nt triangles of which only number t spans a box: its frame is the one finite volume, so it is what the call returns."""
    batch = np.stack([degenerate_triangle(i) for i in range(nt)])
    batch[t] = triangle
    return batch


# ---- inputs: exact ties -------------------------------------------------------------------------------------------
BOX_SIDES = (2.0, 0.5, 1.25)
BOX_ORIGIN = (3.0, -1.5, 0.75)


def tie_box():
    """-> (corners (8, 3), [(triangle, extents)] * 6): triangles whose first edge is a box edge and whose second is the next edge at
    the same corner.  Every frame is a signed permutation matrix, every extent and every volume (1.25) exact."""
    o, s = np.array(BOX_ORIGIN), np.array(BOX_SIDES)
    corners = np.array([[o[0] + i * s[0], o[1] + j * s[1], o[2] + k * s[2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    tris = []
    for i, j in ((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)):
        a = corners[(3 * i + j) % 8]                                 # (a different corner each, inward edges)
        b, c = a.copy(), a.copy()
        b[i] = o[i] + s[i] if a[i] == o[i] else o[i]
        c[j] = o[j] + s[j] if a[j] == o[j] else o[j]
        tris.append((np.stack([a, b, c]), np.array([s[i], s[j], s[3 - i - j]])))
    return corners, tris


def tie_batches():
    """-> [(name, triangles, expected extents)]: the six tied frames in several orders, behind degenerate triangles, and spread
    over two workgroups of frames."""
    _, tris = tie_box()
    out = []
    for name, order in (("identity", range(6)), ("reversed", range(5, -1, -1)), ("rotated", (2, 3, 4, 5, 0, 1)), ("swapped", (4, 1, 5, 0, 3, 2))):
        out.append((name, np.stack([tris[i][0] for i in order]), tris[order[0]][1]))
    out.append(("degenerate_first", np.stack([degenerate_triangle(0), degenerate_triangle(1)] + [tris[i][0] for i in (3, 0, 5)]), tris[3][1]))
    wide = np.stack([degenerate_triangle(i) for i in range(300)])
    wide[10], wide[255], wide[256], wide[299] = tris[1][0], tris[2][0], tris[4][0], tris[5][0]
    out.append(("two_workgroups", wide, tris[1][1]))
    late = np.stack([degenerate_triangle(i) for i in range(300)])
    late[256], late[257] = tris[4][0], tris[0][0]
    out.append(("second_workgroup", late, tris[4][1]))
    return out


def check_tie(got, want):
    ext, vol = got
    assert np.array_equal(ext, want) and vol == 1.25, (ext, vol, want)


# ---- inputs: whole hulls ------------------------------------------------------------------------------------------
HULLS = ("box", "sphere", "blob", "voxel_sphere", "georeferenced")


def _rotated_box(n, dims, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    pts = (rng.random((n, 3)) - 0.5) * np.asarray(dims)
    corners = np.array([[sx, sy, sz] for sx in (-.5, .5) for sy in (-.5, .5) for sz in (-.5, .5)]) * np.asarray(dims)
    return np.vstack([pts, corners]) @ q.T + rng.random(3) * 10


@functools.lru_cache(maxsize=None)
def hull_case(kind):
    """-> (hull vertices, hull triangles) of the shapes of tests/test_extent.py and of a georeferenced fp64 cloud (Qhull on the host)."""
    from scipy.spatial import ConvexHull
    import p2d_reference
    rng = np.random.default_rng(3)
    if kind == "box":
        pts = _rotated_box(2000, (1.0, 2.0, 3.0), 4)
    elif kind == "sphere":
        v = rng.standard_normal((1100, 3)); pts = v / np.linalg.norm(v, axis=1, keepdims=True) * [3.0, 2.0, 1.0]
    elif kind == "blob":
        pts = rng.standard_normal((5000, 3)) * [4.0, 1.0, 0.3]
    elif kind == "voxel_sphere":
        v = rng.standard_normal((20000, 3)); pts = np.unique(np.round(v / np.linalg.norm(v, axis=1, keepdims=True) * 40 + 64), axis=0)
    else:
        pts = p2d_reference.georeferenced(40000, 7)
    hull = ConvexHull(pts)
    verts, tri = np.ascontiguousarray(pts[hull.vertices]), np.ascontiguousarray(pts[hull.simplices])
    if kind in ("sphere", "voxel_sphere", "georeferenced"):           # more than one workgroup of frames, a partial last vertex tile
        assert len(tri) > 256 and len(verts) % 1024 != 0, (kind, len(verts), len(tri))
    return verts, tri


@functools.lru_cache(maxsize=None)
def hull_case_reference(kind):
    return hull_reference(*hull_case(kind))


# ---- k_extreme_rows -----------------------------------------------------------------------------------------------
EXTREME_N = (1, 63, 257, 5000, 262145)
EXTREME_NDIRS = (1, 63, 64, 65, 1006, 1024)


def directions(ndirs):
    """The product's own directions (extent._directions: six axes + a Fibonacci lattice), cut or grown to ndirs rows."""
    from open_pcc_metric_amd.extent import _directions
    return np.ascontiguousarray(_directions(1000 if ndirs <= 1006 else ndirs - 6)[:ndirs])


def slice_len(n):
    return -(-n // (4 * min(-(-n // 256), 1024)))


def outside_cases():
    """(n, nplanes): every nplanes at the small n, and the large cloud against one plane, a few, two tiles and four."""
    return [(n, k) for n in OUTSIDE_N[:-1] for k in OUTSIDE_NPLANES] + [(100003, k) for k in (1, 4, 513, 2000)]


def extreme_cases():
    """(n, ndirs): every ndirs at n = 5000, every n at ndirs = 1006, and the corners."""
    cases = [(5000, k) for k in EXTREME_NDIRS] + [(n, 1006) for n in EXTREME_N if n != 5000]
    return cases + [(1, 1), (63, 64), (257, 65), (262145, 65), (262145, 1024)]


def extreme_settings(n, ndirs):
    """(dtype the cloud is set as, slot): all four for the small clouds, split over the cases of the large one."""
    if n < 262145:
        return [("float32", 0), ("float64", 1), ("float32", 1), ("float64", 0)]
    return {1006: [("float32", 1)], 1024: [("float64", 0)]}.get(ndirs, [("float32", 0), ("float64", 1)])


def tau_extreme(points, dirs):
    p = np.asarray(points, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float32).astype(np.float64)
    return 6.0 * 2.0 ** -24 * np.linalg.norm(d, axis=1) * float(np.max(np.linalg.norm(p, axis=1)))


def _top2(points, dirs):
    """fp64: per direction the largest dot product, its row, and the largest among the other rows."""
    p = np.asarray(points, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float32).astype(np.float64)
    m1, m2, r1 = np.full(len(d), -np.inf), np.full(len(d), -np.inf), np.zeros(len(d), dtype=np.int64)
    cols = np.arange(len(d))
    for b in range(0, len(p), 16384):
        dots = d @ p[b:b + 16384].T                                     # (directions in rows: contiguous reductions)
        a = np.argmax(dots, axis=1)
        v1 = dots[cols, a]
        dots[cols, a] = -np.inf
        v2 = dots.max(axis=1)
        m2 = np.maximum(np.maximum(m2, v2), np.minimum(m1, v1))       # the runner-up of the union of two sets
        up = v1 > m1
        m1[up], r1[up] = v1[up], a[up] + b
    return m1, r1, m2


@functools.lru_cache(maxsize=None)
def planted_cloud(n, ndirs, dtype="float32", centre=(0.0, 0.0, 0.0), radius=1.0):
    """-> (points (n, 3) of dtype, dirs (ndirs, 3) fp32, planted {direction: row}).  min(n, ndirs) spikes centre + R d_k, first at
    rows 0, n - 1 and on both sides of slice boundaries, in a bulk of radius <= R / 2.  Asserted: every spike leads its
    direction by at least 2 tau_k in fp64, so its row is the one answer the bound leaves."""
    dirs = directions(ndirs)
    rng = np.random.default_rng(1000 * ndirs + n % 1000)
    per = slice_len(n)
    last = (n - 1) // per
    want = [0, n - 1] + [m * per + e for m in (last, 1, 2, last // 2) for e in (-1, 0)]
    rows = list(dict.fromkeys(r for r in want if 0 <= r < n))
    count = min(n, ndirs)
    rest = np.setdiff1d(np.arange(n), rows)
    rows = (rows + rng.permutation(rest)[:max(0, count - len(rows))].tolist())[:count]
    ks = rng.permutation(ndirs)[:count]
    v = rng.standard_normal((n, 3))
    pts = v / np.linalg.norm(v, axis=1, keepdims=True) * (0.5 * radius * rng.random((n, 1)) ** (1.0 / 3.0))
    pts[rows] = radius * dirs[ks].astype(np.float64)
    pts = (pts + np.asarray(centre)).astype(dtype)
    planted = {int(k): int(r) for k, r in zip(ks, rows)}
    m1, r1, m2 = _top2(pts, dirs)
    tau = tau_extreme(pts, dirs)
    for k, r in planted.items():
        assert r1[k] == r and m1[k] - m2[k] >= 2.0 * tau[k], (n, ndirs, k, r, m1[k] - m2[k], tau[k])
    pts.setflags(write=False)
    return pts, dirs, planted


def check_extreme(points, dirs, rows, planted=None, label=""):
    """Every returned row reaches the fp64 maximum of its direction within tau_k; a planted direction returns the planted
    point (coordinates, not rows: equal points may stand in several rows).  -> largest (max - got) / tau_k."""
    p = np.asarray(points, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float32).astype(np.float64)
    rows = np.asarray(rows)
    assert rows.shape == (len(d),) and np.all((rows >= 0) & (rows < len(p))), f"{label}: rows {rows}"
    best = np.full(len(d), -np.inf)
    for b in range(0, len(p), 16384):
        best = np.maximum(best, (p[b:b + 16384] @ d.T).max(axis=0))
    got = np.einsum("kc,kc->k", p[rows], d)
    tau = tau_extreme(p, d)
    ratio = (best - got) / tau
    worst = int(np.argmax(ratio))
    assert ratio[worst] <= 1.0, f"{label}: direction {worst}: row {rows[worst]} is {best[worst] - got[worst]} short, tau {tau[worst]}"
    for k, r in (planted or {}).items():
        assert np.array_equal(p[rows[k]], p[r]), f"{label}: direction {k}: row {rows[k]}, planted at {r}"
    return float(ratio[worst])


def negative_side_cloud(dtype="float64"):
    """Centred at -10 e_x with radius 1: every dot product is negative for the directions with d_x > 0.1."""
    return planted_cloud(5000, 1006, dtype, (-10.0, 0.0, 0.0), 1.0)


def duplicated_cloud():
    """Every point twice, in neighbouring rows: which of the two rows is returned is not part of the contract."""
    pts, dirs, planted = planted_cloud(257, 65, "float64")
    return np.repeat(pts, 2, axis=0), dirs, {k: 2 * r for k, r in planted.items()}


def georeferenced_cloud():
    """fp64 coordinates whose fp32 casts collide: only the bound holds."""
    import p2d_reference
    return p2d_reference.georeferenced(40000, 7), directions(1006)


# ---- k_outside_planes ---------------------------------------------------------------------------------------------
OUTSIDE_N = (1, 255, 256, 257, 100003)
OUTSIDE_NPLANES = (1, 4, 511, 512, 513, 2000)
_CENTRE = np.array([300000, -200000, -100000], dtype=np.int64)
_RAD = 40000


@functools.lru_cache(maxsize=None)
def _plane_set():
    """2000 planes n.(x - C) <= n.y with integer normals n = round(256 g) and integer points y = round(RAD g) on them."""
    i = np.arange(2000) + 0.5
    phi, theta = np.arccos(1.0 - 2.0 * i / 2000), np.pi * (1.0 + 5.0 ** 0.5) * i
    g = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)
    nrm = np.round(256 * g).astype(np.int64)
    on = np.round(_RAD * g).astype(np.int64)
    assert len(np.unique(nrm, axis=0)) == 2000
    off8 = -(nrm @ _CENTRE) - np.einsum("kc,kc->k", nrm, on)          # 8 * offset
    return g, nrm, on, off8


def _values8(points_int, nplanes):
    """8 (n.x + off) for every point and plane, exactly (|.| < 2^40 in int64)."""
    _, nrm, _, off8 = _plane_set()
    return points_int @ nrm[:nplanes].T + off8[:nplanes]


@functools.lru_cache(maxsize=None)
def outside_case(n, nplanes, with_margin=True, kind="mixed"):
    """-> dict(points (n, 3) fp64 integers, planes (nplanes, 4), margin, rows {name: row}, expected: sorted rows with
    n.x + off > -margin for some plane, by integer arithmetic).  kind: "mixed", "all" (every row outside), "none"."""
    g, nrm, on, off8 = _plane_set()
    q0 = int(np.max(np.abs(nrm[0])))
    axis0 = int(np.argmax(np.abs(nrm[0])))
    margin8 = q0 if with_margin else 0                                  # 8 * margin: one lattice step along plane 0's main axis
    rng = np.random.default_rng(7 * n + nplanes)
    if kind == "all":
        pts = _CENTRE + on[0] + np.round(g[0] * rng.uniform(100, 500, (n, 1))).astype(np.int64) + rng.integers(-50, 50, (n, 3))
    elif kind == "none":
        pts = _CENTRE + rng.integers(-1000, 1000, (n, 3))
    else:
        v = rng.standard_normal((n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
        r = np.where(rng.random((n, 1)) < 0.1, rng.uniform(0, 0.5 * _RAD, (n, 1)), rng.uniform(_RAD - 300, _RAD + 60, (n, 1)))
        pts = _CENTRE + np.round(v * r).astype(np.int64)
    rows = {}
    if kind == "mixed":
        last = nplanes - 1
        step = np.zeros(3, dtype=np.int64); step[axis0] = -np.sign(nrm[0, axis0])
        special = [("outside_last", on[last] + np.round(20 * g[last]).astype(np.int64)),
                   ("outside_0", on[0] + np.round(20 * g[0]).astype(np.int64)),
                   ("on_0", on[0]),
                   ("margin_inside_0", on[0] + step)]
        if nplanes > 512:
            special.append(("outside_512", on[512] + np.round(20 * g[512]).astype(np.int64)))
        special += [("on_last", on[last]), ("centre", np.zeros(3, dtype=np.int64))]
        at = list(dict.fromkeys(r for r in (n - 1, 0, 255, 256, 1, 2, 3) if 0 <= r < n))
        for (name, rel), row in zip(special, at):
            pts[row] = _CENTRE + rel
            rows[name] = row
    assert np.max(np.abs(pts)) < 2 ** 20
    for name, row in rows.items():                                      # the named rows are what their names say
        val8 = _values8(pts[row], nplanes)
        reported = bool(np.any(val8 > -margin8))
        k = {"0": 0, "512": 512, "last": nplanes - 1}.get(name.rsplit("_", 1)[-1])
        others = k is None or bool(np.all(np.delete(val8, k) <= -margin8))
        if name.startswith("outside_"):
            assert val8[k] > 0 and others, (n, nplanes, name)
        elif name.startswith("on_"):
            assert val8[k] == 0 and others and reported == with_margin, (n, nplanes, name)      # 0 > -margin: strict
        elif name == "margin_inside_0":
            assert val8[0] == -q0 and others and not reported, (n, nplanes, name)
        else:
            assert not reported
    assert np.any(off8[:nplanes] > -margin8)                            # the origin is outside: an unguarded thread past n reports
    expected = np.concatenate([b + np.nonzero(np.any(_values8(pts[b:b + 4096], nplanes) > -margin8, axis=1))[0]
                               for b in range(0, n, 4096)])
    assert {"all": len(expected) == n, "none": len(expected) == 0}.get(kind, True)
    planes = np.column_stack([nrm[:nplanes] / 8.0, off8[:nplanes] / 8.0])
    points = pts.astype(np.float64)
    points.setflags(write=False)
    return dict(points=points, planes=np.ascontiguousarray(planes), margin=margin8 / 8.0, rows=rows, expected=expected)


def check_outside(case, got, label=""):
    """Unique rows, as many as the exact set has, and the same set."""
    got = np.asarray(got)
    assert len(np.unique(got)) == len(got), f"{label}: a row is reported twice"
    assert len(got) == len(case["expected"]), f"{label}: {len(got)} rows, expected {len(case['expected'])}"
    want = set(case["expected"].tolist())
    have = set(got.tolist())
    named = {name: row for name, row in case["rows"].items() if (row in want) != (row in have)}
    assert have == want, f"{label}: {len(have - want)} rows too many, {len(want - have)} missing; named rows that differ: {named}"


# ---- NumPy models of the kernels, one defect at a time --------------------------------------------------------------
DEFECTS = {
    "obb": ("tile_last_vertex", "partial_tile", "frame_index", "not_normalised", "argmin_last", "degenerate_zero"),
    "extreme": ("last_slice", "dirs_from_64", "no_sign_fix"),
    "outside": ("first_tile_only", "last_plane", "rows_past_n", "greater_equal", "margin_sign"),
}


def model_obb_frames(verts, triangles, defect=None):
    """k_obb_frames (256 frames per workgroup, thread t of the grid owns triangle t, vertices in tiles of 1024 with a partial
    last one) and the host's choice in pccm_obb_frames (first smallest finite volume).  Raises ValueError like the call."""
    verts = np.asarray(verts, dtype=np.float64)
    tri = np.asarray(triangles, dtype=np.float64)
    nv, nt = len(verts), len(tri)
    src = np.arange(nt)
    if defect == "frame_index":
        src = np.where(src < 256, src, np.minimum(src + 1, nt - 1))
    a = tri[src, 0]
    u, v0 = tri[src, 1] - a, tri[src, 2] - a
    w = np.cross(u, v0)
    frame = np.stack([u, np.cross(w, u), w], axis=1)                    # (nt, 3 rows, 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        if defect != "not_normalised":
            frame = frame / np.sqrt(np.sum(frame * frame, axis=2, keepdims=True))
        lo, hi = np.full((nt, 3), np.inf), np.full((nt, 3), -np.inf)
        for base in range(0, nv, 1024):
            m = min(1024, nv - base)
            if defect == "partial_tile" and m < 1024:
                break
            if defect == "tile_last_vertex" and m == 1024:
                m -= 1
            loc = np.einsum("tjc,trc->tjr", verts[None, base:base + m] - a[:, None], frame)
            lo, hi = np.fmin(lo, np.fmin.reduce(loc, axis=1)), np.fmax(hi, np.fmax.reduce(loc, axis=1))
        ext = hi - lo
        ok = np.all((ext >= 0.0) & (ext < np.inf), axis=1)
        vol = ext[:, 0] * ext[:, 1] * ext[:, 2]
        if defect == "degenerate_zero":
            vol = np.where(ok & (vol < np.inf), vol, 0.0)
        else:
            vol = np.where(ok & (vol < np.inf), vol, np.inf)
    best = -1
    for t in range(nt):
        if vol[t] < np.inf and (best < 0 or vol[t] < vol[best] or (defect == "argmin_last" and vol[t] == vol[best])):
            best = t
    if best < 0:
        raise ValueError("degenerate convex hull: no triangle spans a box of finite volume")
    return ext[best].copy(), float(vol[best])


def model_extreme_rows(points, dirs, defect=None):
    """k_extreme_rows: 4 waves per workgroup, min(ceil(n / 256), 1024) workgroups, wave w owns rows [w per, (w + 1) per); lane l
    owns the directions l + 64 j; fp32 dot products (not contracted here) under the order-preserving key, row in the low word."""
    p = np.asarray(points).astype(np.float32)
    d = np.asarray(dirs, dtype=np.float32)
    n, per = len(p), slice_len(len(p))
    dots = (d[None, :, 0] * p[:, None, 0] + d[None, :, 1] * p[:, None, 1]) + d[None, :, 2] * p[:, None, 2]
    bits = np.ascontiguousarray(dots).view(np.uint32)
    b = bits if defect == "no_sign_fix" else np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000))
    key = (b.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[:, None]
    if defect == "last_slice":
        key = key[:((n - 1) // per) * per]
    best = key.max(axis=0) if len(key) else np.zeros(len(d), dtype=np.uint64)
    if defect == "dirs_from_64":
        best[64:] = 0
    return (best & np.uint64(0xffffffff)).astype(np.int32)


def model_rows_outside(points, planes, margin, defect=None):
    """k_outside_planes: one thread per row in workgroups of 256 (the threads past n read the origin), planes in tiles of 512."""
    x = np.asarray(points, dtype=np.float64)
    pl = np.asarray(planes, dtype=np.float64)
    n = len(x)
    padded = np.zeros((-(-n // 256) * 256, 3))
    padded[:n] = x
    outside = np.zeros(len(padded), dtype=bool)
    nplanes = len(pl) - 1 if defect == "last_plane" else len(pl)
    for base in range(0, nplanes, 512):
        if defect == "first_tile_only" and base:
            break
        tile = pl[base:min(base + 512, nplanes)]
        val = padded @ tile[:, :3].T + tile[:, 3]
        m = margin if defect == "margin_sign" else -margin
        outside |= np.any(val >= m if defect == "greater_equal" else val > m, axis=1)
    live = np.ones(len(padded), dtype=bool) if defect == "rows_past_n" else np.arange(len(padded)) < n
    return np.nonzero(live & outside)[0].astype(np.int32)
