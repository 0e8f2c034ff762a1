"""NumPy restatement of the colour and joint point-to-distribution values ("Point-to-distribution: colour and
joint"; include/pccm.h, pccm_p2d_build_attrs / PCCM_METRIC_P2D_COLOR / PCCM_METRIC_P2D_JOINT) -- the yardstick of their tests --
and the coloured clouds those tests run on.

TEST INFRASTRUCTURE.  It does not import the product's kernels.  Neighbour rows and the geometry value M_G come from
tests/p2d_reference.py, luma from tests/pointssim_reference.luma (the project's transform_colors, which existing tests pin to the
reference's np.matmul).  Every other step is one NumPy element-wise op on fp64 arrays, so each is rounded separately, as the
device's __dadd_rn / __dmul_rn / __dsub_rn / __ddiv_rn / __dsqrt_rn are; the two sums start from 0.0 and run left to right over the
neighbourhood, one addition per neighbour.  The device's columns must therefore equal color_mahalanobis() and joint() bit for
bit."""
import numpy as np

import p2d_reference as geo
from pointssim_reference import luma

RIDGE = 2.0 ** -20


def luma_moments(ya, yb, nbr):
    """(m, V) of each neighbourhood: mean and RAW population variance (it can round below 0) of e_j = yb[nbr[:, j]] - ya."""
    ya, yb = np.asarray(ya, dtype=np.float64), np.asarray(yb, dtype=np.float64)
    n, kk = nbr.shape
    s1, s2 = np.zeros(n), np.zeros(n)
    for j in range(kk):
        e = yb[nbr[:, j]] - ya
        s1 = s1 + e
        s2 = s2 + e * e
    kkf = np.float64(kk)
    m = s1 / kkf
    return m, s2 / kkf - m * m


def color_mahalanobis(ca, cb, nbr, return_parts=False):
    """The colour column of direction a -> b: M_Y(p) for every point p of a (colours ca) against the colours cb of its
    neighbours `nbr` (rows of b, ascending (d2, row): p2d_reference.knn_rows)."""
    m, raw = luma_moments(luma(ca), luma(cb), np.asarray(nbr, dtype=np.int64))
    v = np.maximum(raw, 0.0) + RIDGE
    out = np.abs(m) / np.sqrt(v)
    if return_parts:
        return out, m, raw
    return out


def joint(mg, my):
    """M_J = sqrt(M_G * M_G + M_Y * M_Y); +inf where M_G is."""
    return np.sqrt(mg * mg + my * my)


def columns(a, b, ca, cb, k, nbr=None):
    """(M_G, M_Y, M_J) of direction a -> b."""
    nbr = geo.knn_rows(a, b, k) if nbr is None else np.asarray(nbr, dtype=np.int64)
    mg = geo.mahalanobis(a, b, k, nbr=nbr)
    my = color_mahalanobis(ca, cb, nbr)
    return mg, my, joint(mg, my)


# ---- the colours of the tests ([n, 3] float64 arrays in [0, 1]) ------------------------------------------------------------------
def smooth_colors(p, seed, noise=0.02, span=1.0):
    """A smooth colour field over the first two coordinates plus noise."""
    rng = np.random.default_rng(seed)
    u, v = p[:, 0], p[:, 1]
    field = np.column_stack([0.5 + 0.4 * span * np.sin(3.0 * u), 0.5 + 0.4 * span * np.cos(2.0 * v), 0.5 + 0.3 * span * np.sin(2.0 * (u + v))])
    return np.clip(field + rng.normal(0, noise, field.shape), 0.0, 1.0)


def to_bytes(colors):
    return np.rint(np.asarray(colors) * 255.0).astype(np.uint8)


def byte_colors(p, seed):
    """(colours, bytes): a slowly varying field (a few byte levels over the whole cloud) quantised to bytes -- most neighbourhoods
    are flat: every neighbour has the same bytes."""
    u8 = to_bytes(smooth_colors(p, seed, noise=0.0, span=0.01))
    return u8 / 255.0, u8


def random_colors(n, seed):
    return np.random.default_rng(seed).random((n, 3))


def random_byte_colors(n, seed):
    u8 = np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)
    return u8 / 255.0, u8


def constant_colors(n, rgb):
    return np.tile(np.asarray(rgb, dtype=np.float64), (n, 1))


def inf_geometry(seed):
    """(a, b): 70 points of b share one location and no other point of b lies within 0.2 of it; the points of a next to it see
    nothing else among their (up to 64) nearest, so their geometry value is +inf -- except the one point of a AT the location,
    whose value is 0."""
    rng = np.random.default_rng(seed)
    spot = np.array([0.5, 0.5, 0.5])
    others = rng.random((1500, 3))
    others = others[np.linalg.norm(others - spot, axis=1) > 0.2]
    b = np.concatenate([np.tile(spot, (70, 1)), others])
    a = np.concatenate([rng.random((800, 3)), spot + rng.normal(0, 1e-3, (60, 3)), spot[None, :]])
    return a[rng.permutation(len(a))], b[rng.permutation(len(b))]


def _family(clouds, colors):
    def make():
        a, b = clouds()
        ca, cb = colors(a, b)
        return a, b, ca, cb
    return make


# name -> () -> (a, b, colours of a, colours of b)
FAMILIES = {
    "surface_smooth": _family(lambda: (geo.surface(3000, 3), geo.surface(2800, 4)),
                              lambda a, b: (smooth_colors(a, 201), smooth_colors(b, 202))),
    # (b: flat neighbourhoods; a: any bytes, so that the flat differences e_j take thousands of values)
    "surface_bytes": _family(lambda: (geo.surface(3000, 3), geo.surface(2800, 4)),
                             lambda a, b: (random_byte_colors(len(a), 203)[0], byte_colors(b, 204)[0])),
    "constant_offset": _family(lambda: (geo.uniform(3000, 1), geo.uniform(2500, 2)),
                               lambda a, b: (constant_colors(len(a), (0.2, 0.4, 0.6)), constant_colors(len(b), (0.25, 0.45, 0.55)))),
    "random": _family(lambda: (geo.uniform(3000, 1), geo.uniform(2500, 2)),
                      lambda a, b: (random_colors(len(a), 205), random_colors(len(b), 206))),
    "duplicates": _family(lambda: (geo.duplicates(2500, 5), geo.duplicates(2000, 6)),
                          lambda a, b: (random_byte_colors(len(a), 207)[0], random_byte_colors(len(b), 208)[0])),
    "lattice": _family(lambda: (geo.lattice(14, 2400, 7), geo.lattice(14, 2200, 8)),
                       lambda a, b: (random_colors(len(a), 209), random_colors(len(b), 210))),
    "b_smaller_than_k": _family(lambda: (geo.uniform(900, 13), geo.uniform(3, 14)),
                                lambda a, b: (random_colors(len(a), 211), random_colors(len(b), 212))),
    "planes": _family(lambda: (geo.planes(40, 2000, 9, (3, 4)), geo.planes(40, 1800, 10, (3, 5))),
                      lambda a, b: (smooth_colors(a / 40.0, 213), smooth_colors(b / 40.0, 214))),
    "inf_geometry": _family(lambda: inf_geometry(215),
                            lambda a, b: (random_colors(len(a), 216), random_colors(len(b), 217))),
}
