"""Planted cases for the uniform-grid engine (k_grid_query, k_grid_query_coop, k_grid_tail: open_pcc_metric_amd/csrc/pccm_grid.hip;
face_bound / settled_by: pccm_grid.h; k_brick_query's ring-1 rule: pccm_brick.hip), each with a host model of what the stop rule must
decide and a proof -- on the host, about the DATA -- that the case is what its family claims.  NumPy only; the truth comes from oracle/
(kd-tree) and, for the small cases, from an fp64 brute force in the reference's expression ((dx*dx)+(dy*dy))+(dz*dz), smallest row
on ties.  The library is never imported here.

The model, written from the kernel source:

  geometry  (org, h, dim) as pccm_grid_geometry reports it; inv_h = 1 / h, slack[a] = (|org[a]| + (dim[a] + 2) h[a]) 2^-48 (geom_of).
  cell      clamp(floor((x - org) * inv_h), 0, dim - 1) per axis (cell_coord).
  L_r       face_bound(q, r): the smallest, over the axes and sides on which the cube [c - r, c + r]^3 still has cells behind it, of
            the distance from q to that face minus slack; inf when it has none.  Evaluated in fp64 as the kernel writes it.
  stop      the search ends at the first ring r in 1 .. 3 with L_r == inf or (L_r > 0 and best_r < L_r^2 (1 - 2^-30)), best_r being
            the smallest squared distance inside the cube.  face_bound never exceeds the distance to anything outside the cube, so
            best_r < L_r^2 implies best_r == d, the query's global nearest distance, and best_r >= d always: the rule depends on d
            alone.  A query SETTLES AT r when r is the first ring with L_r == inf or d < L_r^2 (1 - 2^-30); a query no ring
            settles is FLAGGED for the exact rescan.

The device may contract org + c * h into an FMA, so the model claims no bit equality: a query whose d lies within a relative 2^-20
of the L_r^2 of a ring the rule looks at (or whose L_r is within 2^-20 h of 0) is UNDECIDED, and every planted case must have none
(a condition on the inputs: build() nudges background points that break it, the tests assert it).

Counts the model predicts for one direction of a search (predict()):
  flagged   == nn_stats()["fallback_queries"] on every path: a query that goes to the tail only for lack of an fp32 certificate
            settles at ring 2 at the latest (best_2 <= best_1 < L_1^2 <= L_2^2);
  lo        queries the model does not settle at ring 1: lo <= nn_stats()["tail_queries"] on the paths with a tail;
  band      queries the model settles at ring 1 whose fp32 certificate or fp32 stop rule the host cannot decide (band_mask()):
            tail_queries <= lo + band, and every case keeps band <= lo / 20.
  overflow  the brick kernel alone: queries of a brick whose staged records exceed its LDS budget all go to the tail, whatever
            the stop rule says (brick_overflow(), a port of the budget); they count into lo there.

Cases are planted on a grid the library chooses, in two phases (build()): a FRAME of background points fixes both clouds' sizes and
bounding boxes and leaves a reserved region empty in both clouds; the probes of every scenario are placed inside the region, in
cell units of a geometry -- the predicted one first (predict_geometry(), a port of choose_geometry), the one read back from the
library afterwards.  Scenarios sit 9 cells apart with one query each; offsets from faces are h 2^-10, far above fp32 rounding, so
the same cases serve fp32-exact clouds.

Families:
  F  faces: per axis, side and ring r (18 combinations) a SOUND site -- the true neighbour h 2^-10 beyond the face of the ring-r
     cube, a decoy inside it a little farther away in another direction: the true row must come back, one ring later or from the
     rescan -- and a NOT-LAZY site -- the neighbour inside the cube at L_r (1 - 2^-10): the query must settle there;
  B  boundaries: queries in a corner, an edge and a face cell of the grid (missing faces count as infinitely far), the neighbour at
     L_1 (1 -+ 2^-10); small_case(): planar and collinear pairs (dim = 1) and grids every cube covers (L == inf);
  T  ties: a ring-1 and a ring-2 point at exactly the same distance (dyadic 3-4-5 offsets), the ring-2 point on the smaller row;
     three equidistant points in three x-runs with the smallest row in the highest lane, settling at ring 2 (25 lanes of wave_tail)
     and at ring 3 (49 lanes); three identical points of the first cloud (self search: duplicates at distance 0);
  R  rescan hand-off: flagged queries whose best of three rings (a decoy) and true neighbour (beyond the ring-3 face) are in
     reversed order in the fp32 arithmetic of the rescan's filter (brute_planted.dist32), found by search over candidate pairs;
     every scenario query is alone in its own cloud, so the self search flags all of them with nothing found (INFINITY);
  X  trimmed box (build_trim()): stray points far outside on every side in both clouds, so that the grid covers a quantile box and
     they clamp into boundary cells (plant_x()).
  long_tail_case(): two fp32 clouds in alternating slabs ~4 cells thick: more than 2^18 queries per direction fail ring 1.
"""
import functools
from types import SimpleNamespace

import numpy as np

KMAX = 3                                   # kMaxRing
PPC = 1.4                                  # points_per_cell()
COOP_MIN = 40.0                            # kCoopMinPointsPerRow
TAIL_WAVE_MAX = 1 << 18                    # kTailWaveMax
SEG = 64.0                                 # kSegWidth + 3: cells a segment of k_grid_query_coop can span along x
OFF = 2.0 ** -10                           # planted offsets, in cells
UNDECIDED = 2.0 ** -20
FLAGGED = KMAX + 1
ROOM = 4.0                                 # room on the certificates' widths


# ---- geometry and the stop rule --------------------------------------------------------------------------------------------------
def make_geom(org, h, dim):
    org, h = np.asarray(org, np.float64).copy(), np.asarray(h, np.float64).copy()
    dim = np.asarray(dim, np.int64).copy()
    return SimpleNamespace(org=org, h=h, dim=dim, inv_h=1.0 / h, slack=(np.abs(org) + (dim + 2) * h) * 2.0 ** -48)


def same_geom(g, k):
    return bool(np.array_equal(g.org, k.org) and np.array_equal(g.h, k.h) and np.array_equal(g.dim, k.dim))


def predict_geometry(a, b, scale=1.0, box=None):
    """choose_geometry() for the pair (a, b): the union bounding box (or the trimmed `box` = (lo, hi)), the cell edge from the mean
    point count."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    lo, hi = np.minimum(a.min(axis=0), b.min(axis=0)), np.maximum(a.max(axis=0), b.max(axis=0))
    if box is not None:
        lo, hi = np.asarray(box[0], np.float64), np.asarray(box[1], np.float64)
    npts = (len(a) + len(b)) / 2.0
    ext = hi - lo
    nz = int(np.sum(ext > 0))
    h = 1.0
    if nz:
        h = float(np.prod(ext[ext > 0]) * PPC / npts) ** (1.0 / nz) * scale
    dim = np.where(ext > 0, np.clip(np.ceil(ext / h), 1, 4096), 1).astype(np.int64)
    assert np.prod(dim) <= 1 << 26
    hh = np.where(ext > 0, ext / dim, 1.0) * (1.0 + 2.0 ** -40)
    return make_geom(lo, hh, dim)


def cells(g, p):
    t = np.floor((np.asarray(p, np.float64) - g.org) * g.inv_h)
    return np.clip(t, 0, g.dim - 1).astype(np.int64)


def face_bounds(g, q, c=None, skip=None):
    """L_r of every query for r = 1 .. KMAX -> [n, KMAX], in face_bound's own expressions.  skip = (axis, side): that face is ignored
    (an UNSOUND rule, for the host test of the cases' discriminating power)."""
    q = np.atleast_2d(np.asarray(q, np.float64))
    c = cells(g, q) if c is None else np.atleast_2d(c)
    L = np.full((len(q), KMAX), np.inf)
    for r in range(1, KMAX + 1):
        for a in range(3):
            if skip != (a, 0):
                v = (q[:, a] - (g.org[a] + (c[:, a] - r).astype(np.float64) * g.h[a])) - g.slack[a]
                L[:, r - 1] = np.where(c[:, a] - r > 0, np.minimum(L[:, r - 1], v), L[:, r - 1])
            if skip != (a, 1):
                v = ((g.org[a] + (c[:, a] + r + 1).astype(np.float64) * g.h[a]) - q[:, a]) - g.slack[a]
                L[:, r - 1] = np.where(c[:, a] + r < g.dim[a] - 1, np.minimum(L[:, r - 1], v), L[:, r - 1])
    return L


def lazy_bounds(g, q):
    """A deliberately LAZY rule: L_r replaced by r h (the smallest edge among the axes that have a face at all)."""
    L = face_bounds(g, q)
    return np.where(np.isinf(L), np.inf, np.arange(1, KMAX + 1)[None, :] * g.h.min())


def settled_by(L, d):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.isinf(L) | ((L > 0.0) & (d < L * L * (1.0 - 2.0 ** -30)))


def classify(g, q, d, L=None):
    """-> (ring, undecided): the ring each query settles at (FLAGGED = 4: none) from its nearest squared distance d, and whether the
    decision of a ring the rule looks at lies within the band the model does not claim."""
    L = face_bounds(g, q) if L is None else L
    d = np.asarray(d, np.float64)
    ring = np.full(len(d), FLAGGED, np.int64)
    undecided = np.zeros(len(d), bool)
    for r in range(KMAX, 0, -1):
        ring = np.where(settled_by(L[:, r - 1], d), r, ring)
    for r in range(1, KMAX + 1):
        Lr = L[:, r - 1]
        fin = np.isfinite(Lr)
        L2 = np.where(fin, Lr * Lr, 1.0)
        near = fin & ((np.abs(d - L2) <= UNDECIDED * L2) | (np.abs(Lr) <= UNDECIDED * g.h.max()))
        undecided |= near & (r <= ring)
    return ring, undecided


# ---- truth -----------------------------------------------------------------------------------------------------------------------
def dist64(q, p):
    d = np.asarray(q, np.float64) - np.asarray(p, np.float64)
    return ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])


def brute64(queries, searched, self_search=False):
    """fp64 brute force in the reference's expression, smallest row on ties -> (rows, d2)."""
    q, s = np.asarray(queries, np.float64), np.asarray(searched, np.float64)
    rows, d2 = np.empty(len(q), np.int64), np.empty(len(q))
    step = max(1, (1 << 21) // max(len(s), 1))
    for lo in range(0, len(q), step):
        hi = min(len(q), lo + step)
        d = dist64(q[lo:hi, None, :], s[None, :, :])
        if self_search:
            d[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
        rows[lo:hi] = d.argmin(axis=1)
        d2[lo:hi] = d[np.arange(hi - lo), rows[lo:hi]]
    return rows, d2


def pair_of(case, direction):
    """(queries, searched, self search) of direction 0 (first cloud searches the second), 1 (the reverse) and 2 (first in itself)."""
    return ((case.a, case.b, False), (case.b, case.a, False), (case.a, case.a, True))[direction]


def truth(case, direction):
    """oracle.nn(method="kdtree") of one direction, computed once per case object and left unchanged."""
    if direction not in case.truth:
        from oracle import oracle as orc
        q, s, self_ = pair_of(case, direction)
        rows, d2 = orc.nn(q, s, skip_same_index=self_, method="kdtree")
        rows, d2 = rows.astype(np.int64), np.asarray(d2, np.float64)
        rows.flags.writeable = d2.flags.writeable = False
        case.truth[direction] = (rows, d2)
    return case.truth[direction]


# ---- a literal, slow port of thread_search ----------------------------------------------------------------------------------------
def sort_by_cell(g, s):
    c = cells(g, s)
    lin = (c[:, 2] * g.dim[1] + c[:, 1]) * g.dim[0] + c[:, 0]
    order = np.argsort(lin, kind="stable")
    start = np.searchsorted(lin[order], np.arange(int(np.prod(g.dim)) + 1))
    return order, start


def thread_search_port(g, queries, searched, self_search=False, bounds=face_bounds, grid=None, qrows=None):
    """thread_search() query by query: ring 1 = the 3 x 3 x 3 block, ring r > 1 = the shell of the cube [c - r, c + r]^3, the
    lexicographic (d2, row) minimum over what was scanned, settled_by(bound(q, r), best) after every ring.
    qrows: the queries' own rows in the searched cloud (self search of a subset; default 0 .. n - 1).
    -> (ring [FLAGGED: open after KMAX rings], row, d2 of the best found so far; row -1, d2 inf when nothing was found)."""
    q_all, s = np.asarray(queries, np.float64), np.asarray(searched, np.float64)
    order, start = grid if grid is not None else sort_by_cell(g, s)
    dx, dy, dz = (int(v) for v in g.dim)
    out_ring, out_row, out_d = np.empty(len(q_all), np.int64), np.empty(len(q_all), np.int64), np.empty(len(q_all))
    cq = cells(g, q_all)
    Ls = bounds(g, q_all)
    for i, q in enumerate(q_all):
        cx, cy, cz = (int(v) for v in cq[i])
        best, brow = np.inf, 0x7fffffff
        ring = FLAGGED
        for r in range(1, KMAX + 1):
            for z in range(max(cz - r, 0), min(cz + r, dz - 1) + 1):
                for y in range(max(cy - r, 0), min(cy + r, dy - 1) + 1):
                    row = (z * dy + y) * dx
                    if r == 1 or z in (cz - r, cz + r) or y in (cy - r, cy + r):
                        runs = [(max(cx - r, 0), min(cx + r, dx - 1))]
                    else:
                        runs = [(x, x) for x in (cx - r, cx + r) if 0 <= x <= dx - 1]
                    for x0, x1 in runs:
                        for p in range(start[row + x0], start[row + x1 + 1]):
                            srow = int(order[p])
                            if self_search and srow == (i if qrows is None else int(qrows[i])):
                                continue
                            d = float(dist64(q, s[srow]))
                            if d < best or (d == best and srow < brow):
                                best, brow = d, srow
            if bool(settled_by(Ls[i, r - 1], best)):
                ring = r
                break
        out_ring[i], out_row[i], out_d[i] = ring, (brow if brow != 0x7fffffff else -1), best
    return out_ring, out_row, out_d


# ---- ring-1 candidates: nearest and second nearest (what the certificates of the ring-1 kernels compare) ------------------------------
def ring1_two(g, queries, searched, self_search=False):
    """Smallest and second smallest squared distance among the searched points of the 27 cells around every query -> (d1, d2),
    inf where there are fewer."""
    q, s = np.asarray(queries, np.float64), np.asarray(searched, np.float64)
    order, start = sort_by_cell(g, s)
    sp = s[order]
    c = cells(g, q)
    b1, b2 = np.full(len(q), np.inf), np.full(len(q), np.inf)
    x0, x1 = np.maximum(c[:, 0] - 1, 0), np.minimum(c[:, 0] + 1, g.dim[0] - 1)
    for k in range(9):
        z, y = c[:, 2] + k // 3 - 1, c[:, 1] + k % 3 - 1
        ok = (z >= 0) & (z < g.dim[2]) & (y >= 0) & (y < g.dim[1])
        row = np.where(ok, (z * g.dim[1] + y) * g.dim[0], 0)
        a, e = np.where(ok, start[row + x0], 0), np.where(ok, start[row + x1 + 1], 0)
        idx = np.flatnonzero(e > a)
        pos, end = a[idx], e[idx]
        while len(idx):
            d = dist64(q[idx], sp[pos])
            if self_search:
                d = np.where(order[pos] == idx, np.inf, d)
            o1, o2 = b1[idx], b2[idx]
            b2[idx] = np.minimum(o2, np.maximum(o1, d))
            b1[idx] = np.minimum(o1, d)
            pos = pos + 1
            keep = pos < end
            idx, pos, end = idx[keep], pos[keep], end[keep]
    return b1, b2


def band_mask(g, q, d, ring, path, two):
    """Queries the model settles at ring 1 that the ring-1 kernel of `path` ("coop" / "brick") may still hand to the tail.
    coop (pccm_grid.hip, certification of k_grid_query_coop): thr / best = ((1 + 2^-20) + 2^-20 (|f|_inf + sqrt best) / sqrt best)^2
      (1 + 2^-30), f the query's coordinates relative to its segment's corner: |f|_inf <= min(SEG, dim_x) cells; fp32 distances of relative
      coordinates are off by a few 2^-24 of the same magnitudes, inside the room.  Its stop rule is the fp64 one: no second band.
    brick (pccm_brick.hip): thr = best (1 + 2^-18) + 2e-36 on fp32 distances of fp32-exact inputs; the stop rule asks
      best 1.00001 < L^2 0.99999 with L from face32, whose faces stand 8 M 2^-24 (M: the grid's largest coordinate + 2 h) inside
      the fp64 ones and whose own evaluation rounds three times at that magnitude; the window's x-cell is computed in fp32."""
    d1, d2 = two
    L = face_bounds(g, q)[:, 0]
    s1 = ring == 1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if path == "coop":
            rb = np.sqrt(d1)
            width = ((1.0 + 2.0 ** -20) + 2.0 ** -20 * (min(SEG, float(g.dim[0])) * g.h.max() + rb) / rb) ** 2 * (1.0 + 2.0 ** -30) - 1.0
            return s1 & ~(d2 > d1 * (1.0 + ROOM * width))
        M = np.max(np.maximum(np.abs(g.org), np.abs(g.org + g.dim * g.h)) + 2.0 * g.h)
        cert = s1 & ~(d2 > d1 * (1.0 + ROOM * (2.0 ** -18 + 2.0 ** -21)) + 1.0e-35)
        wl = ROOM * (2.0e-5 + 2.0 ** -18 + 2.0 * 12.0 * M * 2.0 ** -24 / L)
        stop = s1 & np.isfinite(L) & ~(d < L * L * (1.0 - wl))
        t = (np.asarray(q, np.float64)[:, 0] - g.org[0]) * g.inv_h[0]
        edge = s1 & (np.abs(t - np.rint(t)) <= ROOM * 4.0 * M * 2.0 ** -24 * g.inv_h[0])
        return cert | stop | edge


def brick_overflow(g, queries, searched, n_max, n_queries=None):
    """Queries whose brick hands ALL its queries to the tail because the records it would stage exceed its LDS budget
    (launch_brick_query / launch_shape / brick_body, pccm_brick.hip: `T > bp.cap`).  The budget follows the MEAN density
    n_max / ncells (+ a quarter or eight sigma, + 64, rounded up to a compiled plane); a brick is bx x 4 x 2 cells (4 x 4 for a
    shard of at most 0.55 of the rows), stages the runs of (BY + 2)(BZ + 2) rows over its own cells and one more on each side,
    every run padded to an even length.  n_max: the larger cloud; n_queries: rows of the shard (default: all)."""
    q, s = np.asarray(queries, np.float64), np.asarray(searched, np.float64)
    dx, dy, dz = (int(v) for v in g.dim)
    ncells = dx * dy * dz
    density, density_q = n_max / ncells, (len(q) if n_queries is None else n_queries) / ncells
    nbx = -(-dx // 48)
    bx = min(-(-dx // nbx), 64)
    nbx = -(-dx // bx)
    BY, BZ = (4, 4) if density_q <= 0.55 * density else (4, 2)
    expect = (BY + 2) * (BZ + 2) * (bx + 2) * density
    cap = max(int(expect + min(0.25 * expect, 8.0 * np.sqrt(expect))) + 64, 256)
    cap = next((pl for pl in (2176, 3008) if cap + 4 <= pl), 3584) - 4
    cs_ = cells(g, s)
    cnt = np.zeros((dz, dy, dx), np.int64)
    np.add.at(cnt, (cs_[:, 2], cs_[:, 1], cs_[:, 0]), 1)
    nby, nbz = -(-dy // BY), -(-dz // BZ)
    over = np.zeros((nbz, nby, nbx), bool)
    for ix in range(nbx):
        sx0, sx1 = max(ix * bx - 1, 0), min(min(ix * bx + bx, dx) + 1, dx)
        run = cnt[:, :, sx0:sx1].sum(axis=2)
        run = (run + 1) & ~1                                       # odd runs carry a pad record
        run = np.pad(run, ((1, BZ * nbz - dz + 1), (1, BY * nby - dy + 1)))
        csum = np.pad(run.cumsum(axis=0).cumsum(axis=1), ((1, 0), (1, 0)))
        for iz in range(nbz):
            z0, z1 = iz * BZ, iz * BZ + BZ + 2
            y0, y1 = np.arange(nby) * BY, np.arange(nby) * BY + BY + 2
            T = csum[z1, y1] - csum[z0, y1] - csum[z1, y0] + csum[z0, y0]
            over[iz, :, ix] = T > cap
    cq = cells(g, q)
    return over[cq[:, 2] // BZ, cq[:, 1] // BY, cq[:, 0] // bx]


def predict(case, direction, path=None, g=None, bounds=face_bounds):
    """The model's counts for one direction on geometry g (default: the case's own) -> namespace(ring, undecided, flagged, lo, band,
    by_site: {scenario name: ring of its query}); band only for path "coop" / "brick"."""
    g = case.geom if g is None else g
    q, s, self_ = pair_of(case, direction)
    _, d = truth(case, direction)
    ring, und = classify(g, q, d, bounds(g, q))
    out = SimpleNamespace(ring=ring, undecided=np.flatnonzero(und), flagged=int(np.sum(ring == FLAGGED)), lo=int(np.sum(ring != 1)), band=0,
                          band_mask=np.zeros(len(ring), bool))
    if path in ("coop", "brick"):
        key = (direction, path)
        if key not in case.two:
            case.two[key] = ring1_two(g, q, s, self_)
        out.band_mask = band_mask(g, q, d, ring, path, case.two[key])
        out.band = int(np.sum(out.band_mask))
    if direction != 1:
        out.by_site = {sc.name: int(ring[sc.qrow]) for sc in case.sites}
    return out


# ---- frames ----------------------------------------------------------------------------------------------------------------------
# A frame is a box [0, D]^3 in units of the cell edge it aims at (the point count is chosen so that the library's rule gives unit
# cells), laid out along z: a dense zone of uniform background, a sparse zone where both clouds sit on jittered,
# interleaved lattices of spacing 1.7 (no point has a neighbour within ring 1's reach there, in either cloud or its own: that is where
# `lo` comes from), the reserved region, and eight pins at the box's corners in both clouds (they fix the bounding boxes).
# The dense zones are as long as they are because the library sets the point count: cells hold 1.4 points on average over the whole
# box, the region's 50-60 000 cells hold next to none, and the rest may not stand denser than ~3 per cell (fit_scale would shrink
# the cells) nor in less than half of the box along z (trim_box would cut the region off).
FRAMES = {
    # per-thread kernels: n / (dim_y dim_z) < 40.  Sites at x-cell 5, five across y
    "flat": dict(dims=(11, 50, None), dense=130, sparse=0, us=(5,), vs=(5, 14, 23, 32, 41),
                 boundary=dict(corner_under=(0, 0), corner_over=(10, 49), edge_under=(0, 9), edge_over=(10, 9), face_under=(5, 18), face_over=(5, 27))),
    # cooperative and brick kernels: n / (dim_y dim_z) >= 40 (44.7 here)
    "long": dict(dims=(32, 20, None), dense=170, sparse=60, us=(5, 14, 23), vs=(5, 14),
                 boundary=dict(corner_under=(0, 0), corner_over=(31, 19), edge_under=(0, 9), edge_over=(31, 9), face_under=(10, 18), face_over=(20, 18))),
}
LATTICE = 1.7
F_SITES = [("F", a, s, r, sound) for r in (1, 2, 3) for a in range(3) for s in (0, 1) for sound in (True, False)]
T_SITES = [("T_ring",), ("T_lanes", 2), ("T_lanes", 3), ("T_self",)]
R_SITES = [("R", k) for k in range(4)]
B_SITES = [("B", k) for k in ("corner_under", "corner_over", "edge_under", "edge_over", "face_under", "face_over")]
A_POINTS = {"F": 1, "T_ring": 1, "T_lanes": 4, "T_self": 3, "R": 1, "B": 1}
B_POINTS = {"F": 2, "T_ring": 2, "T_lanes": 3, "T_self": 1, "R": 2, "B": 1}


def scenario_name(spec):
    if spec[0] == "F":
        return f"F_{'xyz'[spec[1]]}{'-+'[spec[2]]}_r{spec[3]}_{'sound' if spec[4] else 'notlazy'}"
    return "_".join(str(v) for v in spec)


def r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def dyadic(v, bits=8):
    return np.rint(np.asarray(v, np.float64) * 2.0 ** bits) / 2.0 ** bits


def _pos(g, c, frac):
    return g.org + (np.asarray(c, np.float64) + np.asarray(frac, np.float64)) * g.h


def _axis(a, v=1.0):
    e = np.zeros(3)
    e[a] = v
    return e


def plant(g, spec, c, rng, fmt):
    """The points of one scenario around cell c of geometry g -> (points for the first cloud: the query first, points for the
    second cloud in row order, expectation dict).  fmt: (round the first cloud to fp32, round the second)."""
    kind = spec[0]
    exp = {}
    if kind == "F":
        _, a, s, r, sound = spec
        frac = np.full(3, 0.5)
        frac[a] = 0.75 if s else 0.25
        q = _pos(g, c, frac)
        Lr = (r + 0.25) * g.h[a]
        b = (a + 1) % 3
        if sound:
            true = q + _axis(a, (1.0 if s else -1.0) * (Lr + g.h[a] * OFF))
            decoy = q - _axis(b, Lr + 2.0 * g.h[a] * OFF)
            return [q], [decoy, true], dict(want=1, decoy=0, ring=r + 1, axis=a, side=s, r=r)
        near = q - _axis(b, Lr * (1.0 - OFF))
        spare = q + _axis(b, Lr + 0.2 * g.h[b])                  # (the second slot of the site: farther away, inside the cube)
        return [q], [near, spare], dict(want=0, ring=r, axis=a, side=s, r=r)
    if kind == "B":
        where, mode = spec[1].split("_")
        frac = np.full(3, 0.5)
        inward = None
        for a in range(3):
            if c[a] == 0:
                frac[a] = 0.9
            elif c[a] == g.dim[a] - 1:
                frac[a] = 0.1
            if c[a] in (0, g.dim[a] - 1):
                inward = _axis(a, 1.0 if c[a] == 0 else -1.0)
        q = _pos(g, c, frac)
        L1 = float(face_bounds(g, q)[0, 0])
        near = q + inward * L1 * (1.0 - OFF if mode == "under" else 1.0 + OFF)
        return [q], [near], dict(want=0, ring=1 if mode == "under" else 2, where=where)
    hm = float(g.h.min())
    if kind == "T_ring":                                          # 3-4-5 offsets on a 2^-8 lattice: both distances are (5k)^2 exactly
        k = float(dyadic(0.35 * hm))
        q = dyadic(_pos(g, c, (0.1, 0.2, 0.5)))
        return [q], [q + (0.0, -4 * k, 3 * k), q + (5 * k, 0.0, 0.0)], dict(want=0, ring=2, tie=[0, 1], rings_of=[2, 1])
    if kind == "T_lanes":
        r = spec[1]
        k = float(dyadic((0.35 if r == 2 else 0.55) * hm))
        q = dyadic(_pos(g, c, (0.5, 0.5, 0.5)))
        tied = [q + (0.0, 3 * k, 4 * k), q + (0.0, -4 * k, 3 * k), q + (0.0, 4 * k, -3 * k)]
        # the same three points in the first cloud, behind the query: the self search meets the tie too (SELF kernels: the query's
        # own record lies in the centre lane and is skipped), and each copy answers its twin at distance 0 in directions 0 and 1
        return [q] + tied, tied, dict(want=0, ring=r, tie=[0, 1, 2], self_ring=r, self_want=1)
    if kind == "T_self":
        q = dyadic(_pos(g, c, (0.5, 0.5, 0.5)))
        return [q, q, q], [q + (float(dyadic(1.75 * hm)), 0.0, 0.0)], dict(want=0, ring=2, dups=3)
    if kind == "R":
        return _plant_reversal(g, spec, c, rng, fmt)
    raise KeyError(kind)


def _plant_reversal(g, spec, c, rng, fmt):
    """A flagged query (true neighbour h 2^-10 .. 2^-9 beyond the +x face of the ring-3 cube) with a decoy inside the cube that is
    FARTHER in fp64 and NEARER (every other site: or equal) in the fp32 arithmetic of the rescan's filter, as brute_planted's family R."""
    import brute_planted as bp
    fa, fb = (r32 if fmt[0] else (lambda v: v)), (r32 if fmt[1] else (lambda v: v))
    a = spec[1] % 3
    for _ in range(64):
        frac = np.full(3, 0.5) + rng.uniform(-0.05, 0.05, 3)
        frac[a] = 0.75
        q = fa(_pos(g, c, frac))
        m = 4096
        lat = rng.uniform(-0.05, 0.05, (m, 3)) * g.h
        lat[:, a] = (3.25 + OFF * rng.uniform(1.0, 2.0, m)) * g.h[a]
        trues = fb(q + lat)
        rad = np.sqrt(dist64(q, trues))
        u = rng.normal(size=(m, 3))
        u[:, a] = -np.abs(u[:, a])                                 # away from the face the true neighbour lies behind
        u /= np.linalg.norm(u, axis=1)[:, None]
        decoys = fb(q + u * rng.uniform(rad.min(), rad.max(), (m, 1)))
        cand = np.vstack([trues, decoys])
        is_true = np.arange(2 * m) < m
        d64 = dist64(q, cand)
        d32 = bp.dist32(q.astype(np.float32), cand.astype(np.float32)).astype(np.float64)
        o = np.argsort(d64, kind="stable")
        d64, d32, cand, is_true = d64[o], d32[o], cand[o], is_true[o]
        # neighbours in fp64 order: a true point directly followed by a decoy that is strictly farther in fp64 and not farther in fp32
        ok = is_true[:-1] & ~is_true[1:] & (d64[1:] > d64[:-1]) & (d32[1:] <= d32[:-1])
        # the true point must be the nearest of the pair only: nothing else of the site is planted, so any such pair serves
        hit = np.flatnonzero(ok)
        if len(hit):
            gain = d32[hit] - d32[hit + 1]
            i = int(hit[gain.argmax()])
            return [q], [cand[i + 1], cand[i]], dict(want=1, decoy=0, ring=FLAGGED, reversed32=True, axis=a, side=1, r=3)
    raise AssertionError(f"{scenario_name(spec)}: no fp32 reversal found")


def frame_points(name, fmt, seed):
    """The background of a frame -> (first cloud's, second cloud's, n per cloud, layout); the probes' slots are not included."""
    f = FRAMES[name]
    sites = F_SITES + T_SITES + R_SITES
    per = len(f["us"]) * len(f["vs"])
    stations = -(-len(sites) // per)
    zr = f["dense"] + (2 + f["sparse"] if f["sparse"] else 0)      # where the reserved region starts
    W = zr + 9 * stations + 6 + 9
    D = np.array([f["dims"][0], f["dims"][1], W], np.float64)
    n = int(np.floor(PPC * np.prod(D) / 1.001))
    rng = np.random.default_rng(seed)
    pins = np.array([[x, y, z] for x in (0.0, D[0]) for y in (0.0, D[1]) for z in (0.0, D[2])])
    lat = [np.zeros((0, 3)), np.zeros((0, 3))]
    if f["sparse"]:
        z0 = f["dense"] + 2.0
        ax = [np.arange(0.4, D[0] - 1.2, LATTICE), np.arange(0.4, D[1] - 1.2, LATTICE), np.arange(z0 + 0.4, z0 + f["sparse"] - 1.2, LATTICE)]
        base = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
        lat = [base + rng.uniform(-0.08, 0.08, base.shape), base + LATTICE / 2 + rng.uniform(-0.08, 0.08, base.shape)]
    na_probe = sum(A_POINTS[s[0]] for s in sites + B_SITES)
    nb_probe = sum(B_POINTS[s[0]] for s in sites + B_SITES)
    out = []
    for k, nprobe in enumerate((na_probe, nb_probe)):
        nd = n - len(pins) - len(lat[k]) - nprobe
        dense = rng.uniform(0.0, 1.0, (nd, 3)) * (D[0], D[1], f["dense"])
        bg = np.vstack([pins, lat[k], dense])
        out.append(r32(bg) if fmt[k] else bg)
    return out[0], out[1], n, SimpleNamespace(D=D, zr=zr, stations=stations, sites=sites)


def site_cells(name, g, lay):
    """Cell of every scenario on geometry g: interior sites on a lattice of spacing 9 that starts 5 cells inside the region, boundary
    sites in the last layer of cells."""
    f = FRAMES[name]
    w0 = int(np.ceil((lay.zr - g.org[2]) * g.inv_h[2])) + 5
    top = int(g.dim[2]) - 1
    out = []
    k = 0
    for j in range(lay.stations):
        for u in f["us"]:
            for v in f["vs"]:
                if k < len(lay.sites):
                    out.append((lay.sites[k], np.array([u, v, w0 + 9 * j])))
                    k += 1
    last = w0 + 9 * (lay.stations - 1)
    assert last + 3 < top - 1 and top - last >= 9, f"the reserved region is too short on this grid: last station {last}, top {top}"
    assert max(f["us"]) + 3 < g.dim[0] - 1 and max(f["vs"]) + 3 < g.dim[1] - 1, "the cross-section is too small on this grid"
    for spec in B_SITES:
        u, v = f["boundary"][spec[1]]
        u, v = (g.dim[0] - 1 if u == f["dims"][0] - 1 else u), (g.dim[1] - 1 if v == f["dims"][1] - 1 else v)
        out.append((spec, np.array([u, v, top])))
    return out


def build(name, fmt, g=None, seed=7):
    """The case of frame `name` with clouds rounded to fp32 as fmt = (first, second) says, its probes placed on geometry g (default:
    the predicted one).  Background points whose decision would be UNDECIDED on g are nudged by 2^-6 of a cell (once; the caller
    asserts that none is left)."""
    bga, bgb, n, lay = frame_points(name, fmt, seed)
    rng = np.random.default_rng([seed, 1])
    for attempt in range(2):
        if g is None:
            # provisional: all probes at the centre of the region; the frame alone decides the geometry
            mid = np.array([lay.D[0] / 2, lay.D[1] / 2, lay.zr + 10.0])
            na = n - len(bga)
            nb = n - len(bgb)
            g = predict_geometry(np.vstack([bga, np.tile(mid, (na, 1))]), np.vstack([bgb, np.tile(mid, (nb, 1))]))
        pa, pb, sites = [], [], []
        for spec, c in site_cells(name, g, lay):
            qa, qb, exp = plant(g, spec, c, np.random.default_rng([seed, 2, len(sites)]), fmt)
            qa, qb = [r32(p) if fmt[0] else np.asarray(p, np.float64) for p in qa], [r32(p) if fmt[1] else np.asarray(p, np.float64) for p in qb]
            assert len(qa) == A_POINTS[spec[0]] and len(qb) == B_POINTS[spec[0]]
            sites.append(SimpleNamespace(name=scenario_name(spec), spec=spec, cell=c, qrow=len(bga) + len(pa), arows=[len(bga) + len(pa) + i for i in range(len(qa))],
                                         brows=[len(bgb) + len(pb) + i for i in range(len(qb))], **exp))
            pa += qa
            pb += qb
        a, b = np.vstack([bga] + [np.array(pa)]), np.vstack([bgb] + [np.array(pb)])
        assert len(a) == n and len(b) == n
        case = SimpleNamespace(name=f"{name}_{'32' if fmt[0] else '64'}{'32' if fmt[1] else '64'}", frame=name, fmt=fmt, a=np.ascontiguousarray(a),
                               b=np.ascontiguousarray(b), geom=g, sites=sites, truth={}, two={}, layout=lay, n_background=(len(bga), len(bgb)))
        if attempt == 1:
            return case
        moved = 0
        for d in (0, 1, 2):
            und = predict(case, d).undecided
            cloud = bgb if d == 1 else bga
            und = und[und < len(cloud)]
            und = und[und >= 8]                                     # never a pin
            step = rng.uniform(-1.0, 1.0, (len(und), 3)) * g.h * 2.0 ** -6
            moved_to = np.clip(cloud[und] + step, 0.0, lay.D)
            cloud[und] = r32(moved_to) if fmt[1 if d == 1 else 0] else moved_to
            moved += len(und)
        if moved == 0:
            return case
    return case


# ---- X: the trimmed box -----------------------------------------------------------------------------------------------------------
TRIM_BINS = 1024                           # kTrimBins


def trim_box(a, b):
    """trim_box(): the per-axis [0.1 %, 99.9 %] quantile box of both clouds over coarse histograms, repeated while an axis keeps
    halving -> (lo, hi, boxed)."""
    pts = np.vstack([np.asarray(a, np.float64), np.asarray(b, np.float64)])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    lo0, hi0 = lo.copy(), hi.copy()
    allow = int(len(pts) * 1.0e-3)
    for _ in range(8):
        shrunk = False
        for ax in range(3):
            if not hi[ax] > lo[ax]:
                continue
            iw = TRIM_BINS / (hi[ax] - lo[ax])
            t = np.clip((pts[:, ax] - lo[ax]) * iw, 0.0, TRIM_BINS - 1.0).astype(np.int64)
            h = np.bincount(t, minlength=TRIM_BINS)
            b0, b1, acc = 0, TRIM_BINS - 1, 0
            while b0 < b1 and acc + h[b0] <= allow:
                acc += h[b0]
                b0 += 1
            acc = 0
            while b1 > b0 and acc + h[b1] <= allow:
                acc += h[b1]
                b1 -= 1
            w = (hi[ax] - lo[ax]) / TRIM_BINS
            nlo, nhi = lo[ax] + b0 * w, lo[ax] + (b1 + 1) * w
            shrunk |= bool((nhi - nlo) < 0.5 * (hi[ax] - lo[ax]))
            lo[ax], hi[ax] = nlo, min(nhi, hi[ax])
        if not shrunk:
            break
    return lo, hi, bool(np.any((hi - lo) < 0.5 * (hi0 - lo0)))


# A body as in frame "flat" with dense zones at both ends of z and the reserved region between them (so that the quantile cuts fall
# into background), six pins 1000 units outside (they fix the bounding boxes) and X_STRAY stray points per side, axis and cloud,
# 100 .. 900 units outside; every second stray point of the first cloud has a partner of the second cloud beside it.
X_D, X_ZONES, X_STRAY, X_FAR = (11.0, 50.0, 186.0), (70.0, 116.0), 30, 1000.0
# name -> (kind, axis, side, cell of the site's slot: (x, y, station); -1: the last cell of the axis)
X_SITES = {
    "X2_x-": ("X2", 0, 0, (0, 5, 0)), "X3_x-": ("X3", 0, 0, (0, 14, 0)), "X3far_x-": ("X3far", 0, 0, (0, 23, 0)), "X1_x-": ("X1", 0, 0, (0, 32, 0)),
    "X2_y+": ("X2", 1, 1, (5, -1, 0)),
    "X1_x+": ("X1", 0, 1, (-1, 14, 1)), "X3_y+": ("X3", 1, 1, (5, -1, 1)), "X1_y-": ("X1", 1, 0, (5, 0, 1)),
    "X4_--": ("X4", (0, 1), 0, (0, 0, 2)), "X4_++": ("X4", (0, 1), 1, (-1, -1, 2)), "X1_y+": ("X1", 1, 1, (0, -1, 2)),
    "X1_z-": ("X1", 2, 0, (5, 23, None)), "X1_z+": ("X1", 2, 1, (5, 23, None)),
}
X_RING = {"X1": 1, "X2": 3, "X3": 3, "X3far": FLAGGED, "X4": 1}


def plant_x(g, kind, axis, side, c):
    """X1: a stray point of each cloud 300 cells outside, 0.37 h apart: both clamp into the same boundary cell, ring 1 settles.
    X2: a query 2.6 h outside whose neighbour is 0.4 h inside the box: found in the query's OWN cell, settled only at ring 3.
    X3: a query 2.5 h inside whose neighbour lies 0.4 h outside and clamps into the boundary cell two cells away (ring 3);
    X3far: ... 3 h outside (5.5 h away: flagged, the rescan finds it).  X4: as X1, outside on two axes at once."""
    lo, hi = g.org, g.org + g.dim * g.h
    q = _pos(g, c, (0.5, 0.5, 0.5))
    out_ = -1.0 if side == 0 else 1.0
    face = (lo if side == 0 else hi)
    near = q.copy()
    if kind in ("X1", "X4"):
        for k, ax in enumerate((axis,) if kind == "X1" else axis):
            q[ax] = face[ax] + out_ * (300.0 - 100.0 * k) * g.h[ax]
        near = q + (0.3, 0.2, 0.1) * g.h
    else:
        qa, na = {"X2": (2.6, -0.4), "X3": (-2.5, 0.4), "X3far": (-2.5, 3.0)}[kind]
        q[axis], near[axis] = face[axis] + out_ * qa * g.h[axis], face[axis] + out_ * na * g.h[axis]
    return q, near


def build_trim(fmt, g=None, seed=9):
    """The X case: clouds rounded to fp32 as fmt says, probes placed on geometry g (default: predicted through trim_box())."""
    D = np.array(X_D)
    n = int(np.floor(PPC * np.prod(D) / 1.001))
    rng = np.random.default_rng(seed)
    mid = D / 2
    pins = np.array([[x, y, z] for x in (0.0, D[0]) for y in (0.0, D[1]) for z in (0.0, D[2])])
    far = np.array([mid + _axis(ax, sgn * (X_FAR + D[ax] / 2)) for ax in range(3) for sgn in (-1.0, 1.0)])
    stray = []
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            p = rng.uniform(0.0, 1.0, (X_STRAY, 3)) * D
            p[:, ax] = (0.0 if sgn < 0 else D[ax]) + sgn * rng.uniform(100.0, 900.0, X_STRAY)
            stray.append(p)
    stray = np.vstack(stray)
    partner = stray + np.where(np.arange(len(stray))[:, None] % 2 == 0, rng.uniform(-0.4, 0.4, stray.shape), rng.uniform(-60.0, 60.0, stray.shape))
    nfixed = len(pins) + len(far) + len(stray)
    bgs = []
    for k in range(2):
        nd = n - nfixed - len(X_SITES)
        dense = rng.uniform(0.0, 1.0, (nd, 3)) * D
        z = rng.uniform(0.0, X_ZONES[0] + D[2] - X_ZONES[1], nd)
        dense[:, 2] = np.where(z < X_ZONES[0], z, z - X_ZONES[0] + X_ZONES[1])
        bg = np.vstack([pins, far, stray if k == 0 else np.clip(partner, mid - X_FAR - D / 2, mid + X_FAR + D / 2), dense])
        bgs.append(r32(bg) if fmt[k] else bg)
    for attempt in range(2):
        if g is None:
            prov = np.tile(mid, (len(X_SITES), 1))
            a0, b0 = np.vstack([bgs[0], prov]), np.vstack([bgs[1], prov])
            blo, bhi, boxed = trim_box(a0, b0)
            assert boxed
            g = predict_geometry(a0, b0, box=(blo, bhi))
        w0 = int(np.ceil((X_ZONES[0] - g.org[2]) * g.inv_h[2])) + 5
        assert g.org[2] + (w0 + 18 + 5) * g.h[2] < X_ZONES[1], "the reserved region is too short on this grid"
        pa, pb, sites = [], [], []
        for name, (kind, axis, side, slot) in X_SITES.items():
            c = np.array([g.dim[0] - 1 if slot[0] < 0 else slot[0], g.dim[1] - 1 if slot[1] < 0 else slot[1],
                          (0 if side == 0 else g.dim[2] - 1) if slot[2] is None else w0 + 9 * slot[2]])
            q, near = plant_x(g, kind, axis, side, c)
            q, near = (r32(q) if fmt[0] else q), (r32(near) if fmt[1] else near)
            sites.append(SimpleNamespace(name=name, spec=(kind, axis, side), cell=c, qrow=len(bgs[0]) + len(pa), arows=[len(bgs[0]) + len(pa)],
                                         brows=[len(bgs[1]) + len(pb)], want=0, ring=X_RING[kind]))
            pa.append(q)
            pb.append(near)
        a, b = np.vstack([bgs[0], np.array(pa)]), np.vstack([bgs[1], np.array(pb)])
        case = SimpleNamespace(name=f"trim_{'32' if fmt[0] else '64'}{'32' if fmt[1] else '64'}", frame="trim", fmt=fmt, a=np.ascontiguousarray(a),
                               b=np.ascontiguousarray(b), geom=g, sites=sites, truth={}, two={}, n_fixed=nfixed, n_background=(len(bgs[0]), len(bgs[1])))
        if attempt == 1:
            return case
        moved = 0
        for d in (0, 1, 2):
            cloud = bgs[1] if d == 1 else bgs[0]
            und = predict(case, d).undecided
            und = und[(und >= nfixed) & (und < len(cloud))]           # dense background only
            to = np.clip(cloud[und] + rng.uniform(-1.0, 1.0, (len(und), 3)) * g.h * 2.0 ** -6, 0.0, D)
            cloud[und] = r32(to) if fmt[1 if d == 1 else 0] else to
            moved += len(und)
        if moved == 0:
            return case
    return case


# ---- small cases: planar, collinear and tiny pairs (B) ----------------------------------------------------------------------------
# name -> (points of the first cloud, of the second, shape, the ring-1 kernel the pair must take)
SMALL = {"tiny_3": (3, 3, "cube", "thread"), "tiny_40": (40, 37, "cube", "thread"), "tiny_300": (300, 280, "cube", "thread"),
         "planar_1000": (1000, 950, "plane", "thread"), "collinear_y_400": (400, 380, "line_y", "thread"),
         "slab_3000": (3000, 2900, "slab", "thread"), "collinear_x_500": (500, 500, "line_x", "coop")}
LINE_DENSE, LINE_LATTICE, LINE_STEP = 440, 60, 0.015


def small_case(name):
    """Random fp64 pairs whose grids have dim = 1 on one axis (plane), on two (lines along y and along x), a few cells per axis
    (cube: every ring-3 cube covers the grid, so L == inf settles whatever d is) or two cells on one axis (slab).  A line along y
    has one point per x-row and takes the per-thread kernel, as the short-in-x plane and slab do; a line along x is ONE x-row
    and takes the cooperative kernel: there both clouds share a dense stretch [0, 1] of alternating gaps and each has a stretch of its own where
    its points stand 1.8 cells apart and the other cloud has none (nothing there settles at ring 1 in any direction: `lo`)."""
    n, m, shape, _ = SMALL[name]
    rng = np.random.default_rng([11, sorted(SMALL).index(name)])
    a, b = rng.uniform(0.0, 1.0, (n, 3)), rng.uniform(0.0, 1.0, (m, 3))
    for k, p in enumerate((a, b)):
        if shape in ("plane", "line_x", "line_y"):
            p[:, 2] = 0.25
        if shape in ("plane", "slab"):
            p[:, 0] *= 0.3
        if shape == "line_y":
            p[:, 0] = 7.0
        if shape == "slab":
            p[:, 2] *= 0.03
        if shape == "line_x":
            p[:, 1] = -3.0
            start = 1.05 + k * (LINE_LATTICE * LINE_STEP + 0.05)
            p[LINE_DENSE:, 0] = start + LINE_STEP * (np.arange(LINE_LATTICE) + rng.uniform(-0.03, 0.03, LINE_LATTICE))
            # the shared stretch: gaps alternate 0.8 and 1.2 of the mean, the second cloud stands a quarter of it to the right, so no
            # query there has its two nearest candidates at nearly the same distance (on random data in ONE x-row every sixth has)
            delta = 1.0 / LINE_DENSE
            gaps = np.where(np.arange(LINE_DENSE) % 2 == 0, 0.8, 1.2) * delta
            p[:LINE_DENSE, 0] = np.cumsum(gaps) - gaps[0] + 0.25 * delta * k + rng.uniform(-0.01, 0.01, LINE_DENSE) * delta
    return SimpleNamespace(name=name, frame=None, fmt=(False, False), a=a, b=b, geom=predict_geometry(a, b), sites=[], truth={}, two={})


# ---- the long tail ---------------------------------------------------------------------------------------------------------------
LONG_TAIL_D, LONG_TAIL_SLABS, LONG_TAIL_ISOLATED = 79.0, 20, 24


def long_tail_case(g=None, seed=5):
    """Two fp32 clouds in alternating slabs LONG_TAIL_D / LONG_TAIL_SLABS = 3.95 cells thick along z: a point deeper than ~1.5 cells
    inside its slab has no neighbour of the other cloud within ring 1's reach, and none is deeper than 2, so nearly all of them
    settle by ring 3.  Queries UNDECIDED on g are nudged by 2^-6 of a cell, once."""
    D, S, K = LONG_TAIL_D, LONG_TAIL_SLABS, LONG_TAIL_ISOLATED
    t = D / S
    n = int(np.floor(PPC * D ** 3 / 1.001))
    rng = np.random.default_rng(seed)
    out = []
    for k in range(2):
        p = rng.uniform(0.0, 1.0, (n, 3)) * (D, D, t)
        slab = 2 * rng.integers(0, S // 2, n) + k
        # the first and the last slab of the box have one neighbouring slab only: they keep the half that faces it ...
        p[:, 2] = np.where((slab == 0), t / 2 + p[:, 2] / 2, np.where(slab == S - 1, p[:, 2] / 2, p[:, 2])) + slab * t
        # ... and K points of the first cloud lie on the box's floor, K of the second under its ceiling: nothing of the other cloud
        # within 3.6 cells of them in z, so three rings cannot settle them and the rescan half of the launch has work to wait for
        iso = rng.uniform(0.0, 1.0, (K, 3)) * (D - 10.0, D - 10.0, 0.3) + (5.0, 5.0, 0.0 if k == 0 else D - 0.3)
        p[2:2 + K] = iso
        p[0], p[1] = ((0.0, 0.0, 0.0), (D, D, (S - 1) * t)) if k == 0 else ((D, 0.0, t), (0.0, D, D))
        out.append(r32(p))
    a, b = out
    g = predict_geometry(a, b) if g is None else g
    case = SimpleNamespace(name="long_tail", frame=None, fmt=(True, True), a=a, b=b, geom=g, sites=[], truth={}, two={})
    moved = 0
    for d, cloud in ((0, a), (1, b)):
        und = predict(case, d).undecided
        und = und[und >= 2 + K]
        cloud[und] = r32(np.clip(cloud[und] + rng.uniform(-1.0, 1.0, (len(und), 3)) * g.h * 2.0 ** -6, (0.0, 0.0, t), (D, D, (S - 1) * t)))
        moved += len(und)
    if moved:
        case.truth, case.two = {}, {}
    return case


@functools.lru_cache(maxsize=None)
def cached(kind, *args):
    """Cases on their predicted geometry, built once per process (the host proofs share them)."""
    return {"frame": build, "small": small_case, "long_tail": long_tail_case, "trim": build_trim}[kind](*args)
