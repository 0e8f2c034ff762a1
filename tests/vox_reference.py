"""Planted integer cases for the voxel-brick search (open_pcc_metric_amd/csrc/pccm_vox.hip) and the per-thread lattice search
(pccm_lattice.hip), and the exact reference they are held to.  Host only, NumPy only; shares no code with oracle/ or
tests/nn_reference.py.

The reference is an int64 brute force over every (query, searched point) pair.  Per query it gives the smallest row among the
nearest points (the library's tie rule, include/pccm.h), the squared distance, and `nvox`, the number of DISTINCT voxels at
exactly that distance.  The last one is what makes the split of work between k_vox_query and the tail kernels predictable:

* a best d2 <= 64 is final (every voxel within 8 of a query lies inside the staged 24^3), anything farther goes to the tail;
* with matched rows, at most kVoxTies = 12 equidistant nearest voxels are served by the bricks, 13 or more go to the tail.

The families.  Every probe is one query in a neighbourhood of its own, on a coarse lattice of pitch 48 voxels (6 cells), so
probes never see each other.  The pair's grid starts at the pair's bounding-box minimum and has cells of 8^3 voxels, so the
lowest point of each axis decides every query's in-cell offset: a family pins it with probes whose lowest point lies 8 below
their query (family A), or with an anchor probe -- a query and a searched point in the voxel at the box's corner.  Everything
else sits at least one lattice site further in.  Searched rows are shuffled with a fixed seed; inside a probe the shuffled rows
are handed out in the order the generator lists the points, so it decides which voxel holds the smallest row."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

PITCH = 48                 # voxels between probes: a multiple of 8, six cells
VOX_REACH2 = 64            # the bricks vouch for 8 voxels
VOX_TIES = 12              # kVoxTies
MAX_RING = 3               # kMaxRing: rings of cells the per-thread kernels walk before the exact rescan

B_NEAR = (1, 2, 3, 5, 6, 9, 14, 16)        # tie distances out of c_vox_near
B_WALK = (17, 18, 26, 41, 50, 64)          # ... and out of the sqrtf walk


# ---- the reference ------------------------------------------------------------------------------------------------------
def _as_int(a):
    a = np.asarray(a)
    i = a.astype(np.int64)
    assert a.ndim == 2 and a.shape[1] == 3 and np.array_equal(i, a), "integer (N, 3) coordinates expected"
    return i


def brute_nn(queries, searched, skip_same_index=False, tile=1 << 19):
    """-> (row, d2, nvox): int64 brute force.  row: smallest row among the nearest points of `searched`; d2: the squared distance;
    nvox: distinct voxels of `searched` at exactly d2.  skip_same_index: row i of the queries is row i of the searched cloud and
    does not count (the self search); its voxel does when it holds another point."""
    q, s = _as_int(queries), _as_int(searched)
    n, m = len(q), len(s)
    first = np.zeros(m, dtype=bool)                       # the first row of every distinct voxel
    first[np.unique(s, axis=0, return_index=True)[1]] = True
    row, d2, nvox = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.int64)
    step = max(1, tile // max(m, 1))
    big = np.iinfo(np.int64).max
    for i0 in range(0, n, step):
        i1 = min(n, i0 + step)
        d = q[i0:i1, None, 0] - s[None, :, 0]
        acc = d * d
        for a in (1, 2):
            d = q[i0:i1, None, a] - s[None, :, a]
            acc += d * d
        if skip_same_index:
            acc[np.arange(i1 - i0), np.arange(i0, i1)] = big
        best = acc.min(axis=1)
        row[i0:i1] = acc.argmin(axis=1)                   # the first minimum: the smallest row
        d2[i0:i1] = best
        hit = acc == best[:, None]
        cnt = (hit & first[None, :]).sum(axis=1)
        if skip_same_index:                               # distance 0: the one voxel is the query's own (its first row may be the query)
            cnt = np.where(best == 0, 1, cnt)
        nvox[i0:i1] = cnt
    return row, d2, nvox


def predicted_tail(d2, nvox, rows):
    """Queries k_vox_query hands to the tail kernels: rows=False for <false, false> and <true, false>, True for <false, true>."""
    d2, nvox = np.asarray(d2), np.asarray(nvox)
    return (d2 > VOX_REACH2) | (nvox > VOX_TIES) if rows else d2 > VOX_REACH2


def cell_coords(points, org, h, dim):
    """Per-axis cell of every point, as float64 whole numbers: the arithmetic of cell_coord in pccm_grid.h -- the subtraction and
    the multiplication by inv_h = 1 / h each rounded once, floor, clamp to [0, dim - 1]."""
    q = np.asarray(points, dtype=np.float64)
    org, h, dim = np.asarray(org, np.float64), np.asarray(h, np.float64), np.asarray(dim, np.int64)
    inv_h = 1.0 / h
    return np.clip(np.floor((q - org) * inv_h), 0, dim - 1)


def lattice_fallback(queries, d2, org, h, dim):
    """Queries the per-thread kernels leave to the exact rescan: the nearest neighbour lies beyond MAX_RING cells of the grid
    (org, h, dim as pccm_grid_geometry reports them).  The arithmetic of cell_coord / face_bound / settled_by in pccm_grid.h."""
    q = np.asarray(queries, dtype=np.float64)
    org, h, dim = np.asarray(org, np.float64), np.asarray(h, np.float64), np.asarray(dim, np.int64)
    slack = (np.abs(org) + (dim + 2) * h) * 2.0 ** -48
    c = cell_coords(q, org, h, dim)
    bound = np.full(len(q), np.inf)
    for a in range(3):
        lo = np.where(c[:, a] - MAX_RING > 0, (q[:, a] - (org[a] + (c[:, a] - MAX_RING) * h[a])) - slack[a], np.inf)
        hi = np.where(c[:, a] + MAX_RING < dim[a] - 1, ((org[a] + (c[:, a] + MAX_RING + 1) * h[a]) - q[:, a]) - slack[a], np.inf)
        bound = np.minimum(bound, np.minimum(lo, hi))
    settled = np.isinf(bound) | ((bound > 0.0) & (np.asarray(d2, np.float64) < bound * bound * (1.0 - 2.0 ** -30)))
    return ~settled


# ---- integer vectors of a given length --------------------------------------------------------------------------------------
def vectors_upto(limit):
    """Every integer vector with |v|^2 <= limit, (0, 0, 0) included, in a fixed order."""
    r = int(np.floor(np.sqrt(limit)))
    g = np.arange(-r, r + 1)
    v = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return v[(v * v).sum(axis=1) <= limit]


def vectors_at(d2):
    v = vectors_upto(d2)
    return v[(v * v).sum(axis=1) == d2]


def r3(d2):
    """In how many ways d2 is a sum of three squares (signs and order count)."""
    return len(vectors_at(d2))


# ---- a family -------------------------------------------------------------------------------------------------------------
@dataclass
class Family:
    name: str
    queries: np.ndarray                       # cloud 0, (N, 3) float32 integers
    searched: np.ndarray                      # cloud 1, (M, 3) float32 integers
    org: np.ndarray                           # the grid origin the generator planned: the pair's bounding-box minimum
    dims: np.ndarray                          # ... and its cells of 8^3 voxels per axis
    offsets: Optional[np.ndarray] = None      # (N, 3) planned in-cell offset of every query
    d2: Optional[np.ndarray] = None           # by construction, queries against searched: squared distance,
    row: Optional[np.ndarray] = None          # ... matched row (-1: the construction leaves it to the brute force)
    nvox: Optional[np.ndarray] = None         # ... distinct nearest voxels
    qprobe: Optional[np.ndarray] = None       # lattice families: the probe every query / searched point belongs to
    sprobe: Optional[np.ndarray] = None
    _ref: dict = field(default_factory=dict, repr=False)

    def reference(self, direction):
        """(row, d2, nvox) of direction 0 (queries against searched), 1 (the reverse) or 2 (queries against themselves)."""
        if direction not in self._ref:
            if direction == 0:
                self._ref[0] = brute_nn(self.queries, self.searched)
            elif direction == 1:
                self._ref[1] = brute_nn(self.searched, self.queries)
            else:
                self._ref[2] = brute_nn(self.queries, self.queries, skip_same_index=True)
        return self._ref[direction]

    def cloud(self, direction):
        """(iterating, searched) clouds of a direction."""
        return ((self.queries, self.searched), (self.searched, self.queries), (self.queries, self.queries))[direction]

    def ncells(self):
        return int(np.prod(self.dims))

    def realised_offsets(self, org=None):
        return (self.queries.astype(np.int64) - (self.org if org is None else np.asarray(org).astype(np.int64))) % 8


def _finish(name, queries, searched, org, offsets=None, d2=None, row=None, nvox=None):
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    searched = np.ascontiguousarray(searched, dtype=np.float32)
    lo = np.minimum(queries.min(axis=0), searched.min(axis=0)).astype(np.int64)
    hi = np.maximum(queries.max(axis=0), searched.max(axis=0)).astype(np.int64)
    org = np.asarray(org, dtype=np.int64)
    assert np.array_equal(lo, org), f"{name}: the bounding box starts at {lo}, planned {org}"
    fam = Family(name, queries, searched, org, (hi - lo) // 8 + 1, offsets, d2, row, nvox)
    if offsets is not None:
        assert np.array_equal(fam.realised_offsets(), offsets), f"{name}: in-cell offsets"
    return fam


@dataclass
class Probe:
    """One query at in-cell offset `o` and the points planted around it, relative to the QUERY, in ascending row order."""
    o: tuple
    pts: np.ndarray
    d2: int = -1
    winner: int = -1          # index into pts of the point whose row is expected (-1: left to the brute force)
    nvox: int = -1


def place(name, probes, seed, pins=None, origin=(0, 0, 0)):
    """Put the probes on the lattice.  pins: three probes whose lowest points lie 8 below their query's cell in x, y and z: they
    take the sites (0, 1, 1), (1, 0, 1), (1, 1, 0) and fix the grid's origin; without pins an anchor probe (query and searched point in
    one voxel, in-cell offset 0) takes the site (0, 0, 0).  Everybody else sits at sites >= 1 on every axis."""
    rng = np.random.default_rng(seed)
    probes = list(probes)
    if pins is None:
        probes.append(Probe((0, 0, 0), np.zeros((1, 3), np.int64), 0, 0, 1))
        special = {len(probes) - 1: (0, 0, 0)}
        base = 0
    else:
        special = {pins[0]: (0, 1, 1), pins[1]: (1, 0, 1), pins[2]: (1, 1, 0)}
        base = 8
    rest = [i for i in range(len(probes)) if i not in special]
    side = 1
    while side ** 3 < len(rest):
        side += 1
    sites = np.stack(np.meshgrid(*([np.arange(1, side + 1)] * 3), indexing="ij"), axis=-1).reshape(-1, 3)
    site_of = np.zeros((len(probes), 3), np.int64)
    site_of[rest] = sites[: len(rest)]
    for i, s in special.items():
        site_of[i] = s
    off = np.array([p.o for p in probes], np.int64)
    qpos = site_of * PITCH + base + off + np.asarray(origin, np.int64)
    counts = np.array([len(p.pts) for p in probes])
    owner = np.repeat(np.arange(len(probes)), counts)
    pts = np.concatenate([np.asarray(p.pts, np.int64).reshape(-1, 3) for p in probes]) + qpos[owner]
    m = len(pts)
    # shuffled rows; a probe's rows in ascending order go to its points as listed
    slots = np.sort(owner * m + rng.permutation(m)) % m
    searched = np.empty((m, 3), np.int64)
    searched[slots] = pts
    start = np.concatenate([[0], np.cumsum(counts)])
    qrow = rng.permutation(len(probes))
    queries = np.empty((len(probes), 3), np.int64)
    queries[qrow] = qpos
    offsets = np.empty_like(queries)
    offsets[qrow] = off
    d2, row, nvox = (np.full(len(probes), -1, np.int64) for _ in range(3))
    for i, p in enumerate(probes):
        d2[qrow[i]] = p.d2
        nvox[qrow[i]] = p.nvox
        if p.winner >= 0:
            row[qrow[i]] = slots[start[i] + p.winner]
    fam = _finish(name, queries, searched, origin, offsets, d2, row, nvox)
    fam.qprobe = np.argsort(qrow)
    fam.sprobe = np.empty(m, np.int64)
    fam.sprobe[slots] = owner
    return fam


def _sign_step(v):
    return v + np.sign(v)


# ---- family A: every offset once -------------------------------------------------------------------------------------------
def family_a():
    """Every integer vector with 0 < |v|^2 <= 81, from query in-cell offsets (0, 0, 0), (7, 7, 7) and a seeded random one: one target
    at q + v and a strictly farther decoy on the opposite side, at q - (v + sign(v))."""
    rng = np.random.default_rng(101)
    vs = vectors_upto(81)
    vs = vs[(vs * vs).sum(axis=1) > 0]
    probes, pins = [], [None, None, None]
    for v in vs:
        for o in ((0, 0, 0), (7, 7, 7), tuple(int(x) for x in rng.integers(0, 8, 3))):
            if o == (0, 0, 0) and int(np.abs(v).sum()) == 7 and int(v.max()) == 7:      # (7, 0, 0), (0, 7, 0), (0, 0, 7): decoy 8 below
                pins[int(np.argmax(v))] = len(probes)
            probes.append(Probe(o, np.stack([v, -_sign_step(v)]), int((v * v).sum()), 0, 1))
    return place("A", probes, 102, pins=pins)


# ---- family B: ties ---------------------------------------------------------------------------------------------------------
def tie_counts(d2):
    r = r3(d2)
    return sorted({t for t in (2, 11, 12, 13, r) if t <= r})


def family_b():
    """T equidistant nearest voxels out of the r3(d2) vectors of that length; the smallest row cycles through the vectors."""
    rng = np.random.default_rng(201)
    probes = []
    for d2 in B_NEAR + B_WALK:
        vs = vectors_at(d2)
        r = len(vs)
        stride = 1 if d2 <= 16 else -(-r // 12)
        for t in tie_counts(d2):
            for k in range(0, r, stride):
                pts = vs[(k + np.arange(t)) % r]             # the first one listed takes the smallest row
                probes.append(Probe(tuple(int(x) for x in rng.integers(0, 8, 3)), pts, d2, 0, t))
    return place("B", probes, 202)


# ---- family C: nothing farther is taken for a hit -----------------------------------------------------------------------------
def family_c():
    """Per representable d2 <= 64 one probe whose searched points are EVERY voxel with |v|^2 >= d2 inside Chebyshev radius 8; every
    farther voxel has a smaller row than every nearest one."""
    rng = np.random.default_rng(301)
    g = np.arange(-8, 9)
    box = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    n2 = (box * box).sum(axis=1)
    probes = []
    for d2 in range(1, 65):
        near = box[n2 == d2]
        if len(near) == 0:
            continue
        far = box[n2 > d2]
        far = far[rng.permutation(len(far))]
        near = near[rng.permutation(len(near))]
        probes.append(Probe(tuple(int(x) for x in rng.integers(0, 8, 3)), np.concatenate([far, near]), d2, len(far), len(near)))
    return place("C", probes, 302)


# ---- family D: points per voxel ---------------------------------------------------------------------------------------------
D_MULT = (1, 2, 3, 70)


def family_d():
    """Ties of family B whose voxels hold 1, 2, 3 and 70 points at scattered rows: the voxel with the smallest row wins."""
    rng = np.random.default_rng(401)
    probes = []
    for d2 in (1, 2, 3, 5, 6, 9, 14, 16, 17, 26, 41, 64):
        vs = vectors_at(d2)
        r = len(vs)
        for t in sorted({2, min(12, r)}):
            for k in range(0, r, -(-r // 4)):
                vox = vs[(k + np.arange(t)) % r]
                mult = np.array([D_MULT[(k + j) % 4] for j in range(t)])
                body = np.repeat(np.arange(t), mult)
                first = int(np.flatnonzero(body == 0)[0])
                body = np.delete(body, first)
                body = body[rng.permutation(len(body))]     # the winner's first point, then everybody else in any order
                pts = vox[np.concatenate([[0], body])]
                probes.append(Probe(tuple(int(x) for x in rng.integers(0, 8, 3)), pts, d2, 0, t))
    return place("D", probes, 402)


D_SELF_STEPS = ((1, 0, 0), (0, -1, 0), (0, 0, 1), (-1, 1, 0), (1, 0, -1), (-1, -1, 1), (2, 0, 0), (0, 2, -1), (-3, 0, 0), (2, 2, 1),
                (0, -4, 0), (-8, 0, 0), (0, 7, -3), (5, -5, 3), (8, 0, 0), (-6, 6, 0))


def family_d_self():
    """One cloud, searched against itself and against a reshuffled copy: pairs of voxels A and A + v that hold 1, 2 or 3 points each.
    The self search finds distance 0 exactly where another point shares the voxel."""
    rng = np.random.default_rng(411)
    probes = []
    for v in D_SELF_STEPS:
        for a in (1, 2, 3):
            for b in (1, 2, 3):
                pts = np.concatenate([np.zeros((a, 3), np.int64), np.tile(np.array(v, np.int64), (b, 1))])
                probes.append(Probe(tuple(int(x) for x in rng.integers(0, 8, 3)), pts[rng.permutation(a + b)]))
    whole = place("Dself_points", probes, 412)
    cloud = whole.searched                                  # every planted point, the anchor's included
    fam = _finish("Dself", cloud[rng.permutation(len(cloud))], cloud, whole.org)
    return fam


# ---- family E: crowded --------------------------------------------------------------------------------------------------------
def family_e(name="E", ncell=3):
    """`ncell` x-adjacent cells, fully occupied, three points per voxel (three cells: 4608 records in one tile, 1536 queries per
    cell), against the same block with a checkerboard of voxels removed and shifted by one voxel along x.  Four cells: the last
    cell's per-voxel rows lie beyond the first 4096 entries of the tile, in the second piece k_vox_bricks sorts out."""
    rng = np.random.default_rng(501 + ncell)
    g = np.stack(np.meshgrid(np.arange(8 * ncell), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3)
    queries = np.repeat(g, 3, axis=0)
    kept = g[g.sum(axis=1) % 2 == 1] + np.array([1, 0, 0])
    searched = np.repeat(kept, 3, axis=0)
    return _finish(name, queries[rng.permutation(len(queries))], searched[rng.permutation(len(searched))], (0, 0, 0))


# ---- family F: borders and small grids ----------------------------------------------------------------------------------------
def _border_cells(dims):
    """The 8 corner cells, one cell in the middle of each of the 12 edges and of the 6 faces of an odd-sided grid: no two adjacent."""
    axes = [(0, d // 2, d - 1) for d in dims]
    cells = [(x, y, z) for x in axes[0] for y in axes[1] for z in axes[2]]
    mid = tuple(d // 2 for d in dims)
    return [c for c in cells if c != mid]


def family_f(name, dims, cells=None, origin=(0, 0, 0), seed=601):
    """On a grid of exactly `dims` cells: from every cell of `cells` one probe per direction d in {-1, 0, 1}^3 whose neighbour cell
    exists.  The query sits at in-cell 0 / 3 (4 in odd cells) / 7 for d = -1 / 0 / +1 on each axis and the target at q + d, in the
    neighbour cell.  Two anchor probes (query and searched point in one voxel) hold the box's two corners."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, np.int64)
    cells = _border_cells(dims) if cells is None else cells
    q, t = [np.zeros(3, np.int64), 8 * dims - 1], [np.zeros(3, np.int64), 8 * dims - 1]
    d2 = [0, 0]
    dirs = np.stack(np.meshgrid(*([np.arange(-1, 2)] * 3), indexing="ij"), axis=-1).reshape(-1, 3)
    for c in cells:
        c = np.asarray(c, np.int64)
        mid = 3 + int(c.sum()) % 2
        for d in dirs:
            if np.any(c + d < 0) or np.any(c + d >= dims):
                continue
            o = np.where(d < 0, 0, np.where(d > 0, 7, mid))
            q.append(8 * c + o)
            t.append(8 * c + o + d)
            d2.append(int((d * d).sum()))
    q, t = np.array(q) + np.asarray(origin, np.int64), np.array(t) + np.asarray(origin, np.int64)
    qrow, trow = rng.permutation(len(q)), rng.permutation(len(t))
    queries, searched = np.empty_like(q), np.empty_like(t)
    queries[qrow], searched[trow] = q, t
    want_d2, want_row = np.empty(len(q), np.int64), np.empty(len(q), np.int64)
    want_d2[qrow], want_row[qrow] = d2, trow
    offsets = (queries - np.asarray(origin, np.int64)) % 8
    fam = _finish(name, queries, searched, origin, offsets, want_d2, want_row, np.ones(len(q), np.int64))
    assert np.array_equal(fam.dims, dims), f"{name}: grid of {fam.dims} cells, planned {dims}"
    return fam


F_CASES = {
    "F_border": dict(dims=(5, 5, 5)),                                          # 8 corner, 12 edge and 6 face cells, 26 directions
    "F_1x1x1": dict(dims=(1, 1, 1), cells=[(0, 0, 0)]),
    "F_2x1x1": dict(dims=(2, 1, 1), cells=[(0, 0, 0), (1, 0, 0)]),             # one bitmap word, ncells % 32 != 0
    "F_5x3x3": dict(dims=(5, 3, 3), cells=[(x, y, z) for x in (0, 2, 4) for y in (0, 2) for z in (0, 2)]),   # 45 cells: two words
    "F_negative": dict(dims=(5, 5, 5), origin=(-37, -8, -1000)),
}

GENERATORS = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "Dself": family_d_self, "E": family_e,
              "E4": lambda: family_e("E4", 4)}
GENERATORS.update({k: (lambda k=k: family_f(k, **F_CASES[k])) for k in F_CASES})
NAMES = tuple(GENERATORS)
_CACHE = {}


def family(name):
    """The family of that name, generated once per process (its reference is computed on demand and kept with it)."""
    if name not in _CACHE:
        _CACHE[name] = GENERATORS[name]()
    return _CACHE[name]


def far_blob(fam, seed=701):
    """The `spread` trick of variant_rows.make_pair on a lattice family: an eighth of the probes, moved as they are 20000 voxels
    along x, give a bounding box the voxel bricks do not cover (more than 2048 cells on that axis).  Distances and winners stay: a
    probe moves with all of its points."""
    rng = np.random.default_rng(seed)
    nprobes = int(fam.qprobe.max()) + 1
    moved = np.zeros(nprobes, dtype=bool)
    moved[rng.permutation(nprobes)[: nprobes // 8]] = True
    shift = np.array([20000.0, 0.0, 0.0], np.float32)
    q = np.ascontiguousarray(fam.queries + moved[fam.qprobe][:, None] * shift)
    s = np.ascontiguousarray(fam.searched + moved[fam.sprobe][:, None] * shift)
    lo = np.minimum(q.min(axis=0), s.min(axis=0)).astype(np.int64)
    hi = np.maximum(q.max(axis=0), s.max(axis=0)).astype(np.int64)
    far = Family(fam.name + "_spread", q, s, lo, (hi - lo) // 8 + 1, None, fam.d2, fam.row, fam.nvox)
    # between the two clouds nothing changes: a probe's points stay within 18 voxels of its query and every other probe at least 30
    # away, moved or not (tests/test_vox_reference_host.py holds both directions to a fresh brute force); the self search does change
    far._ref.update({d: fam.reference(d) for d in (0, 1)})
    return far
