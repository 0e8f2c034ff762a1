"""Cases for the filed tails (open_pcc_metric_amd/csrc/pccm_tail_wave.h; tests/test_gpu_tail_filed.py and its child process
tests/tail_filed_child.py run them): uniform fp32 clouds of 60 000 points -- 14 full blocks of 4096 rows and a partial one, about 1e-3
of the rows on the tail lists -- with rows planted on the geometry the library will choose (grid_planted.predict_geometry).

What is planted, all of it fp32-exact:
  tie   a query at a cell centre c on a 2^-9 lattice and two points of the other cloud at c -+ (2^-13, 0, 0): both at exactly 2^-26,
        in ring 1, so the brick kernel has no certificate and the query goes to the tail whatever else holds; rings 2-3 settle it on
        the smaller row (the tie rule);
  copy  a query that IS a point of the other cloud (d2 = 0), taken from the points whose x lies well inside their cell: ring 1
        settles it with a certificate (the second nearest point is not at 0) -- a row that is surely on no tail list.
A block of 4096 rows made of copies and ties alone holds exactly as many tail entries as it has ties.
"""
import functools
from types import SimpleNamespace

import numpy as np

import grid_planted as gp

N = 60_000
BLOCK = 4096
CAP = 32                                   # kTailBlockCap
DELTA = 2.0 ** -13
SPARE = 400                                # the last rows of a cloud are free to be overwritten with tie partners

CASES = {
    # name: (rows of cloud 1, normals dtype, plants)
    "plain": (N, np.float32, ()),
    "edges": (N, np.float64, ("first_last", "quiet_blocks")),
    "cap": (N, np.float32, ("cap",)),
    "cap_plus": (N, np.float32, ("cap_plus",)),
    "outlier": (N, np.float32, ("outlier",)),
    "unequal": (50_000, np.float32, ()),
}
FILED = {"plain": True, "edges": True, "cap": True, "cap_plus": False, "outlier": False, "unequal": False}


def _centres(g, count, rng, taken):
    """`count` cell centres on the 2^-9 lattice, in distinct cells three or more cells inside the grid and apart from one another."""
    out = []
    while len(out) < count:
        c = np.round(rng.uniform(0.1, 0.9, 3) * 512.0) / 512.0
        cell = tuple(gp.cells(g, c[None, :])[0])
        t = (c - g.org) * g.inv_h
        if np.any(np.abs(t - np.floor(t) - 0.5) > 0.3) or any(max(abs(a - b) for a, b in zip(cell, o)) < 3 for o in taken):
            continue
        taken.append(cell)
        out.append(c)
    return np.array(out)


def _tie(a, b, row, c, spare):
    """Row `row` of `a` becomes a tie query at c; two spare rows of `b` become its equidistant partners."""
    a[row] = c
    b[spare.pop()] = c - np.array([DELTA, 0.0, 0.0])
    b[spare.pop()] = c + np.array([DELTA, 0.0, 0.0])


def _copies(g, a, b, rows, rng):
    """Rows `rows` of `a` become copies of points of `b` (not its spare rows) whose x lies well inside their cell."""
    t = (b[: len(b) - SPARE, 0].astype(np.float64) - g.org[0]) * g.inv_h[0]
    good = np.flatnonzero(np.abs(t - np.floor(t) - 0.5) < 0.4)
    good = good[good > 0]                            # (row 0 may be a planted query)
    a[rows] = b[rng.choice(good, len(rows), replace=False)]


def _plant(name, g):
    """The case's clouds with its plants placed on geometry g (None: the geometry of the clouds before anything is planted)."""
    m, _, plants = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    a = rng.random((N, 3), dtype=np.float32)
    b = rng.random((m, 3), dtype=np.float32)
    if "outlier" in plants:
        a[7] = (1.25, 0.5, 0.5)                      # one isolated point: it stretches the box
    g = gp.predict_geometry(a, b) if g is None else g
    if "outlier" in plants:
        assert (1.25 - b[:, 0].max()) * g.inv_h[0] > gp.KMAX + 2     # nothing of the other cloud within three rings
    taken, spare_a, spare_b = [], list(range(N - SPARE, N - 1)), list(range(m - SPARE, m - 1))
    if "first_last" in plants:                       # a tail row in block 0 and in the partial last block, in both directions
        cs = _centres(g, 4, rng, taken)
        _tie(a, b, 0, cs[0], spare_b)
        _tie(a, b, N - 1, cs[1], spare_b)
        _tie(b, a, 0, cs[2], spare_a)
        _tie(b, a, m - 1, cs[3], spare_a)
    if "quiet_blocks" in plants:                     # blocks without any entry
        _copies(g, a, b, np.concatenate([np.arange(blk * BLOCK, (blk + 1) * BLOCK) for blk in (5, 9)]), rng)
    for plant, ties in (("cap", CAP), ("cap_plus", CAP + 1)):
        if plant in plants:                          # block 3 of cloud 0: `ties` entries exactly
            rows = np.arange(3 * BLOCK, 4 * BLOCK)
            _copies(g, a, b, rows, rng)
            cs = _centres(g, ties, rng, taken)
            for k in range(ties):
                _tie(a, b, int(rows[17 + 113 * k]), cs[k], spare_b)
    return a, b, g


@functools.lru_cache(maxsize=None)
def build(name):
    m, ndt, plants = CASES[name]
    g = None
    for _ in range(4):                               # (a plant may overwrite a point that held the bounding box: place again)
        a, b, g = _plant(name, g)
        found = gp.predict_geometry(a, b)
        if gp.same_geom(found, g):
            break
        g = found
    assert gp.same_geom(gp.predict_geometry(a, b), g), "the plants keep moving the bounding box"
    na = np.random.default_rng(1).standard_normal((N, 3)).astype(ndt)
    nb = np.random.default_rng(2).standard_normal((m, 3)).astype(ndt)
    if ndt is np.float64:                            # not fp32-exact: the reductions read fp64 normals
        assert not np.array_equal(nb.astype(np.float32).astype(np.float64), nb)
    for v in (a, b, na, nb):
        v.setflags(write=False)
    return SimpleNamespace(name=name, a=a, b=b, na=na, nb=nb, geom=g, truth={}, two={}, sites=[])


def requests(case, nat):
    """D1 + D2 of both directions; a direction whose iterating cloud is the longer one has no row-indexed D2 (the reference's
    normals[row] would run out of range), so its D1 travels alone."""
    req = []
    for d, it, se in ((nat.DIR_LEFT, case.a, case.b), (nat.DIR_RIGHT, case.b, case.a)):
        req.append((d, nat.METRIC_D1))
        if len(it) <= len(se):
            req.append((d, nat.METRIC_D2))
    return req


def run(case, nat):
    """Eager step, capture, two replays on a fresh context -> per step the totals' bytes, both directions' rows and distances and
    nn_stats; whether the captured graph left the tail launch out; the geometry of the last search."""
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, case.a)
        eng.set_cloud(1, case.b)
        eng.set_normals(0, case.na)
        eng.set_normals(1, case.nb)
        req = requests(case, nat)
        steps = []

        def read():
            totals = np.asarray(eng.reduce_total_many(req), dtype=np.float64)
            cols = [eng.fetch_nn(d) for d in (0, 1)]
            steps.append(SimpleNamespace(totals=totals, idx=[c[0] for c in cols], d2=[c[1] for c in cols], stats=[eng.nn_stats(d) for d in (0, 1)]))

        def sweep():
            eng.drop_caches()
            eng.nn_pair("grid")
            eng.reduce_prefetch_many(req)

        sweep()
        read()
        eng.graph_begin()
        sweep()
        gid = eng.graph_end()
        filed = eng.graph_tail_filed(gid)
        read()
        for _ in range(2):
            eng.graph_launch(gid)
            read()
        return SimpleNamespace(steps=steps, filed=filed, geom=gp.make_geom(*eng.grid_geometry()))
    finally:
        eng.close()
