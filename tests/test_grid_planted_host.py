"""Host proofs for tests/grid_planted.py: the shortcut model (the stop rule as a function of the nearest distance alone) equals a
literal ring-by-ring port of thread_search; every planted case is what its family claims, has no undecided query and keeps
band <= lo / 20; the long-tail construction sends more than 2^18 queries per direction past ring 1; and the count and row
assertions of tests/test_gpu_grid_planted.py would notice a lazy or an unsound stop rule.  No GPU, no library."""
import functools

import numpy as np
import pytest

import brute_planted as bp
import grid_planted as gp

FRAME_CASES = [("flat", (True, True)), ("flat", (False, False)), ("flat", (True, False)), ("flat", (False, True)),
               ("long", (False, False)), ("long", (True, True))]
PATH = {("long", (False, False)): "coop", ("long", (True, True)): "brick"}
IDS = [f"{n}-{int(f[0])}{int(f[1])}" for n, f in FRAME_CASES]


# ---- the model against the literal port ---------------------------------------------------------------------------------------------
SYNTHETIC = {                                  # name -> (org, h, dim, points per cloud)
    "cube_12": ((-3.0, 2.0, 100.0), (0.5, 0.6, 0.55), (12, 12, 12), 500),
    "dim1_z": ((0.0, 0.0, 5.0), (1.0, 1.0, 1.0), (14, 9, 1), 150),
    "dim1_yz": ((1.0e3, 0.0, 0.0), (0.25, 1.0, 1.0), (40, 1, 1), 30),
    "dim2_x": ((0.0, -8.0, 0.0), (1.0, 0.7, 1.3), (2, 10, 11), 200),
    "dim_3_4_6": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (3, 4, 6), 30),           # dim < 2 r + 1 on every axis from ring 1, 2, 3 on
    "dim_5_7_20": ((-1.0e6, 1.0e6, 0.0), (2.0, 2.0, 2.0), (5, 7, 20), 120),
    "sparse_20": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (20, 20, 20), 90),         # most queries open after three rings
}


@pytest.mark.parametrize("name", sorted(SYNTHETIC))
@pytest.mark.parametrize("self_search", [False, True], ids=["pair", "self"])
def test_model_equals_the_ring_by_ring_port(name, self_search):
    org, h, dim, n = SYNTHETIC[name]
    g = gp.make_geom(org, h, dim)
    rng = np.random.default_rng([3, sorted(SYNTHETIC).index(name)])
    ext = g.h * g.dim
    # a tenth of the points outside the grid: they clamp into boundary cells, as trimmed outliers do
    q = g.org + rng.uniform(-0.1, 1.1, (300, 3)) * ext
    s = q if self_search else g.org + rng.uniform(-0.1, 1.1, (n, 3)) * ext
    rows, d = gp.brute64(q, s, self_search)
    ring, und = gp.classify(g, q, d)
    pring, prow, pd = gp.thread_search_port(g, q, s, self_search)
    ok = ~und
    assert ok.sum() >= 290
    assert np.array_equal(ring[ok], pring[ok]), np.flatnonzero(ok & (ring != pring))[:8]
    done = ok & (pring != gp.FLAGGED)
    assert np.array_equal(prow[done], rows[done]) and np.array_equal(pd[done], d[done])
    assert np.all(pd[~done] >= d[~done])
    assert len(set(ring[ok].tolist())) >= (1 if name in ("dim_3_4_6", "dim1_yz") else 2), "the geometry exercises one outcome only"


def test_model_has_every_outcome_on_the_synthetic_geometries():
    seen = set()
    for name in SYNTHETIC:
        org, h, dim, n = SYNTHETIC[name]
        g = gp.make_geom(org, h, dim)
        rng = np.random.default_rng([3, sorted(SYNTHETIC).index(name)])
        q = g.org + rng.uniform(-0.1, 1.1, (300, 3)) * g.h * g.dim
        s = g.org + rng.uniform(-0.1, 1.1, (n, 3)) * g.h * g.dim
        seen |= set(gp.classify(g, q, gp.brute64(q, s)[1])[0].tolist())
    assert seen == {1, 2, 3, gp.FLAGGED}


# ---- the frames ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name, fmt):
    return gp.cached("frame", name, fmt)


@pytest.mark.parametrize("name,fmt", FRAME_CASES, ids=IDS)
def test_frame_case_has_no_undecided_query_and_a_narrow_band(name, fmt):
    c = _case(name, fmt)
    f = gp.FRAMES[name]
    ratio = len(c.a) / float(c.geom.dim[1] * c.geom.dim[2])
    assert (ratio >= gp.COOP_MIN) == (name == "long") and abs(ratio - gp.COOP_MIN) > 4.0, ratio
    assert bp.is_exact32(c.a) == fmt[0] and bp.is_exact32(c.b) == fmt[1]
    assert len(c.a) == len(c.b) and np.all(c.a >= 0.0) and np.all(c.a <= c.layout.D) and np.all(c.b >= 0.0) and np.all(c.b <= c.layout.D)
    # the reserved region is empty of background in both clouds, 5 cells around every interior site's cell
    zmin = min(s.cell[2] for s in c.sites) - 5
    for cloud, nbg in zip((c.a, c.b), c.n_background):
        bg = cloud[8:nbg]
        assert gp.cells(c.geom, bg)[:, 2].max() < zmin
    for d in (0, 1, 2):
        p = gp.predict(c, d, PATH.get((name, fmt)))
        assert len(p.undecided) == 0, f"direction {d}: queries {p.undecided[:8].tolist()} are undecided"
        if (name, fmt) in PATH:
            assert p.lo >= 1000 and p.band <= p.lo / 20, (d, p.lo, p.band)
    assert f["sparse"] == 0 or gp.predict(c, 2).lo > 5000


@pytest.mark.parametrize("name,fmt", FRAME_CASES, ids=IDS)
def test_every_scenario_is_what_it_claims(name, fmt):
    c = _case(name, fmt)
    g = c.geom
    cell_of = {s.name: s.cell for s in c.sites}
    for s in c.sites:                              # 9 cells apart, one query each
        for t in c.sites:
            assert s is t or np.abs(cell_of[s.name] - cell_of[t.name]).max() >= 9, (s.name, t.name)
    qrows = np.array([s.qrow for s in c.sites])
    rows, d = gp.brute64(c.a[qrows], c.b)
    orows, od = gp.truth(c, 0)
    assert np.array_equal(rows, orows[qrows]) and np.array_equal(d, od[qrows])
    ring = gp.predict(c, 0).ring[qrows]
    pring, prow, pd = gp.thread_search_port(g, c.a[qrows], c.b)
    assert np.array_equal(pring, ring)
    kinds = set()
    for k, s in enumerate(c.sites):
        q = c.a[s.qrow]
        cq = gp.cells(g, q)
        assert np.array_equal(cq, s.cell), s.name
        assert rows[k] == s.brows[s.want], f"{s.name}: the neighbour is row {rows[k]}, planted {s.brows[s.want]}"
        assert ring[k] == s.ring, f"{s.name}: the model settles it at {ring[k]}, planted for {s.ring}"
        kind = s.spec[0]
        kinds.add(kind)
        L = gp.face_bounds(g, q)[0]
        if kind in ("F", "R"):
            a, side, r = s.axis, s.side, s.r
            only = gp.face_bounds(g, q, skip=(a, side))[0]
            assert only[r - 1] > L[r - 1], f"{s.name}: face ({a}, {side}) is not the one that binds at ring {r}"
            assert L[r - 1] < (r + 0.2501) * g.h[a]
        if kind == "R" or (kind == "F" and s.spec[4]):
            true, decoy = c.b[s.brows[s.want]], c.b[s.brows[s.decoy]]
            ct, cd = gp.cells(g, true), gp.cells(g, decoy)
            assert (ct[a] - cq[a]) == (r + 1) * (1 if side else -1), f"{s.name}: the true neighbour is not behind the face"
            assert np.abs(cd - cq).max() <= r, f"{s.name}: the decoy is outside the ring-{r} cube"
            assert gp.dist64(q, decoy) > gp.dist64(q, true) > L[r - 1] ** 2
            beyond = abs(true[a] - (g.org[a] + (cq[a] + (r + 1 if side else -r)) * g.h[a]))
            assert beyond < 2.1 * gp.OFF * g.h[a]
            assert prow[k] == (s.brows[s.want] if ring[k] != gp.FLAGGED else s.brows[s.decoy])     # flagged: the decoy is what three rings found
        if kind == "R":
            d32 = bp.dist32(q.astype(np.float32), np.stack([true, decoy]).astype(np.float32))
            assert d32[1] <= d32[0] and ring[k] == gp.FLAGGED, f"{s.name}: no fp32 reversal"
        if kind == "F" and not s.spec[4]:
            assert L[r - 1] ** 2 * (1 - 3 * gp.OFF) < d[k] < L[r - 1] ** 2 * (1 - gp.OFF)
            assert np.abs(gp.cells(g, c.b[rows[k]]) - cq).max() <= r
        if kind == "B":
            at_edge = (cq == 0) | (cq == g.dim - 1)
            assert at_edge.sum() == {"corner": 3, "edge": 2, "face": 1}[s.where]
            assert np.isfinite(L[0]) and abs(d[k] / L[0] ** 2 - 1.0) < 3 * gp.OFF
        if kind.startswith("T"):
            tied = [c.b[r_] for r_ in s.brows[:len(s.tie)]] if hasattr(s, "tie") else []
            assert all(gp.dist64(q, p) == d[k] for p in tied), f"{s.name}: the tie is not exact"
        if kind == "T_ring":
            assert [int(np.abs(gp.cells(g, p) - cq).max()) for p in tied] == s.rings_of and s.brows[0] < s.brows[1]
        if kind == "T_lanes":
            r = s.spec[1]
            lanes = [int((gp.cells(g, p)[2] - cq[2] + r) * (2 * r + 1) + gp.cells(g, p)[1] - cq[1] + r) for p in tied]
            assert lanes[0] > lanes[1] > lanes[2] and len(set(lanes)) == 3 and max(lanes) < (2 * r + 1) ** 2
            assert d[k] >= L[r - 2] ** 2
        if kind == "T_lanes":                  # the same tie inside the first cloud: the self search of the query
            r = s.spec[1]
            srows, sd = gp.truth(c, 2)
            mine = [c.a[x] for x in s.arows[1:]]
            assert all(np.array_equal(m_, t_) for m_, t_ in zip(mine, tied))           # dyadic: fp32-exact, the same in both clouds
            assert all(gp.dist64(q, m_) == sd[s.qrow] for m_ in mine) and srows[s.qrow] == s.arows[1] == min(s.arows[1:])
            slanes = [int((gp.cells(g, m_)[2] - cq[2] + r) * (2 * r + 1) + gp.cells(g, m_)[1] - cq[1] + r) for m_ in mine]
            own = r * (2 * r + 1) + r
            assert slanes[0] > slanes[1] > slanes[2] and own not in slanes and slanes[0] > own > slanes[2]
            sring = gp.predict(c, 2).ring
            assert sring[s.qrow] == s.self_ring == r
            pr2, prow2, _ = gp.thread_search_port(g, c.a[[s.qrow]], c.a, self_search=True, qrows=[s.qrow])
            assert pr2[0] == r and prow2[0] == s.arows[1]
            # the copies answer their twins at distance 0 in direction 0, and the query (the nearest of their own cloud) in the self search
            assert np.all(od[s.arows[1:]] == 0.0) and [int(x) for x in orows[s.arows[1:]]] == s.brows
            assert [int(x) for x in srows[s.arows[1:]]] == [s.qrow] * 3 and np.all(sring[s.arows[1:]] == r)
        if kind == "T_self":
            assert len(s.arows) == 3 and np.all(c.a[s.arows] == q)
            srows, sd = gp.truth(c, 2)
            assert [int(srows[x]) for x in s.arows] == [s.arows[1], s.arows[0], s.arows[0]] and np.all(sd[s.arows] == 0.0)
    assert kinds == {"F", "B", "T_ring", "T_lanes", "T_self", "R"}
    assert sum(1 for s in c.sites if s.spec[0] == "F") == 36
    # the self search: every scenario query but the duplicates (and the boundary sites, which see a pin) is alone within three rings:
    # flagged with nothing found
    alone = [s.qrow for s in c.sites if s.spec[0] not in ("T_self", "T_lanes", "B")]
    assert len(alone) >= 41
    assert np.all(gp.predict(c, 2).ring[alone] == gp.FLAGGED)


@pytest.mark.parametrize("fmt", [(True, True), (False, False)], ids=["11", "00"])
def test_trimmed_box_case_is_what_it_claims(fmt):
    c = gp.cached("trim", fmt)
    g = c.geom
    lo, hi, boxed = gp.trim_box(c.a, c.b)
    assert boxed and gp.same_geom(g, gp.predict_geometry(c.a, c.b, box=(lo, hi))), "the probes' final positions change the box"
    both = np.vstack([c.a, c.b])
    ext = both.max(axis=0) - both.min(axis=0)
    assert np.all(g.dim * g.h < 0.1 * ext), "the grid is not smaller than the bounding box: the case tests nothing"
    top = g.org + g.dim * g.h
    for ax in range(3):                      # at most 0.1 % of the points outside, per side
        assert 30 <= np.sum(both[:, ax] < g.org[ax] - 1.0) <= 1.0e-3 * len(both) and 30 <= np.sum(both[:, ax] > top[ax] + 1.0) <= 1.0e-3 * len(both)
    assert len(c.a) / float(g.dim[1] * g.dim[2]) < gp.COOP_MIN - 4 and bp.is_exact32(c.a) == fmt[0] and bp.is_exact32(c.b) == fmt[1]
    for d in (0, 1, 2):
        p = gp.predict(c, d)
        assert len(p.undecided) == 0 and p.flagged <= 400, (d, p.undecided[:8], p.flagged)
    qrows = np.array([s.qrow for s in c.sites])
    rows, d2 = gp.brute64(c.a[qrows], c.b)
    orows, od = gp.truth(c, 0)
    assert np.array_equal(rows, orows[qrows]) and np.array_equal(d2, od[qrows])
    ring = gp.predict(c, 0).ring[qrows]
    pring, prow, pd = gp.thread_search_port(g, c.a[qrows], c.b)
    assert np.array_equal(pring, ring)
    outside = lambda p, ax: bool(p[ax] < g.org[ax] or p[ax] > top[ax])                        # noqa: E731
    for k, s in enumerate(c.sites):
        kind, axis, side = s.spec
        q, nb = c.a[s.qrow], c.b[s.brows[0]]
        cq, cn = gp.cells(g, q), gp.cells(g, nb)
        assert rows[k] == s.brows[0] and ring[k] == s.ring == gp.X_RING[kind], s.name
        L = gp.face_bounds(g, q)[0]
        if kind in ("X1", "X4"):
            for ax in ((axis,) if kind == "X1" else axis):
                assert outside(q, ax) and outside(nb, ax) and cq[ax] == (0 if side == 0 else g.dim[ax] - 1), s.name
            assert np.array_equal(cq, cn) and d2[k] < 0.2 * g.h.max() ** 2
        if kind == "X2":
            assert outside(q, axis) and not outside(nb, axis) and np.array_equal(cq, cn) and cq[axis] == (0 if side == 0 else g.dim[axis] - 1)
            assert d2[k] > L[1] ** 2 and pring[k] == 3
        if kind in ("X3", "X3far"):
            assert not outside(q, axis) and outside(nb, axis) and cn[axis] == (0 if side == 0 else g.dim[axis] - 1) and abs(cq[axis] - cn[axis]) == 2
            assert np.isinf(gp.face_bounds(g, q, skip=(axis, 1 - side))[0][1]) or L[1] == gp.face_bounds(g, q, skip=(axis, side))[0][1], "ring 2 has a face on the trimmed side"
        if kind == "X3far":
            assert pring[k] == gp.FLAGGED and prow[k] == s.brows[0] and d2[k] > L[2] ** 2
    assert {s.spec[0] for s in c.sites} == set(gp.X_RING)
    for s in c.sites:
        for t in c.sites:
            assert s is t or np.abs(s.cell - t.cell).max() >= 9, (s.name, t.name)


def test_small_cases_cover_flat_grids_and_cubes_that_cover_the_grid():
    dims = {}
    for name in gp.SMALL:
        c = gp.cached("small", name)
        dims[name] = tuple(int(v) for v in c.geom.dim)
        for d in (0, 1, 2):
            q, s, self_ = gp.pair_of(c, d)
            coop = gp.SMALL[name][3] == "coop"
            p = gp.predict(c, d, "coop" if coop else None)
            assert len(p.undecided) == 0
            ratio = len(c.a) / float(c.geom.dim[1] * c.geom.dim[2])
            assert (ratio >= gp.COOP_MIN + 4) if coop else (ratio <= gp.COOP_MIN - 4), (name, ratio)
            if coop:
                assert p.lo >= 60 and p.band <= p.lo / 20, (name, d, p.lo, p.band)
            sub = np.arange(0, len(q), max(1, len(q) // 150))
            pring, prow, pd = gp.thread_search_port(c.geom, q[sub], s, self_, qrows=sub)
            assert np.array_equal(pring, p.ring[sub])
            rows, dd = gp.truth(c, d)
            done = pring != gp.FLAGGED
            assert np.array_equal(prow[done], rows[sub][done]) and np.array_equal(pd[done], dd[sub][done])
            brows, bd = gp.brute64(q, s, self_)
            assert np.array_equal(brows, rows) and np.array_equal(bd, dd)
        inf3 = np.isinf(gp.face_bounds(c.geom, c.a)[:, 2])
        if name in ("tiny_3", "tiny_40"):
            assert max(dims[name]) <= 4 and np.all(inf3) and gp.predict(c, 0).flagged == 0
        if name == "tiny_300":
            assert np.any(inf3) and not np.all(inf3)
    assert dims["planar_1000"][2] == 1 and min(dims["planar_1000"][:2]) > 7
    assert dims["collinear_x_500"][1:] == (1, 1) and dims["collinear_x_500"][0] > 64
    assert dims["collinear_y_400"][0] == dims["collinear_y_400"][2] == 1 and dims["collinear_y_400"][1] > 64
    assert dims["slab_3000"][2] == 2 and min(dims["slab_3000"][:2]) > 7


def test_brick_budget_port_sees_the_frames_dense_zone_overflow_in_shards_only():
    """The whole fp32-exact frame fits the brick kernel's LDS budget everywhere (4 x 2 bricks); a third of its rows takes 4 x 4
    bricks, which the dense zone (1.8 times the mean density) overflows: the port of the budget must say so, or the tail bounds of
    the sharded GPU case mean nothing."""
    c = _case("long", (True, True))
    assert not np.any(gp.brick_overflow(c.geom, c.a, c.b, len(c.a)))
    b, e = bp.shard_of(len(c.a), 1, 3)
    over = gp.brick_overflow(c.geom, c.a[b:e], c.b, len(c.a))
    assert 0.9 * (e - b) < over.sum() < e - b
    sparse = gp.cells(c.geom, c.a[b:e])[:, 2] > gp.FRAMES["long"]["dense"] + 8
    assert not np.any(over & sparse)


def test_long_tail_sends_more_than_2_18_queries_per_direction_past_ring_1():
    c = gp.cached("long_tail")
    assert bp.is_exact32(c.a) and bp.is_exact32(c.b)
    assert len(c.a) / float(c.geom.dim[1] * c.geom.dim[2]) >= gp.COOP_MIN + 4           # the brick kernel, then k_grid_tail
    for d in (0, 1):
        p = gp.predict(c, d)
        assert len(p.undecided) == 0, p.undecided[:8]
        assert p.lo > gp.TAIL_WAVE_MAX + 20_000, p.lo
        assert gp.LONG_TAIL_ISOLATED <= p.flagged <= 4 * gp.LONG_TAIL_ISOLATED, p.flagged


# ---- the assertions bite -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fmt", [FRAME_CASES[0], FRAME_CASES[4]], ids=[IDS[0], IDS[4]])
def test_a_lazy_rule_changes_the_counts(name, fmt):
    """L_r replaced by r h: the not-lazy sites (and the boundary sites planted just under L_1) settle later -- ring 1 -> tail,
    ring 3 -> rescan -- so both asserted counts move by at least the number of such sites."""
    c = _case(name, fmt)
    true, lazy = gp.predict(c, 0), gp.predict(c, 0, bounds=gp.lazy_bounds)
    n1 = sum(1 for s in c.sites if s.ring == 1 and s.spec[0] in ("F", "B"))
    n3 = sum(1 for s in c.sites if s.ring == 3 and s.spec[0] == "F" and not s.spec[4])
    assert n1 == 6 + 3 and n3 == 6
    assert lazy.flagged >= true.flagged + n3
    assert lazy.lo >= true.lo + n1
    if (name, fmt) in PATH:
        band = gp.predict(c, 0, PATH[(name, fmt)]).band
        assert lazy.lo > true.lo + band, "the tail count's band would hide the lazy rule"
    for s in c.sites:
        if s.spec[0] == "F" and not s.spec[4] and s.r in (1, 3):
            assert lazy.by_site[s.name] > true.by_site[s.name], s.name


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("side", [0, 1])
def test_a_rule_that_ignores_one_face_returns_a_wrong_row(axis, side):
    """The search with face (axis, side) left out of face_bound settles the sound sites of that face on their decoys, at every
    ring; every other scenario is unaffected."""
    c = _case(*FRAME_CASES[0])
    qrows = np.array([s.qrow for s in c.sites])
    rows, _ = gp.truth(c, 0)
    bad = functools.partial(gp.face_bounds, skip=(axis, side))
    pring, prow, _ = gp.thread_search_port(c.geom, c.a[qrows], c.b, bounds=bad)
    hit = 0
    for k, s in enumerate(c.sites):
        mine = (s.spec[0] == "R" or (s.spec[0] == "F" and s.spec[4])) and (s.axis, s.side) == (axis, side)
        if mine:
            assert pring[k] == s.r and prow[k] == s.brows[s.decoy] != rows[s.qrow], s.name
            hit += 1
        elif pring[k] != gp.FLAGGED:
            assert prow[k] == rows[s.qrow], s.name
    assert hit == 3 + sum(1 for s in c.sites if s.spec[0] == "R" and (s.axis, s.side) == (axis, side))
