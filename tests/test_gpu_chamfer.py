"""Chamfer and truncated-distance rows on the GPU (include/pccm.h, pccm_reduce_map_total_many; CalculateOptions(chamfer=...,
truncate=...)): np.sum(f(column)) formed by the map mode of the general reduction kernel, no column stored.

Every comparison is ``==`` on float64 bits, against the NumPy restatement of tests/chamfer_reference.py applied to the oracle's
columns and to the GPU's own fetched columns."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
from click.testing import CliRunner

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair, DeviceColumn
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import write_point_cloud
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chamfer_reference as ref  # noqa: E402
import variant_rows as vr  # noqa: E402
from test_gpu_ties_mean import lattice_pair  # noqa: E402

D1, D2, PR = nat.METRIC_D1, nat.METRIC_D2, nat.METRIC_PROJ
CLAMP, ROOT_, BOTH = nat.MAP_CLAMP, nat.MAP_ROOT, nat.MAP_CLAMP | nat.MAP_ROOT


def same(x, y):
    return np.float64(x).tobytes() == np.float64(y).tobytes()


def report(pair, chamfer=True, taus=(), hausdorff=False, p2plane=False, color=None, frame=False, **kw):
    opts = CalculateOptions(color, hausdorff, p2plane, chamfer=chamfer, truncate=taus or None, **kw)
    with np.errstate(divide="ignore"):
        res = MetricCalculator(pair).calculate(transform_options(opts))
        return res.as_df() if frame else res.as_dict()


def oracle_columns(a, b):
    return orc.nn(a, b, method="kdtree")[1], orc.nn(b, a, method="kdtree")[1]


def oracle_d2_columns(a, b, na, nb, mode):
    out = []
    for it, se, nse in ((a, b, nb), (b, a, na)):
        proj = orc.point_to_plane(it, se, orc.nn(it, se, method="kdtree")[0], nse, normal_index=mode)
        out.append(proj * proj)
    return out


def gpu_columns(pair):
    return np.asarray(pair.get_left_neighbour_distances()), np.asarray(pair.get_right_neighbour_distances())


def gpu_d2_columns(pair):
    return [np.asarray(np.square(pair.point_to_plane_column(is_left))) for is_left in (True, False)]


def check_rows(res, left, right, chamfer, taus, left_d2=None, right_d2=None):
    """The new rows of a report -- the last ones, in the stated order -- against the restatement over the columns."""
    want = ref.rows(left, right, chamfer, taus, left_d2, right_d2)
    assert list(res)[-len(want):] == list(want)
    for key, value in want.items():
        assert same(res[key], value), (key, res[key], value)


def uniform(n, m, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3)).astype(np.float32), rng.random((m, 3)).astype(np.float32)


def thresholds_of(column):
    """0, below the column's minimum, at its median -- between the median element and the next larger one, so that the clamp bites
    on some rows and spares others whatever the rounding of sqrt and of tau * tau --, above its maximum."""
    col = np.sort(np.asarray(column, dtype=np.float64))
    n = len(col)
    lo = 0.5 * float(np.sqrt(col[0]))
    at = (n - 1) // 2
    above = col[col > col[at]]
    mid = float(np.sqrt(0.5 * (col[at] + above[0]))) if len(above) else float(np.sqrt(col[at]))
    return ref.thresholds((0.0, lo, mid, 2.0 * float(np.sqrt(col[-1])) + 1.0))


def check_thresholds(column, taus):
    v, n = np.asarray(column), len(column)
    assert taus[0] == 0.0 and len(taus) == (4 if v.min() > 0 else 3)           # (a column that holds 0.0 has nothing below its minimum)
    if v.min() > 0:
        assert np.count_nonzero(v > ref.cap(taus[1])) == n                     # below the minimum: every row is clipped
    if n >= 2 and v.min() < v.max():
        assert 0 < np.count_nonzero(v > ref.cap(taus[-2])) < n                 # at the median: some are, some are not
    assert np.count_nonzero(v > ref.cap(taus[-1])) == 0                        # above the maximum: none is


def check_identities(res, taus):
    top = taus[-1]
    for is_left in (True, False):
        assert same(res[(ref.TMSE, is_left, top)], res[("GeoMSE", is_left, False)])
        assert same(res[(ref.TMEAN, is_left, top)], res[(ref.MEAN, is_left, False)])
        assert same(res[(ref.TMSE, is_left, 0.0)], 0.0) and same(res[(ref.TMEAN, is_left, 0.0)], 0.0)


# ---- reports against the oracle's columns and the GPU's own fetched columns -----------------------------------------------------
@functools.lru_cache(maxsize=16)
def uniform_case(n, m):
    a, b = uniform(n, m, 7 * n + m)
    return a, b, oracle_columns(a, b)


@pytest.mark.parametrize("engine", ["grid", "brute"])
@pytest.mark.parametrize("n, m", [(1, 1), (2, 2), (127, 127), (129, 129), (4095, 4095), (4097, 4097), (8191, 8191), (8193, 8193),
                                  (20000, 20000), (100_003, 100_003), (300, 200), (5000, 4097)])
def test_uniform_pairs(n, m, engine):
    a, b, (left, right) = uniform_case(n, m)
    taus = thresholds_of(left)
    check_thresholds(left, taus)
    with CloudPair(PointCloud(a), PointCloud(b), extent=[1.0, 1.0, 1.0], nn_engine=engine) as pair:
        res = report(pair, True, taus)
        own = gpu_columns(pair)
    check_rows(res, left, right, True, taus)
    check_rows(res, own[0], own[1], True, taus)
    check_identities(res, taus)


# ---- every layout a search leaves its result in -----------------------------------------------------------------------------------
def layout_check(a, b, na=None, nb=None, extent=(1.0, 1.0, 1.0), path=False, **kw):
    mode = kw.get("normal_index", "row")
    left, right = oracle_columns(np.asarray(a), np.asarray(b))
    p2plane = na is not None
    d2 = oracle_d2_columns(np.asarray(a), np.asarray(b), na, nb, mode) if p2plane else (None, None)
    taus = thresholds_of(left)
    check_thresholds(left, taus)
    with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=list(extent), **kw) as pair:
        res = report(pair, True, taus, hausdorff=True, p2plane=p2plane)
        names = pair._engine.last_path(nat.PATH_REDUCE)
        own = gpu_columns(pair)
        own_d2 = gpu_d2_columns(pair) if p2plane else (None, None)
        counts = pair.tie_counts(True) if kw.get("ties") == "mean" else None
    check_rows(res, left, right, True, taus, *d2)
    check_rows(res, own[0], own[1], True, taus, *own_d2)
    check_identities(res, taus)
    if path:      # the mapped batches ran on the general kernel; the report's plain columns still went to their lean kernel
        assert "k_unit_jobs" in names and any(k.startswith("k_unit_lean<") for k in names), names
    return res, counts


@pytest.mark.parametrize("mode", ["row", "neighbour"])
def test_matched_records_with_deferred_projection(mode):
    n = 20000
    a, b = uniform(n, n, 5)
    res, _ = layout_check(a, b, vr._unit(n, 1), vr._unit(n, 2), normal_index=mode, path=True)
    assert res[(ref.MEAN, True, True)] > 0 and not same(res[(ref.MEAN, True, True)], res[(ref.MEAN, True, False)])


def test_fp64_clouds_in_32_byte_records():
    n = 20000
    rng = np.random.default_rng(17)
    a, b = rng.random((n, 3)), rng.random((n, 3))
    assert not np.array_equal(a, a.astype(np.float32).astype(np.float64))      # not fp32-exact: the searches keep fp64 records
    layout_check(a, b, vr._unit(n, 3, True), vr._unit(n, 4, True), path=True)


def test_ties_mean():
    n = 20000
    a, b = uniform(n, n, 23)
    _, counts = layout_check(a, b, vr._unit(n, 5), vr._unit(n, 6), ties="mean")
    assert counts.max() == 1       # tie-free data: the oracle's pick columns are the policy's own


def test_voxelised_integer_pair():
    n = 20000
    rng = np.random.default_rng(29)
    a = np.unique(rng.integers(0, 64, (n, 3)), axis=0).astype(np.float32)
    b = np.unique(rng.integers(0, 64, (n, 3)), axis=0).astype(np.float32)
    layout_check(a, b, extent=(64.0, 64.0, 64.0))


# ---- planted integer lattice ------------------------------------------------------------------------------------------------
def test_planted_lattice_under_both_tie_policies():
    a, b = lattice_pair()
    left, right = oracle_columns(np.asarray(a.points), np.asarray(b.points))
    assert set(np.unique(left)) >= {0.0, 1.0, 2.0} and np.all(left == np.round(left))      # exact small integers
    taus = (0.0, 1.0, 2.0)
    rows = {}
    for ties in ("pick", "mean"):
        with CloudPair(a, b, extent=[24.0, 24.0, 24.0], ties=ties) as pair:
            rows[ties] = report(pair, True, taus)
            own = gpu_columns(pair)
        check_rows(rows[ties], left, right, True, taus)
        check_rows(rows[ties], own[0], own[1], True, taus)
    want = ref.rows(left, right, True, taus)
    assert all(same(rows["pick"][k], rows["mean"][k]) for k in want)
    for ties in ("pick", "mean"):
        for is_left, v in ((True, left), (False, right)):
            n = len(v)         # min(v, 1) is 0 on the coincident points and 1 on every other: the sum counts the others, exactly
            assert rows[ties][(ref.TMSE, is_left, 1.0)] * n == n - np.count_nonzero(v == 0)
            assert same(rows[ties][(ref.TMSE, is_left, 1.0)], np.float64(n - np.count_nonzero(v == 0)) / n)
            assert same(rows[ties][(ref.TMEAN, is_left, 1.0)], rows[ties][(ref.TMSE, is_left, 1.0)])      # sqrt(0) = 0, sqrt(1) = 1


# ---- through the engine (ABI) -------------------------------------------------------------------------------------------------
def test_every_record_form_is_mapped_as_it_is_reduced():
    """Engine x matched rows kept x normals' precision x normal_index x projection fused: plain columns, 32-byte records and
    16-byte matched records with deferred projection.  Eight requests per call, two maps per column and job."""
    n, m = 20_011, 17_001
    a, b, _ = vr.make_pair(n, m, seed=0)
    nn = {0: orc.nn(a, b, method="kdtree"), 1: orc.nn(b, a, method="kdtree")}
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, a); eng.set_cloud(1, b)
        for f64 in (False, True):
            for mode in ("neighbour", "row"):
                la, lb = (n, m) if mode == "neighbour" else (max(n, m),) * 2
                na, nb = vr._unit(la, 7, f64), vr._unit(lb, 8, f64)
                eng.set_normals(0, na); eng.set_normals(1, nb)
                want = {}
                for d, (it, se, nse) in enumerate(((a, b, nb), (b, a, na))):
                    want[(d, D1)] = nn[d][1]
                    proj = orc.point_to_plane(it, se, nn[d][0], nse, normal_index=mode)
                    want[(d, D2)] = proj * proj
                req = []
                for (d, met), col in want.items():                   # the root, and the clamped root at the column's median
                    req += [(d, met, ROOT_, 0.0), (d, met, BOTH, float(np.median(col)))]
                more = [(0, D1, CLAMP, float(np.median(want[(0, D1)]))), (1, D2, CLAMP, np.inf), (1, D2, CLAMP, -1.0), (0, D2, BOTH, 0.0)]
                expect = [ref.totals(want[(d, met)], which, x) for d, met, which, x in req + more]
                for engine in ("grid", "brute"):
                    for want_idx in (True, False):
                        for turn, fuse in enumerate((mode, None)):
                            what = f"{engine} f64={f64} {mode} idx={want_idx} fuse={fuse}"
                            for d in (0, 1):
                                eng.nn_fuse(d, fuse)
                            eng.nn_want_idx(want_idx)
                            eng.drop_caches()
                            eng.nn_pair(engine)
                            if turn:                                 # behind reductions enqueued by the caller, or on its own
                                eng.reduce_prefetch_many([(0, D1), (0, D2), (1, D1), (1, D2)], mode)
                                eng.reduce_map_prefetch_many(req, mode)
                            got = eng.reduce_map_total_many(req, mode) + eng.reduce_map_total_many(more, mode)
                            assert "k_unit_jobs" in eng.last_path(nat.PATH_REDUCE), what
                            for g, w, r in zip(got, expect, req + more):
                                assert all(same(x, y) for x, y in zip(g, w)), (what, r, g, w)
                            plain = eng.reduce_total_many([(1, D2)], mode)[0]
                            assert all(same(x, y) for x, y in zip(got[len(req) + 1], plain)), what       # x = +inf: the plain total
    finally:
        eng.close()


def engine_pair(n=5000, m=4097, seed=61, normals=True):
    a, b = uniform(n, m, seed)
    eng = nat.Engine(0)
    eng.set_cloud(0, a); eng.set_cloud(1, b)
    if normals:
        eng.set_normals(0, vr._unit(n, 1)); eng.set_normals(1, vr._unit(m, 2))
    return eng, a, b


def test_identities_through_the_engine():
    eng, a, b = engine_pair()
    try:
        eng.nn_pair("grid")
        left, right = oracle_columns(a, b)
        plain = eng.reduce_total_many([(0, D1), (1, D1), (0, D2), (1, D2)], "neighbour")
        inf = eng.reduce_map_total_many([(0, D1, CLAMP, np.inf), (1, D1, CLAMP, np.inf), (0, D2, CLAMP, np.inf), (1, D2, CLAMP, np.inf)], "neighbour")
        for p, q in zip(plain, inf):                                     # x = +inf clamps nothing: the plain total's three doubles
            assert all(same(x, y) for x, y in zip(p, q)), (p, q)
        root = eng.reduce_map_total_many([(0, D1, ROOT_, 0.0), (1, D1, ROOT_, 5.0), (0, D2, ROOT_, 0.0), (1, D2, ROOT_, 0.0)], "neighbour")
        for p, q in zip(plain, root):                                    # sqrt is monotonic: min / max commute with it
            assert same(q[1], np.sqrt(p[1])) and same(q[2], np.sqrt(p[2]))
        assert all(same(x, y) for x, y in zip(root[0], ref.totals(left, ROOT_))) and all(same(x, y) for x, y in zip(root[1], ref.totals(right, ROOT_)))
        # cap <= 0 is allowed; the same request twice in a call is answered twice; eight maps of one column in one call
        xs = [float(v) for v in np.quantile(left, [0.1, 0.4, 0.7, 0.95])]
        req = [(0, D1, CLAMP, 0.0), (0, D1, CLAMP, -2.5), (0, D1, BOTH, 0.0), (0, D1, CLAMP, xs[0])] + [(0, D1, BOTH, x) for x in xs[:3]] \
            + [(0, D1, CLAMP, xs[0])]
        eng.reduce_map_prefetch_many(req)
        got = eng.reduce_map_total_many(req)
        for g, (_, _, which, x) in zip(got, req):
            assert all(same(p, q) for p, q in zip(g, ref.totals(left, which, x))), (which, x)
        assert got[0] == (0.0, 0.0, 0.0) and got[1] == (-2.5 * len(left), -2.5, -2.5)
    finally:
        eng.close()


def test_c_calls_and_their_error_codes():
    n, m = 5000, 4000
    a, b = uniform(n, m, 61)
    na, nb = vr._unit(n, 1), vr._unit(m, 2)
    lib = nat.load()
    eng = nat.Engine(0)

    def call(fn, reqs, modes=None, out=True):
        k = len(reqs)
        arr = ctypes.c_int * k
        args = [eng._ctx, k, arr(*[r[0] for r in reqs]), arr(*[r[1] for r in reqs]), arr(*(modes or [1] * k)), arr(*[r[2] for r in reqs]),
                (ctypes.c_double * k)(*[r[3] for r in reqs])]
        buf = (ctypes.c_double * max(3 * k, 1))()
        rc = fn(*args, buf) if out else fn(*args)
        return rc, [tuple(buf[3 * i:3 * i + 3]) for i in range(k)]
    both = ((lib.pccm_reduce_map_prefetch_many, False), (lib.pccm_reduce_map_total_many, True))
    try:
        eng.set_cloud(0, a); eng.set_cloud(1, b)
        for fn, out in both:
            assert call(fn, [(0, D1, ROOT_, 0.0)], out=out)[0] == nat.E_STATE              # no search result yet
        eng.nn_pair("grid")
        left, right = oracle_columns(a, b)
        for fn, out in both:
            assert call(fn, [(2, D1, ROOT_, 0.0)], out=out)[0] == nat.E_ARG                # PCCM_DIR_SELF
            assert call(fn, [(0, PR, ROOT_, 0.0)], out=out)[0] == nat.E_ARG                # other metrics
            assert call(fn, [(0, nat.METRIC_ANGULAR, CLAMP, 1.0)], out=out)[0] == nat.E_ARG
            assert call(fn, [(0, D1, 0, 1.0)], out=out)[0] == nat.E_ARG                    # map 0: the plain calls exist for that
            assert call(fn, [(0, D1, 4, 1.0)], out=out)[0] == nat.E_ARG
            assert call(fn, [(0, D1, -1, 1.0)], out=out)[0] == nat.E_ARG
            assert call(fn, [(0, D1, CLAMP, float("nan"))], out=out)[0] == nat.E_ARG       # NaN cap
            assert call(fn, [(0, D1, BOTH, float("nan"))], out=out)[0] == nat.E_ARG
            assert call(fn, [(0, D1, ROOT_, 0.0)] * 9, out=out)[0] == nat.E_ARG            # n <= 8
            assert call(fn, [], out=out)[0] == nat.OK
            # D2 without normals fails as the reduction does
            total = (ctypes.c_double * 3)()
            assert call(fn, [(0, D2, ROOT_, 0.0)], out=out)[0] == lib.pccm_reduce_total(eng._ctx, 0, D2, 1, total) == nat.E_STATE
        assert lib.pccm_reduce_map_total_many(eng._ctx, 1, None, None, None, None, None, None) == nat.E_ARG
        rc, got = call(lib.pccm_reduce_map_total_many, [(0, D1, ROOT_, float("nan"))])     # the cap is read with PCCM_MAP_CLAMP alone
        assert rc == nat.OK and all(same(x, y) for x, y in zip(got[0], ref.totals(left, ROOT_)))
        eng.set_normals(0, na); eng.set_normals(1, nb)
        assert call(lib.pccm_reduce_map_total_many, [(0, D2, ROOT_, 0.0)], modes=[0])[0] == nat.E_RANGE  # row-indexed normals out of range
        x = float(np.median(left))
        rc, got = call(lib.pccm_reduce_map_total_many, [(1, D2, CLAMP, np.inf), (0, D1, BOTH, x)], modes=[0, 0])
        plain = eng.reduce_total(1, D2, "row")
        assert rc == nat.OK and all(same(p, q) for p, q in zip(got[0], plain)) and all(same(p, q) for p, q in zip(got[1], ref.totals(left, BOTH, x)))
        # staleness: a mapped reduction enqueued on a search whose cloud was replaced is never consumed
        assert call(lib.pccm_reduce_map_prefetch_many, [(0, D1, BOTH, x)], out=False)[0] == nat.OK
        b2 = (b * np.float32(0.9)).astype(np.float32)
        eng.set_cloud(1, b2)
        assert call(lib.pccm_reduce_map_total_many, [(0, D1, BOTH, x)])[0] == nat.E_STATE
        eng.nn_pair("grid")
        rc, got = call(lib.pccm_reduce_map_total_many, [(0, D1, BOTH, x), (1, D1, BOTH, x)])
        left2, right2 = oracle_columns(a, b2)
        assert rc == nat.OK and all(same(p, q) for p, q in zip(got[0], ref.totals(left2, BOTH, x)))
        assert all(same(p, q) for p, q in zip(got[1], ref.totals(right2, BOTH, x))) and not same(got[0][0], ref.totals(left, BOTH, x)[0])
        eng.set_shard(0, 2)
        assert call(lib.pccm_reduce_map_total_many, [(0, D1, ROOT_, 0.0)])[0] == nat.E_STATE             # a sharded context
        assert call(lib.pccm_reduce_map_prefetch_many, [(0, D1, ROOT_, 0.0)], out=False)[0] == nat.E_STATE
    finally:
        eng.close()


# ---- reports: order, the other rows, reuse, graphs, the command line --------------------------------------------------------------
def test_rows_and_the_other_rows_with_every_option(monkeypatch):
    n = 8193
    a, b = uniform(n, n, 41)
    na, nb = vr._unit(n, 1), vr._unit(n, 2)
    taus = (0.0, 0.004, 0.01, 0.05)
    left, right = oracle_columns(a, b)
    d2 = oracle_d2_columns(a, b, na, nb, "row")
    for hausdorff, p2plane, fscore in ((False, False, None), (True, False, (0.01,)), (False, True, None), (True, True, (0.01, 0.02))):
        kw = dict(hausdorff=hausdorff, p2plane=p2plane, fscore=fscore)
        with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0]) as pair:
            plain = report(pair, False, (), **kw)
        with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0]) as pair:
            def never(self):
                raise AssertionError(f"{self!r} was copied to the host")
            monkeypatch.setattr(DeviceColumn, "_materialise", never)
            calls = []
            total_many = pair._engine.reduce_map_total_many
            monkeypatch.setattr(pair._engine, "reduce_map_total_many", lambda reqs, mode="row": calls.append(len(reqs)) or total_many(reqs, mode))
            full = report(pair, True, taus, **kw)
            monkeypatch.undo()
        mapped = (4 if p2plane else 2) + 4 * 4
        assert sum(calls) == mapped and len(calls) == -(-mapped // 8), calls       # fetched in ceil(count / 8) calls
        check_rows(full, left, right, True, taus, *(d2 if p2plane else (None, None)))
        added = (8 if p2plane else 5) + 6 * 4
        assert list(full)[:len(plain)] == list(plain) and len(full) == len(plain) + added
        for key, value in plain.items():           # exactly the same values under all other keys
            assert np.asarray(full[key], dtype=np.float64).tobytes() == np.asarray(value, dtype=np.float64).tobytes(), key
        with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0]) as pair:
            only = report(pair, False, taus[1:3], **kw)
        check_rows(only, left, right, False, taus[1:3])
        assert list(only)[:len(plain)] == list(plain) and len(only) == len(plain) + 6


def test_with_reconst():
    n = 30_000
    a, b0 = uniform(n, n, 21)
    origin = PointCloud(a)
    decoded = [PointCloud((b0 + np.float32(0.001 * k)).astype(np.float32)) for k in range(3)]
    taus = (0.0, 0.005, 0.01, 0.02)
    pair, got = CloudPair(origin, decoded[0], extent=[1.0, 1.0, 1.0]), []
    try:
        for k in range(3):
            if k:
                pair = pair.with_reconst(decoded[k])
            got.append(report(pair, True, taus, hausdorff=True))
    finally:
        pair.close()
    for k in range(3):
        check_rows(got[k], *oracle_columns(a, np.asarray(decoded[k].points)), True, taus)
    assert not same(got[0][(ref.L1,)], got[1][(ref.L1,)])


def test_graph_replays_with_new_decoded_points():
    n = 50_000
    a, b = uniform(n, n, 31)
    taus = (0.0, 0.004, 0.01, 0.05)
    with CloudPair(PointCloud(a), PointCloud(b), extent=[1.0, 1.0, 1.0], use_graph=True) as pair:
        for k in range(3):                         # three decoded clouds of one size under the same pair
            bk = (b * np.float32(1.0 - 0.01 * k)).astype(np.float32)
            if k:
                pair._engine.set_cloud(1, bk)
                pair.clouds = (pair.clouds[0], PointCloud(bk))
                pair.recompute()
            rows = []
            for _ in range(4):                     # eager, capture, two replays
                rows.append(report(pair, True, taus, hausdorff=True))
                pair.recompute()
            assert pair._graph_id is not None
            with CloudPair(PointCloud(a), PointCloud(bk), extent=[1.0, 1.0, 1.0]) as eager:
                want = report(eager, True, taus, hausdorff=True)
            for r in rows:
                assert list(r) == list(want) and all(same(r[key], want[key]) for key in want)
            check_rows(rows[-1], *oracle_columns(a, bk), True, taus)


def test_command_line(tmp_path):
    n = 5000
    a, b = uniform(n, n, 51)
    b = (a + np.float32(0.02) * (b - np.float32(0.5))).astype(np.float32)
    c = (a + np.float32(0.05) * (b - np.float32(0.5))).astype(np.float32)
    pa, pb, pc = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "c.ply")
    write_point_cloud(pa, PointCloud(a))
    write_point_cloud(pb, PointCloud(b))
    write_point_cloud(pc, PointCloud(c))
    args = ["--ocloud", pa, "--pcloud", pb, "--pcloud", pc, "--hausdorff"]
    taus = (0.01, 0.05)

    def expect(decoded):
        want = ref.rows(*oracle_columns(a, decoded), True, taus)
        out = []
        for k, v in want.items():
            sym = k[0] == "SymmetricMetric"
            inner = k[1:len(k) // 2 + 1] if sym else k
            label = inner[0] + (f"[{inner[-1]!r}]" if "Truncated" in inner[0] else "") + ("(symmetric)" if sym else "")
            fields = [] if sym or len(inner) == 1 else [str(inner[1])] + ([str(inner[2])] if inner[0] == ref.MEAN else [])
            out.append([label] + fields + [str(v)])
        return out
    base = CliRunner().invoke(cli, args)
    text = CliRunner().invoke(cli, args + ["--chamfer", "--truncate", "0.05", "--truncate", "0.01"])
    csv = CliRunner().invoke(cli, args + ["--chamfer", "--truncate", "0.05", "--truncate", "0.01", "--csv"])
    assert base.exit_code == 0 and text.exit_code == 0 and csv.exit_code == 0, (base.output, text.output, text.exception, csv.exception)
    base_lines, lines = base.output.rstrip("\n").split("\n"), text.output.rstrip("\n").split("\n")
    per, added = len(base_lines) // 2, 5 + 12
    assert len(base_lines) == 2 * per and len(lines) == 2 * (per + added)
    for k, decoded in enumerate((b, c)):           # one report per processed cloud: today's rows, then the new ones
        mine, theirs = lines[k * (per + added):(k + 1) * (per + added)], base_lines[k * per:(k + 1) * per]
        assert [ln.split() for ln in mine[1:per]] == [ln.split() for ln in theirs[1:]]
        assert [ln.split()[1:] for ln in mine[per:]] == expect(decoded)
    rows = [ln.split(",") for ln in csv.output.split("\n") if ln]      # (to_csv ends its text with a newline of its own)
    assert len(rows) == 2 * (per + added)
    assert [[r[1]] + [f for f in r[2:] if f] for r in rows[-added:]] == expect(c)
