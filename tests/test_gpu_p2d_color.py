"""Colour and joint point-to-distribution rows on the GPU ("Point-to-distribution: colour and joint";
include/pccm.h, pccm_p2d_build_attrs / PCCM_METRIC_P2D_COLOR / PCCM_METRIC_P2D_JOINT; CalculateOptions(p2d_color=True)).

The yardstick is the NumPy restatement of tests/p2d_color_reference.py over the neighbour rows and the geometry value of
tests/p2d_reference.py.  Per-point columns and pooled rows must equal it bit for bit: every step is separately rounded, so a
neighbour out of (d2, row) order, a luma formed another way, an FMA or a reordered sum changes them.  No tolerance anywhere in
this file."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
from click.testing import CliRunner

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import read_point_cloud, write_point_cloud
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud
from open_pcc_metric_amd.sequence import evaluate_pairs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import p2d_color_reference as cref  # noqa: E402
import p2d_reference as ref  # noqa: E402

GEO, COLOR, JOINT = "MahalanobisDistance", "ColorMahalanobisDistance", "JointMahalanobisDistance"
EXTENT = [1.0, 1.0, 1.0]
BOTH = nat.P2D_GEOMETRY | nat.P2D_COLOR


def pair_of(a, b, ca, cb, **kw):
    return CloudPair(PointCloud(a, colors=ca), PointCloud(b, colors=cb), extent=EXTENT, **kw)


def report(pair, k=30, p2d_color=True, **kw):
    opts = CalculateOptions(point_to_distribution=True, p2d_neighbours=k, p2d_color=p2d_color, **kw)
    with np.errstate(divide="ignore", invalid="ignore"):
        return MetricCalculator(pair).calculate(transform_options(opts)).as_dict()


def bits(res):
    return {key: np.asarray(v, dtype=np.float64).tobytes() for key, v in res.items()}


def assert_same(got, want):
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"


def same_bits(value, want):
    return np.float64(value).tobytes() == np.float64(want).tobytes()


def getters(pair, is_left):
    side = "left" if is_left else "right"
    return {cls: getattr(pair, f"get_{side}_{name}") for cls, name in
            ((GEO, "mahalanobis_distances"), (COLOR, "color_mahalanobis_distances"), (JOINT, "joint_mahalanobis_distances"))}


def check_pair(pair, a, b, ca, cb, k, nbr=None):
    """The geometry, colour and joint columns and the pooled rows of both directions of `pair` against the restatement."""
    res = report(pair, k, hausdorff=True)
    assert len([key for key in res if "ColorMahalanobis" in str(key) or "JointMahalanobis" in str(key)]) == 12
    cols = {}
    for is_left, p, q, cp, cq in ((True, a, b, ca, cb), (False, b, a, cb, ca)):
        want_nbr = ref.knn_rows(p, q, k) if nbr is None else nbr[is_left]
        want = dict(zip((GEO, COLOR, JOINT), cref.columns(p, q, cp, cq, k, nbr=want_nbr)))
        for cls, getter in getters(pair, is_left).items():
            column = getter(k)
            assert_same(np.asarray(column), want[cls])
            with np.errstate(invalid="ignore"):
                assert same_bits(np.sum(column), np.sum(want[cls])) and same_bits(np.max(column), np.max(want[cls]))
                assert same_bits(res[(cls, is_left, k)], np.mean(want[cls]))
            assert same_bits(res[("Max" + cls, is_left, k)], np.max(want[cls]))
        assert np.all(np.isfinite(want[COLOR]))
        cols[is_left] = want
    for cls in (GEO, COLOR, JOINT):
        for name, pool in ((cls, np.mean), ("Max" + cls, np.max)):
            left, right = pool(cols[True][cls]), pool(cols[False][cls])
            assert same_bits(res[("SymmetricMetric", name, True, k, name, False, k)], right if right > left else left)
    return cols


@functools.lru_cache(maxsize=None)
def family(name):
    """(a, b, ca, cb, brute-force neighbour rows of both directions at k = 64): the first k columns are the rows at any smaller k."""
    a, b, ca, cb = cref.FAMILIES[name]()
    return a, b, ca, cb, {True: ref.knn_rows(a, b, 64), False: ref.knn_rows(b, a, 64)}


# ---- every family -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 30, 64])
@pytest.mark.parametrize("name", sorted(cref.FAMILIES))
def test_columns_and_rows_are_bit_exact(name, k):
    a, b, ca, cb, rows = family(name)
    with pair_of(a, b, ca, cb) as pair:
        cols = check_pair(pair, a, b, ca, cb, k, nbr={side: r[:, :k] for side, r in rows.items()})
    if name == "lattice":                                        # the data has what it is here for: ties at the k-th distance
        d2 = np.sort(ref.sq_dist(a[:50, None, :], b[None, :, :]), axis=1)
        assert np.any(d2[:, k - 1] == d2[:, k])
    if name == "b_smaller_than_k":
        assert len(b) < k
    if name == "inf_geometry":                                   # ... +inf geometry values, which the joint column propagates
        mg, mj = cols[True][GEO], cols[True][JOINT]
        assert np.sum(np.isinf(mg)) >= 30 and np.array_equal(np.isinf(mj), np.isinf(mg))
    if name in ("surface_bytes", "constant_offset"):             # ... flat neighbourhoods: variances that round to 0 or below
        _, _, raw = cref.color_mahalanobis(ca, cb, rows[True][:, :k], return_parts=True)
        assert np.sum(raw <= 0) > 100


@pytest.mark.parametrize("name", ["surface_bytes", "duplicates"])
def test_float64_float32_and_byte_uploads_give_the_same_bits(name):
    """The families whose colours are bytes / 255: uploaded as float64 rows and as bytes (the device then gathers the packed
    bytes and divides again) the columns are the same bits.  As float32 rows the VALUES differ (k / 255 rounded to fp32), so the
    yardstick is the restatement on those values -- which are no byte quotients, so the device reads the fp64 rows."""
    a, b, ca, cb, rows = family(name)
    k = 30
    nbr = {side: r[:, :k] for side, r in rows.items()}
    want = {True: cref.columns(a, b, ca, cb, k, nbr=nbr[True]), False: cref.columns(b, a, cb, ca, k, nbr=nbr[False])}
    clouds = []
    for p, c in ((a, ca), (b, cb)):
        cloud = PointCloud(p, colors=c.copy())
        cloud.attach_colors_u8(cref.to_bytes(c))
        clouds.append(cloud)
    with CloudPair(*clouds, extent=EXTENT) as u8, pair_of(a, b, ca, cb) as f64:
        for pair in (u8, f64):
            for is_left in (True, False):
                g = getters(pair, is_left)
                for cls, w in zip((GEO, COLOR, JOINT), want[is_left]):
                    assert_same(np.asarray(g[cls](k)), w)
    # one cloud as bytes, the other as float64 rows that are no byte quotients: each side is read in its own form
    ca_off = np.clip(ca + 1e-9, 0.0, 1.0)
    with CloudPair(PointCloud(a, colors=ca_off), clouds[1], extent=EXTENT) as mixed:
        for is_left, (p, q, cp, cq) in ((True, (a, b, ca_off, cb)), (False, (b, a, cb, ca_off))):
            w = cref.columns(p, q, cp, cq, k, nbr=nbr[is_left])
            g = getters(mixed, is_left)
            assert_same(np.asarray(g[COLOR](k)), w[1])
            assert_same(np.asarray(g[JOINT](k)), w[2])
    ca32, cb32 = ca.astype(np.float32), cb.astype(np.float32)
    with pair_of(a, b, ca32, cb32) as f32:
        w = cref.columns(a, b, ca32.astype(np.float64), cb32.astype(np.float64), k, nbr=nbr[True])
        g = getters(f32, True)
        assert_same(np.asarray(g[COLOR](k)), w[1])
        assert_same(np.asarray(g[JOINT](k)), w[2])
    # where the values ARE equal in fp32 and fp64 (dyadic colours) the bits are equal too
    cad, cbd = np.rint(ca * 16.0) / 16.0, np.rint(cb * 16.0) / 16.0
    with pair_of(a, b, cad, cbd) as d64, pair_of(a, b, cad.astype(np.float32), cbd.astype(np.float32)) as d32:
        for is_left in (True, False):
            g64, g32 = getters(d64, is_left), getters(d32, is_left)
            for cls in (COLOR, JOINT):
                assert_same(np.asarray(g32[cls](k)), np.asarray(g64[cls](k)))


# ---- the rows beside the others -------------------------------------------------------------------------------------------------
def coloured_surfaces(n, seed):
    from test_gpu_pointssim import surface
    return surface(n, seed), surface(n, seed + 1)               # (equal sizes: row-indexed point-to-plane normals are legal)


@pytest.mark.parametrize("use_graph", [False, True])
def test_earlier_rows_and_the_geometry_column_do_not_move(use_graph):
    a, b = coloured_surfaces(5000, 221)
    kw = dict(color="ycc", hausdorff=True, point_to_plane=True, hausdorff_rank=(0.5, 0.95))
    with CloudPair(a, b, extent=EXTENT, use_graph=use_graph) as pair:
        before = report(pair, p2d_color=False, **kw)             # every row of today, the geometry rows included
        geometry = [np.asarray(pair.get_left_mahalanobis_distances()).copy(), np.asarray(pair.get_right_mahalanobis_distances()).copy()]
        for _ in range(3 if use_graph else 1):
            if use_graph:
                pair.recompute()                                  # (captured with the new rows the second time, replayed the third)
            both = report(pair, **kw)
            assert list(both)[:len(before)] == list(before)          # the same rows in the same order, then the new ones
            assert {k: v for k, v in bits(both).items() if k in before} == bits(before)
            assert len(both) == len(before) + 12
            assert_same(np.asarray(pair.get_left_mahalanobis_distances()), geometry[0])
            assert_same(np.asarray(pair.get_right_mahalanobis_distances()), geometry[1])
        if use_graph:
            assert pair._graph_id is not None
        assert bits(report(pair, p2d_color=False, **kw)) == bits(before)
    with CloudPair(a, b, extent=EXTENT) as fresh:                 # a pair that builds everything in one call
        assert bits(report(fresh, **kw)) == bits(both)
        assert_same(np.asarray(fresh.get_left_mahalanobis_distances()), geometry[0])


@pytest.mark.parametrize("use_graph", [False, True])
def test_every_option_at_once_equals_each_alone(use_graph):
    a, b = coloured_surfaces(5000, 231)
    attrs = ["geometry", "normal", "curvature", "color"]
    alone = [dict(color="ycc", hausdorff=True), dict(point_to_plane=True, hausdorff=True), dict(plane_to_plane=True, hausdorff=True),
             dict(point_ssim=attrs), dict(hausdorff_rank=(0.5, 0.95), point_to_plane=True),
             dict(point_to_distribution=True, hausdorff=True), dict(point_to_distribution=True, p2d_color=True, hausdorff=True)]
    want = {}
    for kw in alone:
        with CloudPair(a, b, extent=EXTENT) as single:
            with np.errstate(divide="ignore"):
                want.update(bits(MetricCalculator(single).calculate(transform_options(CalculateOptions(**kw))).as_dict()))
    everything = dict(color="ycc", hausdorff=True, point_to_plane=True, plane_to_plane=True, point_ssim=attrs,
                      hausdorff_rank=(0.5, 0.95))
    with CloudPair(a, b, extent=EXTENT, use_graph=use_graph) as pair:
        for _ in range(3 if use_graph else 1):
            got = bits(report(pair, **everything))
            assert set(got) == set(want)
            bad = [key for key in want if got[key] != want[key]]
            assert not bad, bad
            pair.recompute()
        if use_graph:
            assert pair._graph_id is not None


@pytest.mark.parametrize("hausdorff", [False, True])
def test_ties_mean_gives_the_same_rows(hausdorff):
    a, b, ca, cb, _ = family("lattice")
    with pair_of(a, b, ca, cb) as pick:
        want = report(pick, 30, hausdorff=hausdorff)
    with pair_of(a, b, ca, cb, ties="mean") as mean:
        got = report(mean, 30, hausdorff=hausdorff)
    new = [key for key in want if "ColorMahalanobis" in str(key) or "JointMahalanobis" in str(key)]
    assert len(new) == (12 if hausdorff else 6)
    for key in new:
        assert same_bits(got[key], want[key])


def test_with_reconst_and_evaluate_pairs_match_fresh_pairs():
    a = ref.surface(4000, 241)
    ca = cref.smooth_colors(a, 242)
    recs = [ref.surface(3000 + 400 * s, 243 + s) for s in range(3)]
    cols = [cref.smooth_colors(b, 250 + s) for s, b in enumerate(recs)]
    fresh = []
    for b, cb in zip(recs, cols):
        with pair_of(a, b, ca, cb) as single:
            fresh.append(bits(report(single, 30, hausdorff=True)))
    with pair_of(a, recs[0], ca, cols[0]) as pair:
        assert bits(report(pair, 30, hausdorff=True)) == fresh[0]
        cur = pair
        for b, cb, want in zip(recs[1:], cols[1:], fresh[1:]):
            cur = cur.with_reconst(PointCloud(b, colors=cb))
            for metric in (nat.METRIC_P2D, nat.METRIC_P2D_COLOR, nat.METRIC_P2D_JOINT):
                with pytest.raises(nat.PccmStateError):           # new points: every column went with them
                    cur._engine.point_metric(nat.DIR_LEFT, metric)
            assert bits(report(cur, 30, hausdorff=True)) == want
            check_pair(cur, a, b, ca, cb, 30)
        cur.close()
    opts = CalculateOptions(hausdorff=True, point_to_distribution=True, p2d_color=True)
    with np.errstate(divide="ignore"):
        seq = evaluate_pairs([(PointCloud(a, colors=ca), PointCloud(b, colors=cb)) for b, cb in zip(recs, cols)], opts, extent=EXTENT)
    assert [bits(r) for r in seq] == fresh


def test_new_colours_drop_the_colour_columns_and_keep_the_geometry_column():
    a, b, ca, cb, rows = family("surface_smooth")
    k = 30
    nbr = {side: r[:, :k] for side, r in rows.items()}
    new_a, new_b = cref.random_colors(len(a), 261), cref.random_byte_colors(len(b), 262)
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, a)
        eng.set_cloud(1, b)
        eng.set_colors(0, ca)
        eng.set_colors(1, cb)
        eng.nn_pair("auto")
        assert eng.p2d_build(k, BOTH) is True
        mg = {nat.DIR_LEFT: ref.mahalanobis(a, b, k, nbr=nbr[True]), nat.DIR_RIGHT: ref.mahalanobis(b, a, k, nbr=nbr[False])}
        now = [ca, cb]
        for which, upload in ((0, lambda: eng.set_colors(0, new_a)), (1, lambda: eng.set_colors_u8(1, new_b[1]))):
            upload()
            now[which] = (new_a, new_b[0])[which]
            for d in (nat.DIR_LEFT, nat.DIR_RIGHT):              # new colours on EITHER cloud: both directions' colour columns go
                for metric in (nat.METRIC_P2D_COLOR, nat.METRIC_P2D_JOINT):
                    with pytest.raises(nat.PccmStateError):
                        eng.point_metric(d, metric)
                    with pytest.raises(nat.PccmStateError):
                        eng.reduce_total(d, metric)
                assert_same(eng.point_metric(d, nat.METRIC_P2D), mg[d])          # ... the geometry columns stay
            assert eng.p2d_build(k, nat.P2D_GEOMETRY) is False
            assert eng.p2d_build(k, BOTH) is True                                # the rebuild gives the new bits
            assert eng.p2d_build(k, BOTH) is False
            for d, (p, q, cp, cq, side) in ((nat.DIR_LEFT, (a, b, now[0], now[1], True)), (nat.DIR_RIGHT, (b, a, now[1], now[0], False))):
                _, my, mj = cref.columns(p, q, cp, cq, k, nbr=nbr[side])
                assert_same(eng.point_metric(d, nat.METRIC_P2D_COLOR), my)
                assert_same(eng.point_metric(d, nat.METRIC_P2D_JOINT), mj)
                assert_same(eng.point_metric(d, nat.METRIC_P2D), mg[d])
    finally:
        eng.close()


def test_c_calls_and_their_error_codes():
    a, b, ca, cb, rows = family("random")
    k = 30
    nbr = {side: r[:, :k] for side, r in rows.items()}
    lib = nat.load()
    eng = nat.Engine(0)
    CM, JM = nat.METRIC_P2D_COLOR, nat.METRIC_P2D_JOINT
    build = lambda kk, attrs, built: lib.pccm_p2d_build_attrs(eng._ctx, kk, attrs, built)       # noqa: E731
    try:
        built = ctypes.c_int32(7)
        eng.set_cloud(0, a)
        assert build(k, BOTH, ctypes.byref(built)) == nat.E_STATE and built.value == 0          # cloud 1 is missing
        eng.set_cloud(1, b)
        for bad_k in (3, 65, 0, -4):
            assert build(bad_k, BOTH, ctypes.byref(built)) == nat.E_ARG
        for bad_attrs in (4, 8, 7, -1):
            assert build(k, bad_attrs, ctypes.byref(built)) == nat.E_ARG                        # unknown bits
        assert build(k, BOTH, ctypes.byref(built)) == nat.E_STATE and built.value == 0          # no colours at all
        eng.set_colors(0, ca)
        assert build(k, nat.P2D_COLOR, ctypes.byref(built)) == nat.E_STATE                      # cloud 1 has none
        assert build(k, 0, ctypes.byref(built)) == nat.OK and built.value == 1                  # the geometry column is always built
        assert build(k, nat.P2D_GEOMETRY, ctypes.byref(built)) == nat.OK and built.value == 0
        assert lib.pccm_p2d_build(eng._ctx, k, ctypes.byref(built)) == nat.OK and built.value == 0
        eng.nn_pair("auto")
        mg = {nat.DIR_LEFT: ref.mahalanobis(a, b, k, nbr=nbr[True]), nat.DIR_RIGHT: ref.mahalanobis(b, a, k, nbr=nbr[False])}
        assert_same(eng.point_metric(nat.DIR_LEFT, nat.METRIC_P2D), mg[nat.DIR_LEFT])
        for metric in (CM, JM):
            with pytest.raises(nat.PccmStateError):               # geometry only: the colour columns are not built
                eng.point_metric(nat.DIR_LEFT, metric)
        eng.set_colors(1, cb)
        assert_same(eng.point_metric(nat.DIR_LEFT, nat.METRIC_P2D), mg[nat.DIR_LEFT])            # colours do not touch it
        eng.graph_begin()                                         # what is missing would have to be built during capture
        assert build(k, nat.P2D_GEOMETRY, ctypes.byref(built)) == nat.OK and built.value == 0
        assert build(k, BOTH, ctypes.byref(built)) == nat.E_STATE and built.value == 0
        eng.graph_abort()
        eng.nn_pair("auto")
        assert build(k, BOTH, ctypes.byref(built)) == nat.OK and built.value == 1               # geometry found, colour built
        assert build(k, BOTH, ctypes.byref(built)) == nat.OK and built.value == 0
        assert build(k, nat.P2D_COLOR, None) == nat.OK
        want = {}
        for d, (p, q, cp, cq, side) in ((nat.DIR_LEFT, (a, b, ca, cb, True)), (nat.DIR_RIGHT, (b, a, cb, ca, False))):
            _, my, mj = cref.columns(p, q, cp, cq, k, nbr=nbr[side])
            want[d] = {CM: my, JM: mj}
            assert_same(eng.point_metric(d, nat.METRIC_P2D), mg[d])                             # geometry-then-colour: untouched
            for metric in (CM, JM):
                for mode in ("row", "neighbour"):                 # normal_mode is ignored
                    assert_same(eng.point_metric(d, metric, mode), want[d][metric])
                s, mn, mx = eng.reduce_total(d, metric)
                assert same_bits(s, np.sum(want[d][metric])) and mn == np.min(want[d][metric]) and mx == np.max(want[d][metric])
                xvec, mn, mx = eng.reduce(d, metric)
                assert same_bits(eng.finish_sum(xvec, len(want[d][metric])), np.sum(want[d][metric])) and mx == np.max(want[d][metric])
        many = eng.reduce_total_many([(nat.DIR_LEFT, CM), (nat.DIR_RIGHT, nat.METRIC_D1), (nat.DIR_RIGHT, JM), (nat.DIR_LEFT, nat.METRIC_P2D)])
        assert same_bits(many[0][0], np.sum(want[nat.DIR_LEFT][CM])) and same_bits(many[2][0], np.sum(want[nat.DIR_RIGHT][JM]))
        assert same_bits(many[3][0], np.sum(mg[nat.DIR_LEFT]))
        eng.nn(nat.DIR_SELF, "auto")
        for metric in (CM, JM):
            with pytest.raises(ValueError):                       # PCCM_E_ARG: not defined for the self search
                eng.point_metric(nat.DIR_SELF, metric)
            with pytest.raises(ValueError):
                eng.reduce_total(nat.DIR_SELF, metric)
        eng.graph_begin()                                         # everything is there: allowed during capture
        assert build(k, BOTH, ctypes.byref(built)) == nat.OK and built.value == 0
        assert build(12, BOTH, ctypes.byref(built)) == nat.E_STATE
        eng.graph_abort()
        eng.nn_pair("auto")
        assert_same(eng.point_metric(nat.DIR_RIGHT, JM), want[nat.DIR_RIGHT][JM])               # the columns at k = 30 are still there
        # a single combined build at another k equals geometry-then-colour at that k
        assert build(12, nat.P2D_GEOMETRY, ctypes.byref(built)) == nat.OK and built.value == 1
        with pytest.raises(nat.PccmStateError):                   # another k: the colour columns of k = 30 went
            eng.point_metric(nat.DIR_LEFT, CM)
        assert build(12, BOTH, ctypes.byref(built)) == nat.OK and built.value == 1
        staged = {(d, m): eng.point_metric(d, m).copy() for d in (nat.DIR_LEFT, nat.DIR_RIGHT) for m in (nat.METRIC_P2D, CM, JM)}
        assert build(13, BOTH, ctypes.byref(built)) == nat.OK and built.value == 1
        assert build(12, BOTH, ctypes.byref(built)) == nat.OK and built.value == 1
        for (d, m), col in staged.items():
            assert_same(eng.point_metric(d, m), col)
        _, my, mj = cref.columns(a, b, ca, cb, 12, nbr=rows[True][:, :12])
        assert_same(staged[(nat.DIR_LEFT, CM)], my)
        assert_same(staged[(nat.DIR_LEFT, JM)], mj)
        eng.set_cloud(1, b)                                       # new points in either cloud: every column goes
        eng.nn_pair("auto")
        for d in (nat.DIR_LEFT, nat.DIR_RIGHT):
            for metric in (nat.METRIC_P2D, CM, JM):
                with pytest.raises(nat.PccmStateError):
                    eng.point_metric(d, metric)
        assert build(k, BOTH, ctypes.byref(built)) == nat.E_STATE                               # the new cloud 1 has no colours
        eng.set_colors(1, cb)
        eng.set_shard(0, 2)
        assert build(k, BOTH, ctypes.byref(built)) == nat.E_STATE                               # a sharded context
    finally:
        eng.close()


def test_sharded_pairs_and_colourless_clouds_are_refused_before_any_gpu_work():
    a, b, ca, cb, _ = family("random")
    with pair_of(a, b, ca, cb) as pair:
        class Peers:                                              # what Collective(group) says of a group with two ranks
            sharded, group, rank, world = True, object(), 0, 2
        mine = pair._coll
        pair._coll = Peers()
        try:
            with pytest.raises(ValueError, match="sharded"):
                pair.get_left_color_mahalanobis_distances()
            with pytest.raises(ValueError, match="sharded"):
                pair.prefetch_reductions([("p2d_joint", True, 30)])
        finally:
            pair._coll = mine
        with pytest.raises(nat.PccmStateError):                   # nothing was built
            pair._engine.point_metric(nat.DIR_LEFT, nat.METRIC_P2D)
    with CloudPair(PointCloud(a, colors=ca), PointCloud(b), extent=EXTENT) as pair:
        with pytest.raises(ValueError, match="colours"):
            report(pair, 30)
        with pytest.raises(nat.PccmStateError):
            pair._engine.point_metric(nat.DIR_LEFT, nat.METRIC_P2D)
        assert (GEO, True, 30) in report(pair, 30, p2d_color=False)      # the geometry rows alone are still there for it


def test_two_hundred_thousand_points_each():
    """A 200k-point coloured pair against a blocked brute-force restatement (the method of
    test_gpu_p2d.py::test_two_hundred_thousand_points_each): every (query, candidate) distance is formed, block by block (on the GPU
    through torch, one element-wise op at a time), the k + 8 smallest per query go to the host, where the order is decided in
    NumPy by the exact (d2, row) and the cut below the candidates is checked to be strict."""
    import torch
    rng = np.random.default_rng(271)
    n, k = 200_000, 30
    a, b = rng.random((n, 3)), rng.random((n, 3))
    ca, cb = cref.smooth_colors(a, 272), cref.random_byte_colors(n, 273)[0]

    def blocked_rows(p, q, block=1024, extra=8):
        qt = torch.from_numpy(q).to("cuda")
        out = np.empty((len(p), k), dtype=np.int64)
        for s in range(0, len(p), block):
            pt = torch.from_numpy(p[s:s + block]).to("cuda")
            d2 = None
            for x in range(3):
                d = pt[:, None, x] - qt[None, :, x]
                d = d * d
                d2 = d if d2 is None else d2 + d
            cand = torch.topk(d2, k + extra, dim=1, largest=False).indices.cpu().numpy()
            cd2 = ref.sq_dist(p[s:s + block, None, :], q[cand])
            order = np.lexsort((cand, cd2), axis=-1)
            cd2 = np.take_along_axis(cd2, order, axis=-1)
            assert np.all(cd2[:, k - 1] < cd2[:, -1])            # nothing outside the candidates can belong to the first k
            out[s:s + block] = np.take_along_axis(cand, order, axis=-1)[:, :k]
        return out

    nbr = {True: blocked_rows(a, b), False: blocked_rows(b, a)}
    torch.cuda.synchronize()
    with pair_of(a, b, ca, cb) as pair:
        check_pair(pair, a, b, ca, cb, k, nbr=nbr)


def test_command_line(tmp_path):
    a, b, c = ref.surface(3000, 281), ref.surface(2500, 282), ref.surface(2600, 283)
    pa, pb, pc = (str(tmp_path / f"{name}.ply") for name in "abc")
    for s, (path, x) in enumerate(((pa, a), (pb, b), (pc, c))):
        write_point_cloud(path, PointCloud(x, colors=cref.byte_colors(x, 284 + s)[0] if s else cref.random_byte_colors(len(x), 284)[0]),
                          coord_dtype="float")
    ra, rb, rc = read_point_cloud(pa), read_point_cloud(pb), read_point_cloud(pc)
    assert ra.has_colors() and rb.has_colors()
    args = ["--ocloud", pa, "--pcloud", pb, "--pcloud", pc, "--hausdorff", "--point-to-distribution", "--p2d-neighbours", "10",
            "--p2d-color", "--extent", "1", "1", "1"]
    out = CliRunner().invoke(cli, args)
    assert out.exit_code == 0, out.output
    opts = CalculateOptions(hausdorff=True, point_to_distribution=True, p2d_neighbours=10, p2d_color=True)
    texts, csvs = [], []
    for r in (rb, rc):
        with CloudPair(ra, r, extent=EXTENT) as pair:
            with np.errstate(divide="ignore"):
                df = MetricCalculator(pair).calculate(transform_options(opts)).as_df()
            texts.append(df.to_string())
            csvs.append(df.to_csv())
    assert out.output == texts[0] + "\n" + texts[1] + "\n"
    for label in (COLOR, JOINT, "Max" + COLOR, "Max" + JOINT):
        assert label in texts[0] and label + "(symmetric)" in texts[0]
    out = CliRunner().invoke(cli, args + ["--csv"])
    assert out.exit_code == 0 and out.output == csvs[0] + "\n" + csvs[1] + "\n"
    args.remove("--p2d-color")
    plain = CliRunner().invoke(cli, args)
    assert plain.exit_code == 0 and "ColorMahalanobis" not in plain.output and "JointMahalanobis" not in plain.output
    assert "MaxMahalanobisDistance(symmetric)" in plain.output
    out = CliRunner().invoke(cli, ["--ocloud", pa, "--pcloud", pb, "--p2d-color"])
    assert out.exit_code == 2
