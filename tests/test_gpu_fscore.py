"""F-score, precision and recall rows on the GPU (include/pccm.h, pccm_count_many; CalculateOptions(fscore=...)).

A count has no rounding: counts are compared as integers, ratios and F-scores with ``==`` on their float64 bits against the NumPy
restatement of tests/fscore_reference.py, applied to the oracle's columns and to the GPU's own fetched columns."""
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
from open_pcc_metric_amd.sequence import evaluate_pairs
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fscore_reference as ref  # noqa: E402
import variant_rows as vr  # noqa: E402
from test_gpu_ties_mean import lattice_pair  # noqa: E402

D1, D2, PR = nat.METRIC_D1, nat.METRIC_D2, nat.METRIC_PROJ


def same(x, y):
    return np.float64(x).tobytes() == np.float64(y).tobytes()


def report(pair, taus, hausdorff=False, p2plane=False, color=None, frame=False, **kw):
    opts = CalculateOptions(color, hausdorff, p2plane, fscore=taus, **kw)
    with np.errstate(divide="ignore"):
        res = MetricCalculator(pair).calculate(transform_options(opts))
        return res.as_df() if frame else res.as_dict()


def oracle_columns(a, b):
    return orc.nn(a, b, method="kdtree")[1], orc.nn(b, a, method="kdtree")[1]


def gpu_columns(pair):
    return np.asarray(pair.get_left_neighbour_distances()), np.asarray(pair.get_right_neighbour_distances())


def check_rows(res, left, right, taus):
    """The F-score rows of a report -- the last ones, in the stated order -- against the restatement over the two columns."""
    want = ref.rows(left, right, taus)
    assert list(res)[-len(want):] == list(want)
    for key, value in want.items():
        assert same(res[key], value), (key, res[key], value)


def uniform(n, m, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3)).astype(np.float32), rng.random((m, 3)).astype(np.float32)


def thresholds_of(column):
    """Below the column's minimum, at its median, at the square root of one of its elements, above its maximum.  Squaring a
    rounded square root need not give the element back, so the third threshold is taken from an element for which it does: the
    restatement's count then includes that element (checked by the caller)."""
    col = np.sort(np.asarray(column, dtype=np.float64))
    lo = 0.5 * float(np.sqrt(col[0])) if col[0] > 0 else 0.0
    planted = next((float(np.sqrt(v)) for v in col[len(col) // 3:] if np.sqrt(v) * np.sqrt(v) == v), float(np.sqrt(col[-1])))
    return (lo, float(np.sqrt(col[len(col) // 2])), planted, 2.0 * float(np.sqrt(col[-1])) + 1.0), planted


# ---- reports against the oracle's columns and the GPU's own fetched columns -----------------------------------------------------
@functools.lru_cache(maxsize=16)
def uniform_case(n, m):
    a, b = uniform(n, m, 7 * n + m)
    return a, b, oracle_columns(a, b)


@pytest.mark.parametrize("engine", ["grid", "brute"])
@pytest.mark.parametrize("n, m", [(1, 1), (2, 2), (255, 255), (257, 257), (4095, 4095), (4097, 4097), (8193, 8193), (100_003, 100_003),
                                  (300, 200), (5000, 4097)])
def test_uniform_pairs(n, m, engine):
    a, b, (left, right) = uniform_case(n, m)
    taus, planted = thresholds_of(left)
    if n > 2:                                  # the count includes the element the third threshold was taken from
        assert planted * planted in left
        assert ref.count_le(left, planted * planted) == np.count_nonzero(left < planted * planted) + np.count_nonzero(left == planted * planted)
        assert ref.count_le(left, taus[0] * taus[0]) == 0
    assert ref.count_le(left, taus[3] * taus[3]) == n
    with CloudPair(PointCloud(a), PointCloud(b), extent=[1.0, 1.0, 1.0], nn_engine=engine) as pair:
        res = report(pair, taus)
        own = gpu_columns(pair)
    check_rows(res, left, right, taus)
    check_rows(res, own[0], own[1], taus)
    assert res[("GeoInlierRatio", True, max(taus))] == 1.0 and res[("GeoFScore", max(taus))] == 1.0


def test_the_capped_grid():
    """More than 256 x 4096 rows per job: every workgroup walks its rows more than once."""
    n = 1_100_003
    a, b = uniform(n, n, 99)
    with CloudPair(PointCloud(a), PointCloud(b), extent=[1.0, 1.0, 1.0]) as pair:
        left, right = gpu_columns(pair)
        taus, _ = thresholds_of(left)
        res = report(pair, taus)
        assert pair._engine.count_many([(0, D1, np.inf), (1, D1, float(np.median(right)))]) == \
            [n, int(np.count_nonzero(right <= np.median(right)))]
    check_rows(res, left, right, taus)


# ---- planted integer lattice ------------------------------------------------------------------------------------------------
LATTICE_TAUS = (0.0, 1.0, 1.4142135623730951, 2.0)


def test_planted_lattice_under_both_tie_policies():
    a, b = lattice_pair()
    left, right = oracle_columns(np.asarray(a.points), np.asarray(b.points))
    assert set(np.unique(left)) >= {0.0, 1.0, 2.0} and np.all(left == np.round(left))      # exact small integers
    rows = {}
    for ties in ("pick", "mean"):
        with CloudPair(a, b, extent=[24.0, 24.0, 24.0], ties=ties) as pair:
            rows[ties] = report(pair, LATTICE_TAUS)
            own = gpu_columns(pair)
        check_rows(rows[ties], left, right, LATTICE_TAUS)
        check_rows(rows[ties], own[0], own[1], LATTICE_TAUS)
    want = ref.rows(left, right, LATTICE_TAUS)
    assert all(same(rows["pick"][k], rows["mean"][k]) for k in want)
    n = len(left)
    # tau = 0 counts exactly the coincident points; a row with d2 == tau * tau is counted (1.0 and 4.0 exactly; the square of the
    # rounded sqrt(2) is 2.0000000000000004: the rows at 2 are in)
    assert rows["pick"][("GeoInlierRatio", True, 0.0)] == np.count_nonzero(left == 0.0) / n
    assert rows["pick"][("GeoInlierRatio", True, 1.0)] == np.count_nonzero(left <= 1.0) / n > np.count_nonzero(left < 1.0) / n
    assert rows["pick"][("GeoInlierRatio", True, 1.4142135623730951)] == np.count_nonzero(left <= 2.0) / n
    assert rows["pick"][("GeoInlierRatio", False, 2.0)] == np.count_nonzero(right <= 4.0) / n > np.count_nonzero(right < 4.0) / n


# ---- through the engine (ABI) -------------------------------------------------------------------------------------------------
def test_every_record_form_is_counted_as_it_is_reduced():
    """Engine x matched rows kept x normals' precision x normal_index x projection fused: plain columns, 32-byte records and
    16-byte matched records with deferred projection.  The thresholds come from the oracle's columns, so that the counts run on
    the search result as the search left it; afterwards each count is held against count_le of the GPU's own column too
    (pccm_nn_fetch for D1, pccm_point_metric for D2)."""
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
                for (d, met), col in want.items():                   # the median and an element of each column
                    req += [(d, met, float(np.median(col))), (d, met, float(col[len(col) // 7]))]
                expect = [ref.count_le(want[(d, met)], x) for d, met, x in req]
                assert all(c >= 1 for c in expect)
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
                                eng.count_prefetch_many(req, mode)
                            got = eng.count_many(req, mode)
                            assert "k_unit_jobs" in eng.last_path(nat.PATH_REDUCE), what
                            assert got == expect, (what, got, expect)
                            own = {(d, met): eng.fetch_nn(d, want_idx=False)[1] if met == D1 else eng.point_metric(d, met, mode)
                                   for d, met in want}
                            assert got == [ref.count_le(own[(d, met)], x) for d, met, x in req], what
                            assert eng.count_many(req[:3] + [(0, D2, np.inf), (1, D2, -1.0)], mode) == expect[:3] + [n, 0], what
    finally:
        eng.close()


def engine_pair(n=5000, m=4097, seed=61, normals=True):
    a, b = uniform(n, m, seed)
    eng = nat.Engine(0)
    eng.set_cloud(0, a); eng.set_cloud(1, b)
    if normals:
        eng.set_normals(0, vr._unit(n, 1)); eng.set_normals(1, vr._unit(m, 2))
    return eng, a, b


def test_eight_thresholds_on_one_column_and_edge_values():
    eng, a, b = engine_pair()
    try:
        eng.nn_pair("grid")
        left, right = oracle_columns(a, b)
        xs = [float(v) for v in np.quantile(left, [0.1, 0.25, 0.4, 0.55, 0.7, 0.85, 0.95])]
        xs = xs[:4] + [xs[1]] + xs[4:]                               # eight thresholds, two of them equal: two rounds, one merged
        assert len(xs) == 8
        got = eng.count_many([(0, D1, x) for x in xs])
        assert got == [ref.count_le(left, x) for x in xs] and got[4] == got[1]
        mixed = [(1, D1, xs[0]), (0, D1, xs[7]), (1, D1, np.inf), (0, D1, -np.inf), (1, D1, float(right[17])), (0, D1, float(left[0]))]
        eng.count_prefetch_many(mixed)
        assert eng.count_many(mixed) == [ref.count_le(right if d else left, x) for d, _, x in mixed]
        assert eng.count_many([(0, D1, np.inf), (1, D1, np.inf), (0, D1, -np.inf), (1, D1, -0.0)]) == [len(a), len(b), 0, 0]
    finally:
        eng.close()
    eng = nat.Engine(0)
    try:                                                             # an identical pair: every distance is 0.0, and 0.0 <= -0.0
        eng.set_cloud(0, a); eng.set_cloud(1, a.copy())
        eng.nn_pair("grid")
        assert eng.count_many([(0, D1, -0.0), (1, D1, 0.0), (0, D1, -np.inf), (1, D1, -5e-324)]) == [len(a), len(a), 0, 0]
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
        args = [eng._ctx, k, arr(*[r[0] for r in reqs]), arr(*[r[1] for r in reqs]), arr(*(modes or [1] * k)),
                (ctypes.c_double * k)(*[r[2] for r in reqs])]
        buf = (ctypes.c_int64 * max(k, 1))()
        rc = fn(*args, buf) if out else fn(*args)
        return rc, list(buf)[:k]
    both = ((lib.pccm_count_prefetch_many, False), (lib.pccm_count_many, True))
    try:
        eng.set_cloud(0, a); eng.set_cloud(1, b)
        for fn, out in both:
            assert call(fn, [(0, D1, 1.0)], out=out)[0] == nat.E_STATE                # no search result yet
        eng.nn_pair("grid")
        left, right = oracle_columns(a, b)
        for fn, out in both:
            assert call(fn, [(2, D1, 1.0)], out=out)[0] == nat.E_ARG                  # PCCM_DIR_SELF
            assert call(fn, [(0, PR, 1.0)], out=out)[0] == nat.E_ARG                  # other metrics
            assert call(fn, [(0, nat.METRIC_ANGULAR, 1.0)], out=out)[0] == nat.E_ARG
            assert call(fn, [(0, D1, float("nan"))], out=out)[0] == nat.E_ARG         # NaN
            assert call(fn, [(0, D1, 1.0)] * 9, out=out)[0] == nat.E_ARG              # n <= 8
            assert call(fn, [], out=out)[0] == nat.OK
            # D2 without normals fails as the reduction does
            total = (ctypes.c_double * 3)()
            assert call(fn, [(0, D2, 1.0)], out=out)[0] == lib.pccm_reduce_total(eng._ctx, 0, D2, 1, total) == nat.E_STATE
        assert lib.pccm_count_many(eng._ctx, 1, None, None, None, None, None) == nat.E_ARG
        eng.set_normals(0, na); eng.set_normals(1, nb)
        assert call(lib.pccm_count_many, [(0, D2, 1.0)], modes=[0])[0] == nat.E_RANGE  # row-indexed normals out of range
        rc, got = call(lib.pccm_count_many, [(1, D2, np.inf), (0, D1, float(np.median(left)))], modes=[0, 0])
        assert rc == nat.OK and got == [m, ref.count_le(left, np.median(left))]
        # staleness: a count enqueued on a search whose cloud was replaced is never consumed
        x = float(np.median(left))
        assert call(lib.pccm_count_prefetch_many, [(0, D1, x)], out=False)[0] == nat.OK
        b2 = (b * np.float32(0.9)).astype(np.float32)
        eng.set_cloud(1, b2)
        assert call(lib.pccm_count_many, [(0, D1, x)])[0] == nat.E_STATE
        eng.nn_pair("grid")
        rc, got = call(lib.pccm_count_many, [(0, D1, x), (1, D1, x)])
        left2, right2 = oracle_columns(a, b2)
        assert rc == nat.OK and got == [ref.count_le(left2, x), ref.count_le(right2, x)] and got[0] != ref.count_le(left, x)
        eng.set_shard(0, 2)
        assert call(lib.pccm_count_many, [(0, D1, 1.0)])[0] == nat.E_STATE             # a sharded context
        assert call(lib.pccm_count_prefetch_many, [(0, D1, 1.0)], out=False)[0] == nat.E_STATE
    finally:
        eng.close()


# ---- graph replay and reuse -----------------------------------------------------------------------------------------------------
def test_graph_replays_and_new_points():
    n = 50_000
    a, b = uniform(n, n, 31)
    left, right = oracle_columns(a, b)
    taus, _ = thresholds_of(left)
    b2 = (b * np.float32(0.97)).astype(np.float32)
    left2, right2 = oracle_columns(a, b2)
    with CloudPair(PointCloud(a), PointCloud(b), extent=[1.0, 1.0, 1.0], use_graph=True) as pair:
        rows = []
        for _ in range(4):                     # eager, capture, two replays
            rows.append(report(pair, taus, hausdorff=True))
            pair.recompute()
        assert pair._graph_id is not None
        for r in rows:
            check_rows(r, left, right, taus)
            assert list(r) == list(rows[0]) and all(same(r[k], rows[0][k]) for k in r)
        pair._engine.set_cloud(1, b2)          # another cloud of the same size under the same pair
        pair.clouds = (pair.clouds[0], PointCloud(b2))
        pair.recompute()
        second = report(pair, taus, hausdorff=True)
        for _ in range(3):                     # (new points: captured anew, then replayed)
            pair.recompute()
            again = report(pair, taus, hausdorff=True)
            assert list(again) == list(second) and all(same(again[k], second[k]) for k in second)
        assert pair._graph_id is not None
    check_rows(second, left2, right2, taus)
    keys = list(ref.rows(left, right, taus))
    assert any(not same(second[k], rows[0][k]) for k in keys)


def test_with_reconst_and_evaluate_pairs():
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
            got.append(report(pair, taus, hausdorff=True))
    finally:
        pair.close()
    for k in range(3):
        check_rows(got[k], *oracle_columns(a, np.asarray(decoded[k].points)), taus)
    opts = CalculateOptions(None, True, False, fscore=taus)
    for res, mine in zip(evaluate_pairs([(origin, d) for d in decoded], opts, workers=1, extent=[1.0, 1.0, 1.0]), got):
        assert list(res) == list(mine) and all(same(res[k], mine[k]) for k in res)


# ---- nothing leaves the GPU, nothing else moves ---------------------------------------------------------------------------------
def test_no_column_is_materialised_and_other_rows_do_not_move(monkeypatch):
    n = 8193
    rng = np.random.default_rng(42)
    a, b = uniform(n, n, 41)
    na, nb = vr._unit(n, 1), vr._unit(n, 2)
    ca, cb = rng.integers(0, 256, (n, 3)) / 255.0, rng.integers(0, 256, (n, 3)) / 255.0
    ra, rb = rng.integers(0, 65536, n).astype(np.float64), rng.integers(0, 65536, n).astype(np.float64)
    every = dict(hausdorff=True, p2plane=True, color="ycc", plane_to_plane=True, point_ssim=("geometry", "normal", "curvature", "color"),
                 hausdorff_rank=(0.5, 0.99), point_to_distribution=True, p2d_color=True, resolution_psnr=True, reflectance=True)
    taus = (0.0, 0.004, 0.01, 0.05)

    def clouds():
        return PointCloud(a, na, ca, reflectance=ra), PointCloud(b, nb, cb, reflectance=rb)
    with CloudPair(*clouds(), extent=[1.0, 1.0, 1.0]) as pair:
        plain = report(pair, None, **every)
    with CloudPair(*clouds(), extent=[1.0, 1.0, 1.0]) as pair:
        def never(self):
            raise AssertionError(f"{self!r} was copied to the host")
        monkeypatch.setattr(DeviceColumn, "_materialise", never)
        full = report(pair, taus, **every)
        monkeypatch.undo()
        check_rows(full, *gpu_columns(pair), taus)
    assert list(full)[:len(plain)] == list(plain) and len(full) == len(plain) + 12
    for key, value in plain.items():           # exactly the same values under all other keys
        assert np.asarray(full[key], dtype=np.float64).tobytes() == np.asarray(value, dtype=np.float64).tobytes(), key


# ---- command line -------------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path):
    n = 5000
    a, b = uniform(n, n, 51)
    b = (a + np.float32(0.02) * (b - np.float32(0.5))).astype(np.float32)
    pa, pb = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    write_point_cloud(pa, PointCloud(a))
    write_point_cloud(pb, PointCloud(b))
    args = ["--ocloud", pa, "--pcloud", pb, "--hausdorff"]
    left, right = oracle_columns(a, b)
    want = ref.rows(left, right, (0.01, 0.05))
    assert 0.0 < want[("GeoFScore", 0.01)] < want[("GeoFScore", 0.05)] <= 1.0
    expect = [[f"{k[0]}[{k[-1]!r}]"] + ([str(k[1]), str(v)] if len(k) == 3 else [str(v)]) for k, v in want.items()]
    base = CliRunner().invoke(cli, args)
    text = CliRunner().invoke(cli, args + ["--fscore", "0.05", "--fscore", "0.01"])
    csv = CliRunner().invoke(cli, args + ["--fscore", "0.05", "--fscore", "0.01", "--csv"])
    assert base.exit_code == 0 and text.exit_code == 0 and csv.exit_code == 0, (base.output, text.output, text.exception, csv.exception)
    base_lines, lines = base.output.rstrip("\n").split("\n"), text.output.rstrip("\n").split("\n")
    assert len(lines) == len(base_lines) + 6
    assert [ln.split() for ln in lines[1:len(base_lines)]] == [ln.split() for ln in base_lines[1:]]       # today's rows, then the new ones
    assert [ln.split()[1:] for ln in lines[len(base_lines):]] == expect
    rows = [ln.split(",") for ln in csv.output.rstrip("\n").split("\n")]
    assert len(rows) == len(base_lines) + 6
    assert [[r[1]] + [f for f in r[2:] if f] for r in rows[-6:]] == expect
