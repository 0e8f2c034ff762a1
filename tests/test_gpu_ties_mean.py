"""ties="mean" on the GPU (include/pccm.h, PCCM_TIES_MEAN): every equidistant nearest neighbour, averaged in ascending row
order, stands for the matched point of both directional sweeps.  The yardstick is the NumPy restatement of tests/ties_reference.py
(dense chunked enumeration of the tie sets; the CPU oracle's arithmetic for projections and colours)."""
import os

import numpy as np
import pytest
from click.testing import CliRunner

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import write_point_cloud
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud
from open_pcc_metric_amd.sequence import evaluate_pairs
from oracle import oracle as orc
from ties_reference import MeanOracleEngine, tie_mean, tie_sets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lattice_pair(seed=3, side=24, count=2600):
    rng = np.random.default_rng(seed)
    a = np.unique(rng.integers(0, side, (count, 3)), axis=0).astype(np.float32)
    b = np.unique(rng.integers(0, side, (count, 3)), axis=0).astype(np.float32)
    n = min(len(a), len(b))
    a, b = a[rng.permutation(len(a))[:n]], b[rng.permutation(len(b))[:n]]      # equal sizes: row-indexed normals are legal
    na, nb = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    ca, cb = rng.integers(0, 256, (n, 3)) / 255.0, rng.integers(0, 256, (n, 3)) / 255.0
    return PointCloud(a, na, ca), PointCloud(b, nb, cb)


def report(pair, color="ycc"):
    with np.errstate(divide="ignore"):
        res = MetricCalculator(pair).calculate(transform_options(CalculateOptions(color, True, True))).as_dict()
    return {k: np.asarray(v, dtype=np.float64).tobytes() for k, v in res.items()}


def oracle_report(a, b, mode, color="ycc", ties="mean"):
    return report(CloudPair(a, b, extent=[24.0, 24.0, 24.0], normal_index=mode, ties=ties, _engine=MeanOracleEngine()), color)


def p2p_column(pair, is_left):
    """EuclideanDistance(point_to_plane=True) per point: the square of the projection column (metric.py:179), on the device."""
    return np.asarray(np.square(pair.point_to_plane_column(is_left)))


@pytest.mark.parametrize("mode", ["row", "neighbour"])
@pytest.mark.parametrize("color", ["rgb", "ycc", "yuv"])
def test_lattice_rows_match_the_restatement(mode, color):
    a, b = lattice_pair()
    with CloudPair(a, b, extent=[24.0, 24.0, 24.0], normal_index=mode, ties="mean") as pair:
        got = report(pair, color)
        for is_left, (q, r, nr, cr) in ((True, (a, b, b.normals, b.colors)), (False, (b, a, a.normals, a.colors))):
            _, sets = tie_sets(q.points, r.points)
            assert max(len(s) for s in sets) > 1
            c = tie_mean(r.points, sets)
            nrm = np.asarray(nr) if mode == "row" else tie_mean(nr, sets)
            want = np.square(orc.point_to_plane(q.points, c, np.arange(len(c)), nrm, normal_index=mode))
            assert p2p_column(pair, is_left).tobytes() == want.tobytes()
            neigh = np.asarray(pair.get_left_neighbour_colors() if is_left else pair.get_right_neighbour_colors())
            assert neigh.tobytes() == tie_mean(cr, sets).tobytes()
            assert np.array_equal(pair.tie_counts(is_left), [len(s) for s in sets])
    assert got == oracle_report(a, b, mode, color)
    with CloudPair(a, b, extent=[24.0, 24.0, 24.0], normal_index=mode) as pick:
        base = report(pick, color)
    assert base == oracle_report(a, b, mode, color, ties="pick")
    differ = {k for k in got if got[k] != base[k]}
    assert differ and all(k[k[0] == "SymmetricMetric"] in ("GeoMSE", "GeoPSNR", "GeoHausdorffDistance", "GeoHausdorffDistancePSNR", "ColorMSE", "ColorPSNR",
                                   "ColorHausdorffDistance", "ColorHausdorffDistancePSNR") for k in differ)
    d1 = [k for k in got if k[0].startswith("Geo") and k[2] is False]
    assert d1 and all(got[k] == base[k] for k in d1)                           # D1 rows: the pick's, bit for bit


@pytest.mark.parametrize("scheme", ["rgb", "ycc", "yuv"])
def test_ctypes_set_ties_then_colour_reduce(scheme):
    a, b = lattice_pair(seed=5)
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, a.points)
        eng.set_cloud(1, b.points)
        eng.set_colors(0, a.colors)
        eng.set_colors(1, b.colors)
        eng.set_ties("mean")
        eng.nn_pair("auto")
        sums, maxs = eng.color_reduce(nat.DIR_LEFT, scheme, 1.0)
        avg = tie_mean(b.colors, tie_sets(a.points, b.points)[1])
        _, wsum, wmax = orc.color_columns(a.colors, avg, np.arange(len(avg)), scheme, 1.0)
        assert np.asarray(sums).tobytes() == wsum.tobytes() and np.asarray(maxs).tobytes() == wmax.tobytes()
        eng.reset()                                     # back to the pick (pccm_ctx_reset)
        eng.set_cloud(0, a.points)
        eng.set_cloud(1, b.points)
        eng.nn_pair("auto")
        with pytest.raises(nat.PccmStateError):
            eng.tie_counts(nat.DIR_LEFT)
    finally:
        eng.close()


def test_tie_free_data_gives_the_picks_report():
    rng = np.random.default_rng(11)
    for n in (1000, 20000, 1 << 20):
        a, b = rng.random((n, 3), dtype=np.float32), rng.random((n, 3), dtype=np.float32)
        small = n <= 20000
        ca = cb = None
        if small:
            ca, cb = rng.integers(0, 256, (n, 3)) / 255.0, rng.integers(0, 256, (n, 3)) / 255.0
        pa, pb = PointCloud(a, rng.standard_normal((n, 3)), ca), PointCloud(b, rng.standard_normal((n, 3)), cb)
        color = "ycc" if small else None
        for mode in ("row", "neighbour"):
            with CloudPair(pa, pb, extent=[1, 1, 1], normal_index=mode) as pick:
                want = report(pick, color)
            with CloudPair(pa, pb, extent=[1, 1, 1], normal_index=mode, ties="mean") as mean:
                assert report(mean, color) == want
                assert np.all(mean.tie_counts(True) == 1)


def test_permuting_b_leaves_the_mean_report_alone():
    a, b = lattice_pair(seed=7)
    rng = np.random.default_rng(1)
    a, b = (PointCloud(c.points, rng.integers(-3, 4, c.points.shape).astype(np.float64), c.colors) for c in (a, b))   # exact sums
    perm = rng.permutation(len(b.points))
    bp = PointCloud(b.points[perm], b.normals[perm], b.colors[perm])
    out = {}
    for ties in ("pick", "mean"):
        for name, bb in (("b", b), ("bp", bp)):
            with CloudPair(a, bb, extent=[24.0, 24.0, 24.0], normal_index="neighbour", ties=ties) as pair:
                out[ties, name] = report(pair, "ycc")
    # A's rows against B: the same virtual neighbours, the same row order (the other direction sums B's rows in the new order)
    geo = [("GeoMSE", True, True), ("GeoPSNR", True, True), ("GeoHausdorffDistance", True, True), ("GeoHausdorffDistance", False, True)]
    assert all(out["mean", "b"][k] == out["mean", "bp"][k] for k in geo)
    for k in out["mean", "b"]:
        if k[0] in ("ColorMSE", "GeoMSE"):
            # A's colour rows: averages of the same colours in another order (a few ulp); B's rows are also summed in B's new order
            x = np.frombuffer(out["mean", "b"][k]); y = np.frombuffer(out["mean", "bp"][k])
            assert np.allclose(x, y, rtol=(8 * np.finfo(float).eps) if k[1] is True else 1e-12, atol=0), k
    assert out["pick", "b"][geo[0]] != out["pick", "bp"][geo[0]]                            # the pick's D2 moves


def test_outlier_beyond_the_cell_walk_gets_its_whole_tie_set():
    # B: a 64^3 lattice and, away from it, the 24 points at distance sqrt(5) around c = (100, 100, 100).  A: points inside the
    # lattice (one nearest neighbour each, settled by the cell walk); c itself (24 ties: more than the walk's list holds); and an
    # outlier beyond a corner of the lattice, equidistant from (0, 31, 0) and (0, 32, 0), whose ball holds EVERY cell of any grid
    # over these clouds on all three axes -- far more than the walk's 4096.  Both go to the exact scan.
    g = np.stack(np.meshgrid(*[np.arange(64)] * 3, indexing="ij"), -1).reshape(-1, 3)
    off = np.array([p for p in np.ndindex(5, 5, 5) if np.sum(np.square(np.array(p) - 2)) == 5]) - 2
    assert len(off) == 24
    b = np.concatenate([g, 100 + off]).astype(np.float32)
    a = np.concatenate([g[:500] + 0.25, [[100.0, 100.0, 100.0], [-1000.0, 31.5, -1000.0]]]).astype(np.float32)
    with CloudPair(PointCloud(a), PointCloud(b), extent=[64, 64, 64], ties="mean") as pair:
        k = pair.tie_counts(True)
        assert k[-2] == 24 and k[-1] == 2
        assert pair._engine.tie_scan_queries(0) == 2          # those two, and only they, went past the cell walk to the exact scan
        ev = np.asarray(pair.get_left_error_vector())
        assert ev[-2].tolist() == [0.0, 0.0, 0.0]                           # the mean of the 24 is c
        assert ev[-1].tolist() == [-1000.0, 0.0, -1000.0]                   # the midpoint of (0, 31, 0) and (0, 32, 0)
        _, sets = tie_sets(a, b, chunk=64)
        assert np.array_equal(k, [len(s) for s in sets])
        assert ev.tobytes() == (a.astype(np.float64) - tie_mean(b, sets)).tobytes()

def test_engines_agree_and_a_voxel_surface_matches_the_restatement():
    a, b = lattice_pair(seed=9)
    reps = []
    for eng in ("auto", "grid", "brute"):
        with CloudPair(a, b, extent=[24.0, 24.0, 24.0], nn_engine=eng, normal_index="neighbour", ties="mean") as pair:
            reps.append(report(pair))
    assert reps[0] == reps[1] == reps[2]
    # voxelised sphere shells (integer content: the voxel engine's territory)
    rng = np.random.default_rng(2)
    def shell(r, n):
        v = rng.standard_normal((n, 3))
        v = np.round(64 + r * v / np.linalg.norm(v, axis=1, keepdims=True))
        return np.unique(v, axis=0).astype(np.float32)
    sa, sb = shell(50.0, 30000), shell(50.5, 30000)
    n = min(len(sa), len(sb))
    sa, sb = sa[:n], sb[:n]
    pa = PointCloud(sa, rng.standard_normal((n, 3)), rng.integers(0, 256, (n, 3)) / 255.0)
    pb = PointCloud(sb, rng.standard_normal((n, 3)), rng.integers(0, 256, (n, 3)) / 255.0)
    with CloudPair(pa, pb, extent=[128.0, 128.0, 128.0], normal_index="neighbour", ties="mean") as pair:
        lo, hi = np.minimum(sa.min(0), sb.min(0)), np.maximum(sa.max(0), sb.max(0))
        assert pair._engine.nn_stats(0)["splits"] == int(np.prod(np.floor((hi - lo) / 8.0) + 1)), "not the voxel-brick grid"
        got = report(pair)
        assert pair._engine.tie_scan_queries(0) == 0
    want = report(CloudPair(pa, pb, extent=[128.0, 128.0, 128.0], normal_index="neighbour", ties="mean", _engine=MeanOracleEngine()))
    assert got == want


def test_resident_pairs_keep_the_policy():
    a, b = lattice_pair(seed=3)
    _, b2 = lattice_pair(seed=4)
    fresh = oracle_report(a, b, "neighbour")
    with CloudPair(a, b, extent=[24.0, 24.0, 24.0], normal_index="neighbour", ties="mean", use_graph=True) as pair:
        assert report(pair) == fresh
        pair.recompute()
        assert report(pair) == fresh
        pair.recompute()
        assert report(pair) == fresh
        nxt = pair.with_reconst(b2)
    try:
        assert nxt.ties == "mean"
        assert report(nxt) == oracle_report(a, b2, "neighbour")
    finally:
        nxt.close()
    opts = CalculateOptions("ycc", True, True)
    seq = evaluate_pairs([(a, b), (a, b2)], opts, extent=[24.0, 24.0, 24.0], normal_index="neighbour", ties="mean")
    for (x, y), got in zip([(a, b), (a, b2)], seq):
        with CloudPair(x, y, extent=[24.0, 24.0, 24.0], normal_index="neighbour", ties="mean") as single:
            with np.errstate(divide="ignore"):
                want = MetricCalculator(single).calculate(transform_options(opts)).as_dict()
        assert {k: np.asarray(v).tobytes() for k, v in got.items()} == {k: np.asarray(v).tobytes() for k, v in want.items()}


def test_cli_ties_mean_prints_the_api_text(tmp_path):
    a, b = lattice_pair(seed=3)
    pa, pb = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    write_point_cloud(pa, a, coord_dtype="float")
    write_point_cloud(pb, b, coord_dtype="float")
    from open_pcc_metric_amd.io import read_point_cloud
    ra, rb = read_point_cloud(pa), read_point_cloud(pb)
    args = ["--ocloud", pa, "--pcloud", pb, "--color", "ycc", "--hausdorff", "--point-to-plane", "--extent", "24", "24", "24"]
    with np.errstate(divide="ignore"):
        out = CliRunner().invoke(cli, args + ["--ties", "mean"])
        plain = CliRunner().invoke(cli, args)
    assert out.exit_code == 0 and plain.exit_code == 0, out.output + plain.output
    with CloudPair(ra, rb, extent=[24.0, 24.0, 24.0], ties="mean") as pair:
        with np.errstate(divide="ignore"):
            text = MetricCalculator(pair).calculate(transform_options(CalculateOptions("ycc", True, True))).as_df().to_string()
    assert out.output == text + "\n"
    assert out.output != plain.output
