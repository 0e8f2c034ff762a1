"""Host-side contract of the F-score rows (CalculateOptions(fscore=...)): option validation, row order, labels and keys, the
default report untouched, the metric nodes over plain arrays and over a CloudPair on an engine without the count call, and the
checks that run before any GPU work.  Counts are integers and ratios are compared on their float64 bits.  No GPU needed."""
import itertools
import os
import sys

import numpy as np
import pytest
from click.testing import CliRunner

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import CalculateResult, MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import write_point_cloud
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fscore_reference as ref  # noqa: E402
from conftest import load_golden  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402


def same(x, y):
    return np.float64(x).tobytes() == np.float64(y).tobytes()


def keys(opts):
    return [m._key() for m in transform_options(opts)]


# ---- options -----------------------------------------------------------------------------------------------------------------
def test_option_is_normalised():
    assert CalculateOptions().fscore == ()
    assert CalculateOptions(fscore=None).fscore == ()
    assert CalculateOptions(fscore=0.01).fscore == (0.01,)
    assert CalculateOptions(fscore=0).fscore == (0.0,)
    assert CalculateOptions(fscore=[0.05, 0.01, 0.05, np.float64(0.02)]).fscore == (0.01, 0.02, 0.05)       # duplicates, unsorted
    assert CalculateOptions(fscore=(t for t in (2.0, 0.25))).fscore == (0.25, 2.0)
    assert CalculateOptions(fscore=[0.0, -0.0, 1]).fscore == (0.0, 1.0)
    assert all(type(t) is float for t in CalculateOptions(fscore=[np.float32(0.5), 1]).fscore)
    assert CalculateOptions(fscore=[0.1, 0.2, 0.3, 0.4, 0.1]).fscore == (0.1, 0.2, 0.3, 0.4)                 # four DISTINCT values


@pytest.mark.parametrize("bad", [True, False, np.True_, float("nan"), float("inf"), -float("inf"), -0.5, -1e-300, "0.5", b"1",
                                 [0.5, "x"], [None], [0.1, 0.2, 0.3, 0.4, 0.5], [0.5, True], [0.1, float("nan")], object()])
def test_bad_thresholds_raise(bad):
    with pytest.raises(ValueError):
        CalculateOptions(fscore=bad)
    with pytest.raises(ValueError):                               # whether or not the rows are what the caller is after
        CalculateOptions(None, True, True, hausdorff_rank=0.5, fscore=bad)


@pytest.mark.parametrize("taus", [(0.01,), (0.5, 0.0, 0.01, 0.1)], ids=["one", "four"])
@pytest.mark.parametrize("color, hd, p2plane", list(itertools.product([None, "ycc"], [False, True], [False, True])))
def test_rows_follow_every_existing_row(taus, color, hd, p2plane):
    extra = dict(plane_to_plane=hd, point_ssim=("geometry",) if color else (), hausdorff_rank=(0.9,) if p2plane else None,
                 point_to_distribution=hd, p2d_color=bool(hd and color), resolution_psnr=p2plane, reflectance=bool(color))
    base = keys(CalculateOptions(color, hd, p2plane, **extra))
    opts = CalculateOptions(color, hd, p2plane, fscore=taus, **extra)
    got = keys(opts)
    assert got[:len(base)] == base                                # every other row, reflectance included, where it was
    assert got[len(base):] == ref.keys(taus)
    metrics = transform_options(opts)[len(base):]
    for m in metrics:
        m.value = 0.5
    df = CalculateResult(metrics).as_df()
    labels, sides = [], []
    for t in sorted(taus):
        labels += [f"GeoInlierRatio[{t!r}]"] * 2 + [f"GeoFScore[{t!r}]"]
        sides += [True, False, ""]
    assert list(df["label"]) == labels
    assert list(df["is_left"]) == sides and list(df["point-to-plane"]) == [""] * len(labels)


def test_without_the_option_the_rows_are_todays():
    for color, hd, p2plane in itertools.product([None, "ycc"], [False, True], [False, True]):
        base = keys(CalculateOptions(color, hd, p2plane))
        assert keys(CalculateOptions(color, hd, p2plane, fscore=None)) == base
        assert keys(CalculateOptions(color, hd, p2plane, fscore=())) == base
        assert not any("Inlier" in str(k) or "FScore" in str(k) for k in base)
    assert len(keys(CalculateOptions("ycc", True, True))) == 32


def test_dependencies_and_keys():
    from open_pcc_metric_amd.metric import GeoFScore, GeoHausdorffDistance, GeoInlierRatio
    import open_pcc_metric.metric as alias
    assert alias.GeoFScore is GeoFScore and alias.GeoInlierRatio is GeoInlierRatio
    f = GeoFScore(0.01)
    assert f._key() == ("GeoFScore", 0.01)
    deps = f._get_dependencies()
    assert deps["precision"]._key() == ("GeoInlierRatio", False, 0.01) and deps["recall"]._key() == ("GeoInlierRatio", True, 0.01)
    euclid = deps["recall"]._get_dependencies()["euclidean_distance"]
    assert euclid._key() == GeoHausdorffDistance(True, False)._get_dependencies()["euclidean_distance"]._key()
    assert GeoInlierRatio._pccm_waits is True


def test_fscore_of_nothing_is_zero():
    assert same(ref.fscore(0.0, 0.0), 0.0)
    from open_pcc_metric_amd.metric import GeoFScore, GeoInlierRatio
    p, r = GeoInlierRatio(False, 1.0), GeoInlierRatio(True, 1.0)
    f = GeoFScore(1.0)
    for pv, rv in ((0.0, 0.0), (1.0, 1.0), (0.5, 0.0), (0.3, 0.7), (1 / 3, 2 / 3)):
        p.value, r.value = np.float64(pv), np.float64(rv)
        f.calculate(precision=p, recall=r)
        assert same(f.value, ref.fscore(pv, rv)) and type(f.value) is np.float64
    p.value, r.value = np.float64(0.0), np.float64(0.0)
    f.calculate(precision=p, recall=r)
    assert same(f.value, 0.0)


# ---- the nodes over plain arrays ---------------------------------------------------------------------------------------------
class StandIn:
    """A pair whose getters return plain ndarrays (as the reference's unit tests inject them)."""
    def __init__(self, left, right):
        self.d = {True: np.asarray(left, dtype=np.float64), False: np.asarray(right, dtype=np.float64)}

    def get_left_neighbour_distances(self):
        return self.d[True]

    def get_right_neighbour_distances(self):
        return self.d[False]

    def get_boundary_sqrt_distances(self):
        return np.array([0.5, 1.0])

    def get_extent(self):
        return np.array([1.0, 2.0, 3.0])


def test_nodes_over_plain_arrays_equal_the_restatement():
    rng = np.random.default_rng(0)
    left, right = rng.random(257) ** 3, np.round(rng.random(131) * 8) / 4            # the right column is full of ties
    left[:5] = [0.0, -0.0, np.inf, 0.25, 0.25]
    taus = (0.0, 0.5, 1.0, float(np.sqrt(left[100])))
    with np.errstate(divide="ignore"):                            # (the column holds an inf: the PSNR rows beside these)
        res = MetricCalculator(StandIn(left, right)).calculate(transform_options(CalculateOptions(fscore=taus))).as_dict()
    want = ref.rows(left, right, taus)
    assert list(res)[-len(want):] == list(want)
    for key, value in want.items():
        assert same(res[key], value), key
    assert res[("GeoInlierRatio", True, 0.0)] == 2 / 257          # 0.0 and -0.0 both lie within 0
    assert ref.count_le(left, 0.25) == np.count_nonzero(left <= 0.25) >= 2            # a row equal to the threshold is counted
    assert ref.count_le(left, -0.0) == 2 and ref.count_le(left, np.inf) == 257 and ref.count_le(left, -np.inf) == 0


# ---- a CloudPair on an engine without the count call, over the golden pairs ---------------------------------------------------
def golden_pair(name, **kw):
    g = load_golden(name)
    pair = CloudPair(PointCloud(g["a"], g["na"]), PointCloud(g["b"], g["nb"]), extent=list(g["extent"]), _engine=OracleEngine(), **kw)
    return g, pair


@pytest.mark.parametrize("name", ["uniform_300_color", "lattice_ties_400", "identical_100"])
def test_engine_without_count_falls_back_to_the_column(name):
    assert not hasattr(OracleEngine, "count_many") and not hasattr(OracleEngine, "count_prefetch_many")
    g, pair = golden_pair(name)
    left, right = g["left_d2"], g["right_d2"]
    mid = np.sort(left)[len(left) // 2]
    taus = ref.thresholds((0.0, float(np.sqrt(mid)), float(np.sqrt(np.max(left))), float(np.sqrt(np.max(left))) * 2.0 + 1.0))
    with np.errstate(divide="ignore"):
        res = MetricCalculator(pair).calculate(transform_options(CalculateOptions(None, True, fscore=taus))).as_dict()
        base = MetricCalculator(pair).calculate(transform_options(CalculateOptions(None, True))).as_dict()
    for key, value in base.items():                               # every earlier row is what it was
        assert same(res[key], value), key
    want = ref.rows(left, right, taus)
    assert list(res)[len(base):] == list(want)
    for key, value in want.items():
        assert same(res[key], value), (key, res[key], value)
    column = pair.get_left_neighbour_distances()
    for x in (0.0, -0.0, mid, np.inf, -np.inf):
        assert column.count_le(x) == ref.count_le(left, x)
    with pytest.raises(ValueError):
        column.count_le(float("nan"))
    assert same(res[("GeoFScore", taus[-1])], 1.0)                # beyond the largest distance everything is an inlier
    if name == "identical_100":
        assert all(same(res[k], 1.0) for k in want)               # tau = 0 on identical clouds: every point is reproduced
    if name == "lattice_ties_400":                                # integer squared distances: the median itself is counted
        assert res[("GeoInlierRatio", True, float(np.sqrt(mid)))] == np.count_nonzero(left <= mid) / len(left) >= 0.5


def test_sharded_pairs_are_refused_before_the_engine_is_touched():
    from open_pcc_metric_amd.options import check_fscore
    check_fscore(CalculateOptions(), group=object())              # no F-score rows: nothing to check
    check_fscore(CalculateOptions(fscore=0.5))
    check_fscore(CalculateOptions(fscore=0.5), group=None)
    with pytest.raises(ValueError, match="sharded"):
        check_fscore(CalculateOptions(fscore=0.5), group=object())
    _, pair = golden_pair("uniform_300_color")

    class Peers:                                                  # what Collective(group) says of a group with two ranks
        sharded, group, rank, world = True, object(), 0, 2
    pair._coll = Peers()
    calls = list(pair._engine.calls)
    with pytest.raises(ValueError, match="sharded"):
        MetricCalculator(pair).calculate(transform_options(CalculateOptions(fscore=0.5)))
    assert pair._engine.calls == calls


def test_cli_refuses_a_bad_threshold_before_any_context(tmp_path, monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a GPU context was asked for")
    monkeypatch.setattr(nat, "acquire_engine", no_context)
    monkeypatch.setattr(nat, "Engine", no_context)
    rng = np.random.default_rng(0)
    pa, pb = str(tmp_path / "a.xyz"), str(tmp_path / "b.xyz")
    write_point_cloud(pa, PointCloud(rng.random((20, 3))))
    write_point_cloud(pb, PointCloud(rng.random((20, 3))))
    for extra in (["--fscore", "-0.1"], ["--fscore", "nan"], ["--fscore", "inf"], ["--fscore", "x"],
                  sum((["--fscore", str(t)] for t in (0.1, 0.2, 0.3, 0.4, 0.5)), [])):
        out = CliRunner().invoke(cli, ["--ocloud", pa, "--pcloud", pb] + extra)
        assert out.exit_code == 2, (extra, out.output, out.exception)
    # (nothing was read either: the files of a refused call need not exist)
    out = CliRunner().invoke(cli, ["--ocloud", str(tmp_path / "none.ply"), "--pcloud", pb, "--fscore", "-1"])
    assert out.exit_code == 2, (out.output, out.exception)
    out = CliRunner().invoke(cli, ["--help"])
    assert out.exit_code == 0 and "--fscore" in out.output
