"""Host-side contract of the density-aware Chamfer rows (CalculateOptions(dcd=..., dcd_squared=...)): option validation, row order,
labels, keys and dependencies, the default report untouched, the metric nodes over plain arrays and over a CloudPair on an engine
without the density reduction, the checks that run before any GPU work, and which reduction kernel a density job goes to.  Values
are compared on their float64 bits.  No GPU needed."""
import itertools
import os
import shutil
import subprocess
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
import dcd_reference as ref  # noqa: E402
from conftest import load_golden  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def same(x, y):
    return np.float64(x).tobytes() == np.float64(y).tobytes()


def keys(opts):
    return [m._key() for m in transform_options(opts)]


# ---- options -----------------------------------------------------------------------------------------------------------------
def test_options_are_normalised():
    assert CalculateOptions().dcd == () and CalculateOptions().dcd_squared is False
    assert CalculateOptions(dcd=None).dcd == ()
    assert CalculateOptions(dcd=40).dcd == (40.0,)
    assert CalculateOptions(dcd=0).dcd == (0.0,)
    assert CalculateOptions(dcd=[40, 5.0, 40.0, np.float64(1000)]).dcd == (5.0, 40.0, 1000.0)                 # duplicates, unsorted
    assert CalculateOptions(dcd=(a for a in (2.0, 0.25))).dcd == (0.25, 2.0)
    got = CalculateOptions(dcd=[-0.0, 1e300]).dcd
    assert got == (0.0, 1e300) and np.float64(got[0]).tobytes() == np.float64(0.0).tobytes()                   # -0.0 becomes 0.0
    assert all(type(a) is float for a in CalculateOptions(dcd=[np.float32(0.5), 1]).dcd)
    assert CalculateOptions(dcd=[1, 2, 3, 4, 1]).dcd == (1.0, 2.0, 3.0, 4.0)                                   # four DISTINCT values
    assert CalculateOptions(dcd=40, dcd_squared=1).dcd_squared is True
    assert CalculateOptions(fscore=0.5, truncate=0.25, dcd=40).fscore == (0.5,)                                 # each keeps its own


@pytest.mark.parametrize("bad", [True, False, np.True_, float("nan"), float("inf"), -float("inf"), -0.5, -1e-300, "40", b"1",
                                 [40, "x"], [None], [1, 2, 3, 4, 5], [40, True], [1, float("nan")], object()])
def test_bad_alphas_raise(bad):
    with pytest.raises(ValueError, match="dcd"):
        CalculateOptions(dcd=bad)
    with pytest.raises(ValueError, match="dcd"):
        CalculateOptions(None, True, True, chamfer=True, fscore=0.5, truncate=0.1, dcd=bad)


def test_dcd_squared_alone_raises():
    for empty in (None, (), []):
        with pytest.raises(ValueError, match="dcd_squared"):
            CalculateOptions(dcd=empty, dcd_squared=True)
    assert CalculateOptions(dcd=None, dcd_squared=False).dcd == ()


def expected_keys(alphas, squared):
    one = np.ones(4)
    zero = np.zeros(4, dtype=np.int64)
    return list(ref.rows(one, one, zero, zero, 4, 4, alphas, squared))


@pytest.mark.parametrize("alphas, squared", [((40.0,), False), ((40.0, 0.0, 5.0), True), ((1e300, 0.5, 0.0, 1000), False)],
                         ids=["one", "squared", "four"])
@pytest.mark.parametrize("color, hd, p2plane", list(itertools.product([None, "ycc"], [False, True], [False, True])))
def test_rows_follow_every_existing_row(alphas, squared, color, hd, p2plane):
    extra = dict(plane_to_plane=hd, point_ssim=("geometry",) if color else (), hausdorff_rank=(0.9,) if p2plane else None,
                 point_to_distribution=hd, p2d_color=bool(hd and color), resolution_psnr=p2plane, reflectance=bool(color),
                 fscore=(0.01, 0.1) if hd else None, chamfer=bool(color) or p2plane, truncate=(0.5, 0.01) if hd or p2plane else None)
    base = keys(CalculateOptions(color, hd, p2plane, **extra))
    opts = CalculateOptions(color, hd, p2plane, dcd=alphas, dcd_squared=squared, **extra)
    got = keys(opts)
    assert got[:len(base)] == base                                # every other row, the truncated rows included, where it was
    assert got[len(base):] == expected_keys(alphas, squared)
    assert len(got) - len(base) == 3 * len(alphas)
    metrics = transform_options(opts)[len(base):]
    for m in metrics:
        m.value = 0.5
    df = CalculateResult(metrics).as_df()
    labels, sides = [], []
    for a in sorted(alphas):
        tag = f"[{float(a)!r}, squared]" if squared else f"[{float(a)!r}]"
        labels += ["GeoDensityAwareDistance" + tag] * 2 + ["GeoDensityAwareChamfer" + tag]
        sides += [True, False, ""]
    assert list(df["label"]) == labels
    assert list(df["is_left"]) == sides and list(df["point-to-plane"]) == [""] * len(labels)
    assert not any("symmetric" in label for label in labels)      # (as for the F-score: the Chamfer row is the symmetric one)


def test_labels_are_as_stated():
    metrics = transform_options(CalculateOptions(dcd=40))
    for m in metrics:
        m.value = 0.5
    assert list(CalculateResult(metrics).as_df()["label"])[-3:] == ["GeoDensityAwareDistance[40.0]"] * 2 + ["GeoDensityAwareChamfer[40.0]"]
    metrics = transform_options(CalculateOptions(dcd=40, dcd_squared=True))
    for m in metrics:
        m.value = 0.5
    assert list(CalculateResult(metrics).as_df()["label"])[-3:] == ["GeoDensityAwareDistance[40.0, squared]"] * 2 + \
        ["GeoDensityAwareChamfer[40.0, squared]"]


def test_without_the_options_the_rows_are_todays():
    for color, hd, p2plane in itertools.product([None, "ycc"], [False, True], [False, True]):
        base = keys(CalculateOptions(color, hd, p2plane))
        assert keys(CalculateOptions(color, hd, p2plane, dcd=None, dcd_squared=False)) == base
        assert keys(CalculateOptions(color, hd, p2plane, dcd=())) == base
        assert not any("Density" in str(k) for k in base)
    assert len(keys(CalculateOptions("ycc", True, True))) == 32


def test_dependencies_and_keys():
    from open_pcc_metric_amd.metric import (DirectionalMetric, EuclideanDistance, GeoDensityAwareChamfer, GeoDensityAwareDistance,
                                            GeoHausdorffDistance, MatchedRows, PrimaryMetric, SecondaryMetric)
    import open_pcc_metric.metric as alias
    import open_pcc_metric.options as alias_options
    assert alias.GeoDensityAwareChamfer is GeoDensityAwareChamfer and alias.MatchedRows is MatchedRows
    assert alias_options.CalculateOptions(dcd=40, dcd_squared=True).dcd == (40.0,)
    assert GeoDensityAwareDistance(True, 40)._key() == ("GeoDensityAwareDistance", True, 40.0, False)
    assert GeoDensityAwareDistance(False, 40.0, squared=True)._key() == ("GeoDensityAwareDistance", False, 40.0, True)
    assert GeoDensityAwareChamfer(5)._key() == ("GeoDensityAwareChamfer", 5.0, False)
    assert GeoDensityAwareChamfer(5, True)._key() == ("GeoDensityAwareChamfer", 5.0, True)
    assert MatchedRows(True)._key() == ("MatchedRows", True) and MatchedRows(False)._key() == ("MatchedRows", False)
    assert issubclass(MatchedRows, PrimaryMetric) and issubclass(MatchedRows, DirectionalMetric)
    assert issubclass(GeoDensityAwareDistance, SecondaryMetric) and issubclass(GeoDensityAwareDistance, DirectionalMetric)
    assert GeoDensityAwareDistance._pccm_waits is True
    assert GeoDensityAwareDistance(False, 40, squared=True)._pccm_request() == ("density", False, 40.0, True)
    deps = GeoDensityAwareDistance(False, 40.0)._get_dependencies()
    assert [d._key() for d in deps.values()] == [EuclideanDistance(False, False)._key(), ("MatchedRows", False)]
    assert deps["euclidean_distance"]._key() == GeoHausdorffDistance(False, False)._get_dependencies()["euclidean_distance"]._key()
    deps = GeoDensityAwareChamfer(40.0, True)._get_dependencies()
    assert [d._key() for d in deps.values()] == [("GeoDensityAwareDistance", True, 40.0, True), ("GeoDensityAwareDistance", False, 40.0, True)]
    assert nat.MAP_DENSITY == 4
    for name in ("pccm_match_counts", "pccm_reduce_density_prefetch_many", "pccm_reduce_density_total_many"):
        assert name in nat.SYMBOLS


def test_the_calculator_tells_the_pair_about_density_rows():
    class Recorder:
        def __init__(self):
            self.wanted = None

        def prefetch_reductions(self, wanted):
            self.wanted = list(wanted)

    pair = Recorder()
    MetricCalculator(pair)._plan(transform_options(CalculateOptions(dcd=(40, 5), dcd_squared=True)))
    dens = [w for w in pair.wanted if w[0] == "density"]
    assert sorted(dens) == sorted(("density", side, a, True) for side in (True, False) for a in (5.0, 40.0))
    assert (True, False) in pair.wanted and (False, False) in pair.wanted          # the D1 columns they read


# ---- the nodes over plain arrays ---------------------------------------------------------------------------------------------
class StandIn:
    """A pair whose getters return plain ndarrays (as the reference's unit tests inject them)."""
    def __init__(self, left, right, left_idx, right_idx):
        self.d = {True: np.asarray(left, dtype=np.float64), False: np.asarray(right, dtype=np.float64)}
        self.idx = {0: np.asarray(left_idx), 1: np.asarray(right_idx)}

    def get_left_neighbour_distances(self):
        return self.d[True]

    def get_right_neighbour_distances(self):
        return self.d[False]

    def _neighbour_index(self, direction):
        return self.idx[direction]

    def get_boundary_sqrt_distances(self):
        return np.array([0.5, 1.0])

    def get_extent(self):
        return np.array([1.0, 2.0, 3.0])


@pytest.mark.parametrize("squared", [False, True])
def test_nodes_over_plain_arrays_equal_the_restatement(squared):
    rng = np.random.default_rng(0)
    n0, n1 = 9001, 131
    left, right = rng.random(n0) ** 3, np.round(rng.random(n1) * 8) / 4                # the right column is full of ties
    left[:4] = [0.0, 0.25, 0.25, 4.0]
    left_idx = rng.integers(0, n1, n0)                                                 # every row of B shared by ~70 rows of A
    right_idx = rng.permutation(n0)[:n1]                                               # ... and no row of A shared
    alphas = (0.0, 1.0 / float(np.sqrt(np.max(left))), 40.0, 1e300)
    res = MetricCalculator(StandIn(left, right, left_idx, right_idx)).calculate(
        transform_options(CalculateOptions(dcd=alphas, dcd_squared=squared))).as_dict()
    want = ref.rows(left, right, left_idx, right_idx, n0, n1, alphas, squared)
    assert list(res)[-len(want):] == list(want) and len(want) == 3 * 4
    for key, value in want.items():
        assert same(res[key], value), key
        assert 0.0 <= res[key] <= 1.0
    m = np.bincount(left_idx, minlength=n1)
    assert same(res[(ref.SIDE, True, 0.0, squared)], np.sum(1.0 - 1.0 / m[left_idx]) / n0)
    assert same(res[(ref.SIDE, False, 0.0, squared)], 0.0)                             # nobody shares: every term is 1 - 1 / 1
    assert same(res[(ref.SIDE, True, 1e300, squared)], ref.huge_alpha_side(left, left_idx, n1))
    assert same(res[(ref.BOTH, 40.0, squared)], (res[(ref.SIDE, True, 40.0, squared)] + res[(ref.SIDE, False, 40.0, squared)]) / np.float64(2))
    # the coverage reading of alpha = 0: 1 - (distinct matched rows) / n, up to the rounding of the sum
    assert abs(res[(ref.SIDE, True, 0.0, squared)] - (1.0 - np.count_nonzero(m) / n0)) < 1e-12


# ---- a CloudPair on an engine without the density reduction, over the golden pairs --------------------------------------------
def golden_pair(name, **kw):
    g = load_golden(name)
    pair = CloudPair(PointCloud(g["a"], g["na"]), PointCloud(g["b"], g["nb"]), extent=list(g["extent"]), _engine=OracleEngine(), **kw)
    return g, pair


@pytest.mark.parametrize("name", ["uniform_300_color", "lattice_ties_400", "identical_100"])
def test_engine_without_the_calls_falls_back_to_the_host_formula(name):
    from open_pcc_metric_amd.cloud_pair import density_on_host
    for call in ("reduce_density_total_many", "reduce_density_prefetch_many", "match_counts"):
        assert not hasattr(OracleEngine, call)
    g, pair = golden_pair(name)
    n0, n1 = len(g["a"]), len(g["b"])
    left, right = g["left_d2"], g["right_d2"]
    left_idx, right_idx = pair._neighbour_index(nat.DIR_LEFT), pair._neighbour_index(nat.DIR_RIGHT)
    top = float(np.sqrt(np.max(left)))
    alphas = ref.alphas_of((0.0, 1.0 / top if top > 0 else 1.0, 1e300))
    for squared in (False, True):
        with np.errstate(divide="ignore"):
            res = MetricCalculator(pair).calculate(transform_options(CalculateOptions(None, True, dcd=alphas, dcd_squared=squared))).as_dict()
            base = MetricCalculator(pair).calculate(transform_options(CalculateOptions(None, True))).as_dict()
        for key, value in base.items():                          # every earlier row is what it was
            assert same(res[key], value), key
        want = ref.rows(left, right, left_idx, right_idx, n0, n1, alphas, squared)
        assert list(res)[len(base):] == list(want)
        for key, value in want.items():
            assert same(res[key], value), (key, res[key], value)
        if name == "identical_100":                               # a cloud against itself: every point is matched once, at distance 0
            assert all(same(res[k], 0.0) for k in want)
    column = pair.get_left_neighbour_distances()
    counts = pair.match_counts(True)
    assert counts.dtype == np.uint32 and np.array_equal(counts, ref.counts(left_idx, n1)) and int(counts.sum()) == n0
    assert np.array_equal(pair.match_counts(False), ref.counts(right_idx, n0))
    for alpha, squared in ((0.0, False), (alphas[1], False), (alphas[1], True), (1e300, True)):
        got = column.density(alpha, squared)
        assert all(same(a, b) for a, b in zip(got, ref.totals(left, left_idx, n1, alpha, squared))), (alpha, squared)
        assert all(same(a, b) for a, b in zip(got, density_on_host(left, left_idx, counts, alpha, squared)))
    for bad in (float("nan"), -1.0, float("inf")):
        with pytest.raises(ValueError):
            column.density(bad)
    with pytest.raises(ValueError):
        pair.get_boundary_sqrt_distances().density(1.0)           # defined on the two directions' D1 columns


def test_sharded_pairs_and_mean_ties_are_refused_before_the_engine_is_touched():
    from open_pcc_metric_amd.options import check_dcd
    check_dcd(CalculateOptions(), ties="mean", group=object())    # no such rows: nothing to check
    check_dcd(CalculateOptions(dcd=40))
    check_dcd(CalculateOptions(dcd=40), ties="pick", group=None)
    with pytest.raises(ValueError, match="sharded"):
        check_dcd(CalculateOptions(dcd=40), group=object())
    with pytest.raises(ValueError, match="mean"):
        check_dcd(CalculateOptions(dcd=40), ties="mean")
    _, pair = golden_pair("uniform_300_color")

    class Peers:                                                  # what Collective(group) says of a group with two ranks
        sharded, group, rank, world = True, object(), 0, 2
    whole = pair._coll
    pair._coll = Peers()
    calls = list(pair._engine.calls)
    with pytest.raises(ValueError, match="sharded"):
        MetricCalculator(pair).calculate(transform_options(CalculateOptions(dcd=40)))
    with pytest.raises(ValueError, match="sharded"):
        pair.match_counts()
    assert pair._engine.calls == calls
    pair._coll = whole
    pair.ties = "mean"
    with pytest.raises(ValueError, match="mean"):
        MetricCalculator(pair).calculate(transform_options(CalculateOptions(dcd=40)))
    with pytest.raises(ValueError, match="mean"):
        pair.get_left_neighbour_distances().density(40.0)
    with pytest.raises(ValueError, match="mean"):
        pair.match_counts(False)
    assert pair._engine.calls == calls


def test_cli_refuses_a_bad_alpha_before_any_context(tmp_path, monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a GPU context was asked for")
    monkeypatch.setattr(nat, "acquire_engine", no_context)
    monkeypatch.setattr(nat, "Engine", no_context)
    rng = np.random.default_rng(0)
    pa, pb = str(tmp_path / "a.xyz"), str(tmp_path / "b.xyz")
    write_point_cloud(pa, PointCloud(rng.random((20, 3))))
    write_point_cloud(pb, PointCloud(rng.random((20, 3))))
    for extra in (["--dcd", "-0.1"], ["--dcd", "nan"], ["--dcd", "inf"], ["--dcd", "x"], ["--dcd-squared"], ["--dcd-squared", "1"],
                  ["--dcd", "40", "--ties", "mean"], sum((["--dcd", str(a)] for a in (1, 2, 3, 4, 5)), [])):
        out = CliRunner().invoke(cli, ["--ocloud", pa, "--pcloud", pb] + extra)
        assert out.exit_code == 2, (extra, out.output, out.exception)
    # (nothing was read either: the files of a refused call need not exist)
    out = CliRunner().invoke(cli, ["--ocloud", str(tmp_path / "none.ply"), "--pcloud", pb, "--dcd", "40", "--dcd", "-1"])
    assert out.exit_code == 2, (out.output, out.exception)
    out = CliRunner().invoke(cli, ["--help"])
    assert out.exit_code == 0 and "--dcd" in out.output and "--dcd-squared" in out.output


# ---- which kernel a density job goes to ---------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
def test_a_density_job_has_no_lean_kernel(tmp_path):
    exe = str(tmp_path / "dcd_shape_host")
    build = subprocess.run(
        [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "open_pcc_metric_amd", "csrc"),
         os.path.join(ROOT, "tests", "dcd_shape_host_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    lines = run.stdout.splitlines()
    assert len(lines) == 18 * 9 + 2
    for line in lines[:-2]:
        head, verdict = line.split(": ")
        f = head.split()
        cfg, m0, m1 = int(f[3]), int(f[7]), int(f[8])
        assert m0 in (0, 4, 6) and m1 in (0, 4, 6)
        mapped = m0 != 0 or (cfg == 0 and m1 != 0)                 # (cfg 0: the two-column jobs)
        assert verdict == ("general" if mapped else "lean"), line
    assert sum(1 for ln in lines[:-2] if ln.endswith(": lean")) == 6 * 1 + 12 * 3       # map 0 on every reduced column
    assert lines[-2] == "keys ok"
    assert int(lines[-1].split()[1]) <= 4096                       # UnitJobs still fits the kernel arguments
