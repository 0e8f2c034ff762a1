"""Host-side contract of the Chamfer and truncated-distance rows (CalculateOptions(chamfer=..., truncate=...)): option validation,
row order, labels and keys, the default report untouched, the metric nodes over plain arrays and over a CloudPair on an engine
without the mapped reduction, the checks that run before any GPU work, and which reduction kernel a mapped job goes to.  Values
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
from open_pcc_metric_amd.cloud_pair import CloudPair, mapped_on_host
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import write_point_cloud
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chamfer_reference as ref  # noqa: E402
from conftest import load_golden  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def same(x, y):
    return np.float64(x).tobytes() == np.float64(y).tobytes()


def keys(opts):
    return [m._key() for m in transform_options(opts)]


# ---- options -----------------------------------------------------------------------------------------------------------------
def test_options_are_normalised():
    assert CalculateOptions().chamfer is False and CalculateOptions().truncate == ()
    assert CalculateOptions(chamfer=1).chamfer is True
    assert CalculateOptions(truncate=None).truncate == ()
    assert CalculateOptions(truncate=0.01).truncate == (0.01,)
    assert CalculateOptions(truncate=0).truncate == (0.0,)
    assert CalculateOptions(truncate=[0.05, 0.01, 0.05, np.float64(0.02)]).truncate == (0.01, 0.02, 0.05)     # duplicates, unsorted
    assert CalculateOptions(truncate=(t for t in (2.0, 0.25))).truncate == (0.25, 2.0)
    assert CalculateOptions(truncate=[0.0, -0.0, 1]).truncate == (0.0, 1.0)
    assert all(type(t) is float for t in CalculateOptions(truncate=[np.float32(0.5), 1]).truncate)
    assert CalculateOptions(truncate=[0.1, 0.2, 0.3, 0.4, 0.1]).truncate == (0.1, 0.2, 0.3, 0.4)               # four DISTINCT values
    assert CalculateOptions(fscore=0.5, truncate=0.25).fscore == (0.5,)                                          # each keeps its own


@pytest.mark.parametrize("bad", [True, False, np.True_, float("nan"), float("inf"), -float("inf"), -0.5, -1e-300, "0.5", b"1",
                                 [0.5, "x"], [None], [0.1, 0.2, 0.3, 0.4, 0.5], [0.5, True], [0.1, float("nan")], object()])
def test_bad_thresholds_raise(bad):
    with pytest.raises(ValueError, match="truncate"):
        CalculateOptions(truncate=bad)
    with pytest.raises(ValueError, match="truncate"):
        CalculateOptions(None, True, True, chamfer=True, fscore=0.5, truncate=bad)


def expected_keys(chamfer, taus, p2plane):
    n = 8
    left_d2 = np.ones(n) if p2plane else None
    return list(ref.rows(np.ones(n), np.ones(n), chamfer, taus, left_d2, left_d2))


@pytest.mark.parametrize("chamfer, taus", [(True, ()), (False, (0.5, 0.01)), (True, (0.5, 0.0, 0.01, 0.1))], ids=["chamfer", "truncate", "both"])
@pytest.mark.parametrize("color, hd, p2plane", list(itertools.product([None, "ycc"], [False, True], [False, True])))
def test_rows_follow_every_existing_row(chamfer, taus, color, hd, p2plane):
    extra = dict(plane_to_plane=hd, point_ssim=("geometry",) if color else (), hausdorff_rank=(0.9,) if p2plane else None,
                 point_to_distribution=hd, p2d_color=bool(hd and color), resolution_psnr=p2plane, reflectance=bool(color),
                 fscore=(0.01, 0.1) if hd else None)
    base = keys(CalculateOptions(color, hd, p2plane, **extra))
    opts = CalculateOptions(color, hd, p2plane, chamfer=chamfer, truncate=taus, **extra)
    got = keys(opts)
    assert got[:len(base)] == base                                # every other row, the F-score rows included, where it was
    assert got[len(base):] == expected_keys(chamfer, taus, p2plane)
    metrics = transform_options(opts)[len(base):]
    for m in metrics:
        m.value = 0.5
    df = CalculateResult(metrics).as_df()
    labels, sides, planes = [], [], []
    if chamfer:
        for p2p in (False, True) if p2plane else (False,):
            labels += ["GeoMeanDistance"] * 2 + ["GeoMeanDistance(symmetric)"]
            sides += [True, False, ""]
            planes += [p2p, p2p, ""]
        labels += ["GeoChamferL1", "GeoChamferL2"]
        sides += ["", ""]
        planes += ["", ""]
    for t in sorted(taus):
        for name in ("GeoTruncatedMSE", "GeoTruncatedMeanDistance") if chamfer else ("GeoTruncatedMSE",):
            labels += [f"{name}[{t!r}]"] * 2 + [f"{name}[{t!r}](symmetric)"]
            sides += [True, False, ""]
            planes += [""] * 3
    assert list(df["label"]) == labels
    assert list(df["is_left"]) == sides and list(df["point-to-plane"]) == planes


def test_without_the_options_the_rows_are_todays():
    for color, hd, p2plane in itertools.product([None, "ycc"], [False, True], [False, True]):
        base = keys(CalculateOptions(color, hd, p2plane))
        assert keys(CalculateOptions(color, hd, p2plane, chamfer=False, truncate=None)) == base
        assert keys(CalculateOptions(color, hd, p2plane, truncate=())) == base
        assert not any("Chamfer" in str(k) or "Truncated" in str(k) or "MeanDistance" in str(k) for k in base)
    assert len(keys(CalculateOptions("ycc", True, True))) == 32


def test_dependencies_and_keys():
    from open_pcc_metric_amd.metric import (GeoChamferL1, GeoChamferL2, GeoHausdorffDistance, GeoMeanDistance, GeoMSE, GeoTruncatedMeanDistance,
                                            GeoTruncatedMSE)
    import open_pcc_metric.metric as alias
    import open_pcc_metric.options as alias_options
    assert alias.GeoChamferL1 is GeoChamferL1 and alias.GeoTruncatedMSE is GeoTruncatedMSE
    assert alias_options.CalculateOptions(chamfer=True, truncate=0.5).truncate == (0.5,)
    assert GeoMeanDistance(True, False)._key() == ("GeoMeanDistance", True, False)
    assert GeoChamferL1()._key() == ("GeoChamferL1",) and GeoChamferL2()._key() == ("GeoChamferL2",)
    assert GeoTruncatedMSE(False, 0.01)._key() == ("GeoTruncatedMSE", False, 0.01)
    assert GeoTruncatedMeanDistance(True, 0.01)._key() == ("GeoTruncatedMeanDistance", True, 0.01)
    deps = GeoChamferL1()._get_dependencies()
    assert [d._key() for d in deps.values()] == [("GeoMeanDistance", True, False), ("GeoMeanDistance", False, False)]
    deps = GeoChamferL2()._get_dependencies()
    assert [d._key() for d in deps.values()] == [GeoMSE(True, False)._key(), GeoMSE(False, False)._key()]
    euclid = GeoTruncatedMSE(True, 0.5)._get_dependencies()["euclidean_distance"]
    assert euclid._key() == GeoHausdorffDistance(True, False)._get_dependencies()["euclidean_distance"]._key()
    # what the calculator tells prefetch_reductions: (is_left, point_to_plane, root, clamp) with the clamp tau * tau in fp64
    assert GeoMeanDistance(False, True)._pccm_request() == ("mapped", False, True, True, None)
    assert GeoTruncatedMSE(True, 0.1)._pccm_request() == ("mapped", True, False, False, float(np.float64(0.1) * np.float64(0.1)))
    assert GeoTruncatedMeanDistance(False, 0.1)._pccm_request() == ("mapped", False, False, True, float(np.float64(0.1) * np.float64(0.1)))
    for cls in (GeoMeanDistance, GeoTruncatedMSE, GeoTruncatedMeanDistance):
        assert cls._pccm_waits is True


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
    left, right = rng.random(9001) ** 3, np.round(rng.random(131) * 8) / 4            # the right column is full of ties
    left[:4] = [0.0, 0.25, 0.25, 4.0]
    taus = (0.0, 0.5, float(np.sqrt(left[100])), 3.0)
    opts = CalculateOptions(chamfer=True, truncate=taus)
    res = MetricCalculator(StandIn(left, right)).calculate(transform_options(opts)).as_dict()
    want = ref.rows(left, right, True, taus)
    assert list(res)[-len(want):] == list(want) and len(want) == 5 + 6 * 4
    for key, value in want.items():
        assert same(res[key], value), key
    assert same(res[("GeoChamferL2",)], res[("GeoMSE", True, False)] + res[("GeoMSE", False, False)])
    assert same(res[("GeoTruncatedMSE", True, 0.0)], 0.0) and same(res[("GeoTruncatedMeanDistance", False, 0.0)], 0.0)
    assert same(res[("GeoTruncatedMSE", True, 3.0)], res[("GeoMSE", True, False)])                  # nothing is clipped at 3
    assert same(res[("GeoTruncatedMeanDistance", True, 3.0)], res[("GeoMeanDistance", True, False)])
    assert res[("GeoTruncatedMSE", True, 0.5)] < res[("GeoMSE", True, False)]                       # ... and something at 0.5
    only = MetricCalculator(StandIn(left, right)).calculate(transform_options(CalculateOptions(truncate=taus))).as_dict()
    want = ref.rows(left, right, False, taus)
    assert list(only)[-len(want):] == list(want) and all(same(only[k], v) for k, v in want.items())
    for which, x in ((ref.ROOT, None), (ref.CLAMP, 0.25), (ref.CLAMP | ref.ROOT, 0.25), (ref.CLAMP, np.inf), (ref.CLAMP, -1.0)):
        got = mapped_on_host(left, bool(which & ref.ROOT), x if which & ref.CLAMP else None)
        assert all(same(g, w) for g, w in zip(got, ref.totals(left, which, x)))


# ---- a CloudPair on an engine without the mapped reduction, over the golden pairs ---------------------------------------------
def golden_pair(name, **kw):
    g = load_golden(name)
    pair = CloudPair(PointCloud(g["a"], g["na"]), PointCloud(g["b"], g["nb"]), extent=list(g["extent"]), _engine=OracleEngine(), **kw)
    return g, pair


@pytest.mark.parametrize("name", ["uniform_300_color", "lattice_ties_400", "identical_100"])
def test_engine_without_the_call_falls_back_to_the_column(name):
    assert not hasattr(OracleEngine, "reduce_map_total_many") and not hasattr(OracleEngine, "reduce_map_prefetch_many")
    g, pair = golden_pair(name)
    left, right = g["left_d2"], g["right_d2"]
    mid = np.sort(left)[len(left) // 2]
    taus = ref.thresholds((0.0, float(np.sqrt(mid)), float(np.sqrt(np.max(left))) * 2.0 + 1.0))
    with np.errstate(divide="ignore"):
        res = MetricCalculator(pair).calculate(transform_options(CalculateOptions(None, True, chamfer=True, truncate=taus))).as_dict()
        base = MetricCalculator(pair).calculate(transform_options(CalculateOptions(None, True))).as_dict()
    for key, value in base.items():                               # every earlier row is what it was
        assert same(res[key], value), key
    want = ref.rows(left, right, True, taus)
    assert list(res)[len(base):] == list(want)
    for key, value in want.items():
        assert same(res[key], value), (key, res[key], value)
    column = pair.get_left_neighbour_distances()
    for root, clamp in ((True, None), (False, mid), (True, mid), (False, np.inf), (True, 0.0), (False, None)):
        which = (ref.ROOT if root else 0) | (ref.CLAMP if clamp is not None else 0)
        assert all(same(a, b) for a, b in zip(column.mapped(root=root, clamp=clamp), ref.totals(left, which, clamp))), (root, clamp)
    with pytest.raises(ValueError):
        column.mapped(clamp=float("nan"))
    assert same(res[("GeoTruncatedMSE", True, taus[-1])], res[("GeoMSE", True, False)])
    assert same(res[("GeoTruncatedMeanDistance", True, taus[-1])], res[("GeoMeanDistance", True, False)])
    if name == "identical_100":
        assert all(same(res[k], 0.0) for k in want)


def test_sharded_pairs_are_refused_before_the_engine_is_touched():
    from open_pcc_metric_amd.options import check_chamfer, check_truncate
    check_chamfer(CalculateOptions(), group=object())             # no such rows: nothing to check
    check_truncate(CalculateOptions(), group=object())
    check_chamfer(CalculateOptions(chamfer=True))
    check_truncate(CalculateOptions(truncate=0.5), group=None)
    with pytest.raises(ValueError, match="sharded"):
        check_chamfer(CalculateOptions(chamfer=True), group=object())
    with pytest.raises(ValueError, match="sharded"):
        check_truncate(CalculateOptions(truncate=0.5), group=object())
    _, pair = golden_pair("uniform_300_color")

    class Peers:                                                  # what Collective(group) says of a group with two ranks
        sharded, group, rank, world = True, object(), 0, 2
    pair._coll = Peers()
    calls = list(pair._engine.calls)
    for opts in (CalculateOptions(chamfer=True), CalculateOptions(truncate=0.5)):
        with pytest.raises(ValueError, match="sharded"):
            MetricCalculator(pair).calculate(transform_options(opts))
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
    for extra in (["--truncate", "-0.1"], ["--truncate", "nan"], ["--truncate", "inf"], ["--truncate", "x"], ["--chamfer", "1"],
                  sum((["--truncate", str(t)] for t in (0.1, 0.2, 0.3, 0.4, 0.5)), [])):
        out = CliRunner().invoke(cli, ["--ocloud", pa, "--pcloud", pb] + extra)
        assert out.exit_code == 2, (extra, out.output, out.exception)
    # (nothing was read either: the files of a refused call need not exist)
    out = CliRunner().invoke(cli, ["--ocloud", str(tmp_path / "none.ply"), "--pcloud", pb, "--chamfer", "--truncate", "-1"])
    assert out.exit_code == 2, (out.output, out.exception)
    out = CliRunner().invoke(cli, ["--help"])
    assert out.exit_code == 0 and "--chamfer" in out.output and "--truncate" in out.output


# ---- which kernel a mapped job goes to ----------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
def test_a_mapped_job_has_no_lean_kernel(tmp_path):
    exe = str(tmp_path / "chamfer_shape_host")
    build = subprocess.run(
        [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "open_pcc_metric_amd", "csrc"),
         os.path.join(ROOT, "tests", "chamfer_shape_host_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    lines = run.stdout.splitlines()
    assert len(lines) == 18 * 16 + 1
    for line in lines[:-1]:
        head, verdict = line.split(": ")
        f = head.split()
        cfg, m0, m1 = int(f[3]), int(f[7]), int(f[8])
        mapped = m0 != 0 or (cfg == 0 and m1 != 0)                 # (cfg 0: the two-column jobs)
        assert verdict == ("general" if mapped else "lean"), line
    assert sum(1 for ln in lines[:-1] if ln.endswith(": lean")) == 6 * 1 + 12 * 4       # map 0 on every reduced column
    assert int(lines[-1].split()[1]) <= 4096                       # UnitJobs still fits the kernel arguments
