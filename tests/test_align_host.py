"""Host-side contract of alignment (``CloudPair(transform=..., align="icp")``; INTEGRATION.md, "Alignment") without a GPU: the
planted registration cases on the NumPy restatement, option and command-line validation, ``CloudPair`` driven end to end on a CPU
double that can move a cloud, and pccm_stale.h's points_moved in a sanitized stand-alone program."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from click.testing import CliRunner

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd import align as al
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import write_point_cloud
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import align_reference as ref  # noqa: E402
from align_engine import AlignOracleEngine  # noqa: E402

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def same(x, y):
    return np.asarray(x, dtype=np.float64).tobytes() == np.asarray(y, dtype=np.float64).tobytes()


# ---- the planted cases on the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("degrees", [0.5, 1.0])
def test_small_motions_are_recovered_in_three_iterations(degrees):
    """A jittered 10^3 lattice moved by 0.5 / 1 degree about (1, 2, 3) and a shift <= 0.1, then permuted: the first search matches
    every point to its planted partner, so one Kabsch step lands on the planted inverse and the loop stops at its third search.
    Measured with this restatement: max |T - inverse| = 2.3e-15 (0.5 degrees) and 2.4e-15 (1 degree); asserted at 100 x 2.4e-15."""
    origin, processed, planted, perm = ref.planted_pair(degrees)
    trace = []
    got = ref.icp(origin, processed, trace=trace)
    assert np.array_equal(trace[0], perm)                  # every point found its partner at once
    assert got["iterations"] == 3 and got["converged"] and got["fitness"] == 1.0
    err = np.max(np.abs(got["transformation"] - np.linalg.inv(planted)))
    print("max |T - inverse| =", err)
    assert err <= 2.4e-13
    assert np.max(np.abs(got["points"] - origin[perm])) <= 1e-12


@pytest.mark.parametrize("degrees", [5.0, 10.0])
def test_larger_motions_need_more_iterations_and_still_arrive(degrees):
    """At 5 and 10 degrees the first search mismatches some points: more searches are needed (4 and 8 on these clouds), the end
    is the same."""
    origin, processed, planted, perm = ref.planted_pair(degrees)
    trace = []
    got = ref.icp(origin, processed, trace=trace)
    assert not np.array_equal(trace[0], perm) and np.array_equal(trace[-1], perm)
    assert 3 < got["iterations"] <= 30 and got["converged"]
    assert np.max(np.abs(got["transformation"] - np.linalg.inv(planted))) <= 1e-12


def test_trimming_recovers_a_partial_overlap_that_plain_icp_misses():
    """Rows with x < 6.5 against rows with x > 2.5 moved by 3 degrees: within 0.5 only the overlap takes part (400 of 700 points:
    fitness 0.571) and the motion is recovered; untrimmed, the points without a partner pull the clouds onto each other."""
    origin, processed, planted = ref.partial_pair()
    inverse = np.linalg.inv(planted)
    trimmed = ref.icp(origin, processed, align_distance=0.5)
    assert trimmed["converged"] and trimmed["fitness"] == 400 / 700
    assert np.max(np.abs(trimmed["transformation"] - inverse)) <= 1e-12
    plain = ref.icp(origin, processed)
    assert np.max(np.abs(plain["transformation"] - inverse)) > 1.0


def test_fewer_than_three_inliers_raise():
    origin, processed, _, _ = ref.planted_pair(1.0)
    with pytest.raises(ValueError):
        ref.icp(origin, processed + 100.0, align_distance=0.5)


# ---- options ------------------------------------------------------------------------------------------------------------------
def test_a_rigid_transform_is_accepted_as_3x4_or_4x4():
    m = ref.rigid((1, 2, 3), 20.0, (1.0, -2.0, 0.5))
    assert same(al.check_transform(m), m) and same(al.check_transform(m[:3]), m)
    assert same(al.check_transform(m.tolist()), m)
    assert al.check_transform(None) is None


@pytest.mark.parametrize("bad", ["x", np.eye(3), np.eye(5), np.diag([2.0, 2.0, 2.0, 1.0]), np.diag([1.0, 1.0, -1.0, 1.0]),
                                 np.full((4, 4), np.nan), np.eye(4) + 1e-6, np.vstack([np.eye(3, 4), [0, 0, 0, 2.0]]),
                                 np.vstack([np.eye(3, 4), [1e-3, 0, 0, 1.0]]), [[1, 0, 0, np.inf], [0, 1, 0, 0], [0, 0, 1, 0]]])
def test_a_transform_that_is_not_rigid_raises(bad):
    with pytest.raises(ValueError, match="transform"):
        al.check_transform(bad)


@pytest.mark.parametrize("kw", [dict(align="kabsch"), dict(align=True), dict(align_distance=0.0), dict(align_distance=-1.0),
                                dict(align_distance=float("nan")), dict(align_distance=float("inf")), dict(align_distance="1"),
                                dict(align_iterations=0), dict(align_iterations=1001), dict(align_iterations=2.5),
                                dict(align_iterations=True), dict(align_tolerance=-1e-9), dict(align_tolerance=float("nan")),
                                dict(align_tolerance=float("inf")), dict(align_tolerance="x")])
def test_bad_alignment_settings_raise_before_any_engine_call(kw):
    eng = AlignOracleEngine()
    pts = PointCloud(np.random.default_rng(0).random((10, 3)))
    base = dict(align="icp")
    base.update(kw)
    with pytest.raises(ValueError, match="align"):
        CloudPair(pts, pts, _engine=eng, **base)
    assert eng.calls == [] and eng.pts == [None, None]


def test_sharded_pairs_are_refused_before_any_engine_call():
    eng = AlignOracleEngine()
    pts = PointCloud(np.random.default_rng(0).random((10, 3)))
    for kw in (dict(align="icp"), dict(transform=np.eye(4))):
        with pytest.raises(ValueError, match="group"):
            CloudPair(pts, pts, _engine=eng, group=object(), **kw)
    assert eng.calls == [] and eng.pts == [None, None]


def test_settings_are_normalised():
    t, align, tau2, iterations, tolerance = al.check_align("icp", 0.5, np.int64(7), 0)
    assert t is None and align == "icp" and tau2 == 0.25 and iterations == 7 and tolerance == 0.0
    assert al.check_align(None)[2] == float("inf")
    assert CalculateOptions().align is None and CalculateOptions(align="icp").align == "icp"
    with pytest.raises(ValueError, match="align"):
        CalculateOptions(align="x")


def test_the_rows_follow_every_existing_row_and_are_absent_by_default():
    rich = dict(hausdorff=True, point_to_plane=True, fscore=0.5, chamfer=True, truncate=0.25, dcd=40)
    plain = [m._key() for m in transform_options(CalculateOptions(**rich))]
    with_rows = [m._key() for m in transform_options(CalculateOptions(align="icp", **rich))]
    assert with_rows == plain + [("AlignmentFitness",), ("AlignmentRMSE",)]
    assert [m._key() for m in transform_options(CalculateOptions())] == [m._key() for m in transform_options(CalculateOptions(align=None))]


# ---- CloudPair on the CPU double ----------------------------------------------------------------------------------------------
def test_with_the_options_off_the_engine_sees_todays_calls():
    origin, processed, _, _ = ref.planted_pair(1.0)
    a, b = AlignOracleEngine(), AlignOracleEngine()
    CloudPair(PointCloud(origin), PointCloud(processed), _engine=a)
    CloudPair(PointCloud(origin), PointCloud(processed), _engine=b, transform=None, align=None, align_distance=None,
              align_iterations=30, align_tolerance=1e-6)
    assert a.calls == b.calls == [("nn", nat.DIR_LEFT), ("nn", nat.DIR_RIGHT)]


@pytest.mark.parametrize("degrees", [1.0, 5.0])
def test_a_pair_aligns_like_the_restatement(degrees):
    origin, processed, planted, _ = ref.planted_pair(degrees)
    want = ref.icp(origin, processed)
    eng = AlignOracleEngine()
    pair = CloudPair(PointCloud(origin), PointCloud(processed), _engine=eng, align="icp")
    got = pair.alignment
    assert got.iterations == want["iterations"] and got.converged == want["converged"]
    assert same(got.fitness, want["fitness"]) and same(got.inlier_rmse, want["inlier_rmse"])
    assert same(got.transformation, want["transformation"])
    assert same(eng.get_points(1), want["points"]) and same(eng.get_points(0), origin)
    # the searches of the report come after the last move, both directions
    assert eng.calls[-2:] == [("nn", nat.DIR_LEFT), ("nn", nat.DIR_RIGHT)]
    assert [c for c in eng.calls if c[0] == "nn"][:want["iterations"]] == [("nn", nat.DIR_RIGHT)] * want["iterations"]
    # the report: the rows of a fresh pair on the restatement's final points, then the two alignment rows
    opts = dict(hausdorff=True, fscore=0.1, chamfer=True)
    rows = MetricCalculator(pair).calculate(transform_options(CalculateOptions(align="icp", **opts))).as_dict()
    fresh = CloudPair(PointCloud(origin), PointCloud(want["points"]), _engine=AlignOracleEngine())
    base = MetricCalculator(fresh).calculate(transform_options(CalculateOptions(**opts))).as_dict()
    assert list(rows)[:-2] == list(base) and list(rows)[-2:] == [("AlignmentFitness",), ("AlignmentRMSE",)]
    for key, value in base.items():
        assert same(rows[key], value), key
    assert same(rows[("AlignmentFitness",)], want["fitness"]) and same(rows[("AlignmentRMSE",)], want["inlier_rmse"])


def test_a_transform_moves_the_cloud_and_its_normals_and_starts_icp():
    origin, processed, planted, perm = ref.planted_pair(10.0)
    guess = np.linalg.inv(ref.rigid((1.0, 2.0, 3.0), 9.0, (0.1, -0.05, 0.08)))
    guess = al.check_transform(guess)
    normals = np.random.default_rng(3).normal(size=processed.shape)
    cloud = PointCloud(processed)
    cloud.normals = normals
    eng = AlignOracleEngine()
    pair = CloudPair(PointCloud(origin), cloud, _engine=eng, transform=guess, estimate_normals=False)
    assert pair.alignment.iterations == 0 and pair.alignment.fitness is None and not pair.alignment.converged
    assert same(pair.alignment.transformation, guess)
    assert same(eng.get_points(1), ref.move_points(processed, guess))
    assert same(pair.get_normals(1), ref.move_normals(normals, guess))             # (the engine's, not the file's)
    with pytest.raises(ValueError, match="not aligned"):
        MetricCalculator(pair).calculate(transform_options(CalculateOptions(align="icp")))
    want = ref.icp(origin, processed, start=guess)
    both = CloudPair(PointCloud(origin), PointCloud(processed), _engine=AlignOracleEngine(), transform=guess[:3], align="icp")
    assert both.alignment.iterations == want["iterations"] and same(both.alignment.transformation, want["transformation"])
    assert np.max(np.abs(both.alignment.transformation - np.linalg.inv(planted))) <= 1e-12


def test_trimming_and_the_iteration_limit_reach_the_loop():
    origin, processed, planted = ref.partial_pair()
    want = ref.icp(origin, processed, align_distance=0.5)
    pair = CloudPair(PointCloud(origin), PointCloud(processed), _engine=AlignOracleEngine(), align="icp", align_distance=0.5)
    assert same(pair.alignment.fitness, 400 / 700) and same(pair.alignment.transformation, want["transformation"])
    capped = CloudPair(PointCloud(origin), PointCloud(processed), _engine=AlignOracleEngine(), align="icp", align_distance=0.5,
                       align_iterations=2)
    assert capped.alignment.iterations == 2 and not capped.alignment.converged
    with pytest.raises(ValueError, match="three"):
        CloudPair(PointCloud(origin), PointCloud(processed + 100.0), _engine=AlignOracleEngine(), align="icp", align_distance=0.5)


def test_with_reconst_aligns_every_decoded_cloud_itself():
    origin, first, _, _ = ref.planted_pair(1.0)
    _, second, _, _ = ref.planted_pair(5.0, seed=0, shift=(-0.1, 0.1, 0.0))
    eng = AlignOracleEngine()
    pair = CloudPair(PointCloud(origin), PointCloud(first), _engine=eng, align="icp")
    one = pair.alignment
    nxt = pair.with_reconst(PointCloud(second))
    want1, want2 = ref.icp(origin, first), ref.icp(origin, second)
    assert same(one.transformation, want1["transformation"])
    assert nxt.alignment.iterations == want2["iterations"] and same(nxt.alignment.transformation, want2["transformation"])
    assert same(nxt._engine.get_points(1), want2["points"]) and same(nxt._engine.get_points(0), origin)


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_cli_refuses_bad_values_before_any_file_or_context(tmp_path, monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a GPU context was asked for")
    monkeypatch.setattr(nat, "acquire_engine", no_context)
    monkeypatch.setattr(nat, "Engine", no_context)
    good, bad, short = str(tmp_path / "t.txt"), str(tmp_path / "bad.txt"), str(tmp_path / "short.txt")
    al.write_transform_file(good, ref.rigid((0, 0, 1), 30.0, (1, 2, 3)))
    with open(bad, "w") as f:
        f.write(" ".join(["2"] + ["0"] * 3 + ["0", "1", "0", "0"] + ["0", "0", "1", "0"]))
    with open(short, "w") as f:
        f.write("1 0 0 0 1 0 0 0 1")
    none = ["--ocloud", str(tmp_path / "none_a.ply"), "--pcloud", str(tmp_path / "none_b.ply")]
    for extra in (["--align", "kabsch"], ["--align", "icp", "--align-distance", "0"], ["--align", "icp", "--align-distance", "nan"],
                  ["--align", "icp", "--align-iterations", "0"], ["--align", "icp", "--align-iterations", "1001"],
                  ["--align", "icp", "--align-tolerance", "-1"], ["--align-distance", "0.5"], ["--align-out", str(tmp_path / "o.txt")],
                  ["--transform", bad], ["--transform", short], ["--transform", str(tmp_path / "missing.txt")]):
        out = CliRunner().invoke(cli, none + extra)
        assert out.exit_code == 2, (extra, out.output, out.exception)
    out = CliRunner().invoke(cli, ["--help"])
    for name in ("--align", "--align-distance", "--align-iterations", "--align-tolerance", "--transform", "--align-out"):
        assert name in out.output


def test_transform_files_round_trip_every_bit(tmp_path):
    m = ref.rigid((1, 2, 3), 12.3456789, (0.1, 1e-9, -3e7))
    path = str(tmp_path / "t.txt")
    al.write_transform_file(path, m)
    assert same(al.read_transform_file(path), m)
    with open(path, "w") as f:
        f.write("\n".join(" ".join(repr(float(v)) for v in row) for row in m[:3]))
    assert same(al.read_transform_file(path), m)


# ---- points_moved -------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
def test_a_moved_cloud_leaves_each_product_as_the_table_says(tmp_path):
    exe = str(tmp_path / "align_stale_host")
    build = subprocess.run(
        [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "open_pcc_metric_amd", "csrc"),
         os.path.join(ROOT, "tests", "align_stale_host_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert " checks, 0 failed" in run.stdout
