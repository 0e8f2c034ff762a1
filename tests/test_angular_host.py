"""Host-side contract of the plane-to-plane rows (CalculateOptions(plane_to_plane=True)): row order and keys, the default report
untouched, the command line flag, the C constant, and the NumPy restatement's fixed points.  No GPU needed."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.metric import AngularSimilarities, AngularSimilarity, MinAngularSimilarity, SymmetricMetric
from open_pcc_metric_amd.options import CalculateOptions, transform_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from angular_reference import angular_similarity, angular_tie_mean  # noqa: E402


def keys(opts):
    return [m._key() for m in transform_options(opts)]


@pytest.mark.parametrize("color", [None, "ycc"])
@pytest.mark.parametrize("p2plane", [False, True])
@pytest.mark.parametrize("hd", [False, True])
def test_rows_follow_every_existing_row(color, p2plane, hd):
    base = keys(CalculateOptions(color, hd, p2plane))
    got = keys(CalculateOptions(color, hd, p2plane, plane_to_plane=True))
    assert got[:len(base)] == base
    new = [("AngularSimilarity", True), ("AngularSimilarity", False),
           ("SymmetricMetric", "AngularSimilarity", True, "AngularSimilarity", False)]
    if hd:
        new += [("MinAngularSimilarity", True), ("MinAngularSimilarity", False),
                ("SymmetricMetric", "MinAngularSimilarity", True, "MinAngularSimilarity", False)]
    assert got[len(base):] == new


def test_without_the_option_the_rows_are_todays():
    assert CalculateOptions("ycc", True, True).plane_to_plane is False
    for args in [(), ("ycc",), ("rgb", True), (None, True, True), ("ycc", True, True)]:
        assert keys(CalculateOptions(*args)) == keys(CalculateOptions(*args, plane_to_plane=False))
        assert not any("Angular" in str(k) for k in keys(CalculateOptions(*args)))
    assert len(keys(CalculateOptions("ycc", True, True))) == 32


def test_symmetric_rows_are_higher_is_better():
    for m in transform_options(CalculateOptions(None, True, False, plane_to_plane=True)):
        if isinstance(m, SymmetricMetric) and isinstance(m.metrics[0], (AngularSimilarity, MinAngularSimilarity)):
            assert m.is_proportional


class _Pair:
    """A stand-in CloudPair whose angular columns are plain ndarrays: the metric nodes then run through NumPy itself."""

    def __init__(self, left, right):
        self.cols = {True: np.asarray(left, dtype=np.float64), False: np.asarray(right, dtype=np.float64)}
        self.wanted = None

    def get_left_angular_similarities(self):
        return self.cols[True]

    def get_right_angular_similarities(self):
        return self.cols[False]

    def prefetch_reductions(self, wanted):
        self.wanted = list(wanted)


def test_report_values_from_plain_columns():
    rng = np.random.default_rng(5)
    left, right = rng.random(1000), rng.random(700)
    pair = _Pair(left, right)
    metrics = [m for m in transform_options(CalculateOptions(None, True, False, plane_to_plane=True))
               if "Angular" in str(m._key())]
    res = MetricCalculator(pair).calculate(metrics).as_dict()
    assert sorted(pair.wanted, key=str) == [("angular", False), ("angular", True)]
    assert res[("AngularSimilarity", True)] == np.sum(left) / 1000
    assert res[("AngularSimilarity", False)] == np.sum(right) / 700
    assert res[("MinAngularSimilarity", True)] == np.min(left)
    sym = res[("SymmetricMetric", "AngularSimilarity", True, "AngularSimilarity", False)]
    assert sym == min(np.sum(left) / 1000, np.sum(right) / 700)
    assert res[("SymmetricMetric", "MinAngularSimilarity", True, "MinAngularSimilarity", False)] == min(np.min(left), np.min(right))
    node = AngularSimilarities(is_left=True)
    node.calculate(pair)
    assert node.value is pair.cols[True]


def test_cli_help_lists_the_flag():
    env = dict(os.environ, PYTHONPATH=ROOT)
    for pkg in ("open_pcc_metric_amd", "open_pcc_metric"):
        out = subprocess.run([sys.executable, "-m", pkg, "--help"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=120)
        assert out.returncode == 0, out.stderr
        assert "--plane-to-plane" in out.stdout


def test_header_defines_the_metric():
    text = open(os.path.join(ROOT, "include", "pccm.h")).read()
    assert re.search(r"^#define PCCM_METRIC_ANGULAR 3\b", text, re.M)
    from open_pcc_metric_amd import _native as nat
    assert nat.METRIC_ANGULAR == 3


def test_restatement_fixed_points():
    rng = np.random.default_rng(1)
    a = rng.standard_normal((500, 3))
    scale = 2.0 ** rng.integers(-8, 8, (500, 1))                        # (exact: |dot| / den rounds to 1 exactly)
    assert np.all(angular_similarity(a, a) == 1.0)                        # parallel
    assert np.all(angular_similarity(a, a * scale) == 1.0)
    assert np.all(angular_similarity(a, -a * scale) == 1.0)               # antiparallel
    near = angular_similarity(a, a * (rng.random((500, 1)) * 10 + 0.1))   # parallel up to rounding: c may fall short of 1 by ulps
    assert np.all((near <= 1.0) & (near > 1.0 - 1e-7))
    perp = np.cross(a, rng.standard_normal((500, 3)))
    got = angular_similarity(a, perp)
    assert np.max(np.abs(got)) < 1e-15                                    # perpendicular (up to the rounding of the cross product)
    ex = np.array([[1.0, 0, 0], [0, 2.0, 0], [0, 0, -3.0], [1.0, 0, 0]])
    ey = np.array([[0, 5.0, 0], [0, 0, 1.0], [4.0, 0, 0], [0, 0, -1.0]])
    assert angular_similarity(ex, ey).tolist() == [0.0, 0.0, 0.0, 0.0]
    z = np.zeros((3, 3))
    assert angular_similarity(z, a[:3]).tolist() == [0.0] * 3             # zero-length normals count as perpendicular
    assert angular_similarity(a[:3], z).tolist() == [0.0] * 3
    assert angular_similarity(z, z).tolist() == [0.0] * 3


@pytest.mark.parametrize("deg", [0, 30, 45, 60, 90, 120, 135, 150, 180])
def test_restatement_known_angles(deg):
    t = math.radians(deg)
    a = np.array([[1.0, 0.0, 0.0]])
    b = np.array([[math.cos(t), math.sin(t), 0.0]])
    folded = min(deg, 180 - deg)                                          # unoriented normals
    assert abs(angular_similarity(a, b)[0] - (1.0 - folded / 90.0)) < 1e-14


def test_tie_mean_adds_per_neighbour_values_in_row_order():
    own = np.array([[1.0, 0.0, 0.0]])
    other = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert angular_tie_mean(own, other, [np.array([0, 1])]).tolist() == [1.0]            # opposite signs do not cancel
    assert angular_tie_mean(own, other, [np.array([0, 1, 2])]).tolist() == [(1.0 + 1.0 + 0.0) / 3.0]
