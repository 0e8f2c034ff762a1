"""Host-side contract of the PointSSIM rows (CalculateOptions(point_ssim=...)): row order, labels and keys, the default report
untouched, the command line flags, the checks that run before any GPU context exists, the C constants, and the NumPy
restatement's fixed points.  No GPU needed."""
import itertools
import os
import re
import sys

import numpy as np
import pytest
from click.testing import CliRunner

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import CalculateResult
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import write_point_cloud
from open_pcc_metric_amd.metric import (ColorSSIM, CurvatureSSIM, GeometrySSIM, NormalSSIM, SSIMSimilarities, SymmetricMetric)
from open_pcc_metric_amd.options import CalculateOptions, check_point_ssim, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pointssim_reference as ref  # noqa: E402

ATTRS = ("geometry", "normal", "curvature", "color")
CLASS = {"geometry": "GeometrySSIM", "normal": "NormalSSIM", "curvature": "CurvatureSSIM", "color": "ColorSSIM"}


def keys(opts):
    return [m._key() for m in transform_options(opts)]


SUBSETS = [c for r in range(1, 5) for c in itertools.combinations(ATTRS, r)]


@pytest.mark.parametrize("subset", SUBSETS, ids="-".join)
@pytest.mark.parametrize("color, hd, p2plane, plane", [(None, False, False, False), ("ycc", True, True, True),
                                                       ("rgb", False, True, False), (None, True, False, True)])
def test_rows_follow_every_existing_row_in_fixed_order(subset, color, hd, p2plane, plane):
    base = keys(CalculateOptions(color, hd, p2plane, plane_to_plane=plane))
    given = tuple(reversed(subset))                               # the caller's order does not matter
    opts = CalculateOptions(color, hd, p2plane, plane_to_plane=plane, point_ssim=given, ssim_neighbours=9)
    got = keys(opts)
    assert got[:len(base)] == base
    new = []
    for a in ATTRS:
        if a in subset:
            cls = CLASS[a]
            new += [(cls, True, 9), (cls, False, 9), ("SymmetricMetric", cls, True, 9, cls, False, 9)]
    assert got[len(base):] == new
    metrics = transform_options(opts)[len(base):]
    for m in metrics:
        m.value = 0.5
    labels = list(CalculateResult(metrics).as_df()["label"])
    want = []
    for a in ATTRS:
        if a in subset:
            want += [CLASS[a], CLASS[a], CLASS[a] + "(symmetric)"]
    assert labels == want
    sym = [m for m in metrics if isinstance(m, SymmetricMetric)]
    assert all(m.is_proportional for m in sym)                   # higher is better: the smaller side
    assert all(isinstance(m.metrics[0], (GeometrySSIM, NormalSSIM, CurvatureSSIM, ColorSSIM)) for m in sym)


def test_dependencies_and_keys():
    m = GeometrySSIM(is_left=False, k=7)
    dep = m._get_dependencies()["ssim_similarities"]
    assert isinstance(dep, SSIMSimilarities)
    assert (dep.attribute, dep.is_left, dep.k) == ("geometry", False, 7)
    assert ColorSSIM(True)._key() == ("ColorSSIM", True, 12)
    assert {SSIMSimilarities(True, a)._key() for a in ATTRS}.__len__() == 4


def test_without_the_option_the_rows_are_todays():
    for color, hd, p2plane in itertools.product([None, "ycc"], [False, True], [False, True]):
        base = keys(CalculateOptions(color, hd, p2plane))
        assert keys(CalculateOptions(color, hd, p2plane, point_ssim=None)) == base
        assert keys(CalculateOptions(color, hd, p2plane, point_ssim=())) == base
        assert not any("SSIM" in str(k) for k in base)


@pytest.mark.parametrize("kw", [dict(point_ssim=["texture"]), dict(point_ssim=["geometry"], ssim_neighbours=1),
                                dict(point_ssim=["geometry"], ssim_neighbours=65), dict(point_ssim=["geometry"], ssim_neighbours=2.5)])
def test_bad_options_raise(kw):
    with pytest.raises(ValueError):
        CalculateOptions(**kw)


def test_help_lists_both_flags():
    out = CliRunner().invoke(cli, ["--help"])
    assert out.exit_code == 0
    assert "--point-ssim" in out.output and "--ssim-neighbours" in out.output
    for a in ATTRS:
        assert a in out.output


def cloud(n=20, seed=0, normals=True, colors=True):
    rng = np.random.default_rng(seed)
    return PointCloud(rng.random((n, 3)), rng.standard_normal((n, 3)) if normals else None,
                      rng.random((n, 3)) if colors else None)


def test_checks_raise_before_any_context(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a GPU context was asked for")
    monkeypatch.setattr(nat, "acquire_engine", no_context)
    monkeypatch.setattr(nat, "Engine", no_context)
    full, bare = cloud(), cloud(normals=False, colors=False)
    ok = CalculateOptions(point_ssim=["geometry", "normal", "curvature", "color"])
    check_point_ssim(ok, full, full)                              # nothing missing
    check_point_ssim(CalculateOptions(), bare, bare, ties="mean", group=object())   # no PointSSIM rows: nothing to check
    cases = [
        (CalculateOptions(point_ssim=["color"]), full, bare, {}),
        (CalculateOptions(point_ssim=["color"]), bare, full, {}),
        (CalculateOptions(point_ssim=["normal"]), bare, full, dict(estimate_normals=False)),
        (CalculateOptions(point_ssim=["geometry"]), full, full, dict(ties="mean")),
        (CalculateOptions(point_ssim=["geometry"]), full, full, dict(group=object())),
    ]
    for opts, a, b, kw in cases:
        with pytest.raises(ValueError):
            check_point_ssim(opts, a, b, **kw)
    check_point_ssim(CalculateOptions(point_ssim=["normal"]), bare, bare)            # estimated, as plane-to-plane does


def test_cli_checks_before_any_context(tmp_path, monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a GPU context was asked for")
    monkeypatch.setattr(nat, "acquire_engine", no_context)
    monkeypatch.setattr(nat, "Engine", no_context)
    pa, pb = str(tmp_path / "a.xyz"), str(tmp_path / "b.xyz")
    write_point_cloud(pa, cloud(normals=False, colors=False))
    write_point_cloud(pb, cloud(seed=1, normals=False, colors=False))
    for extra in (["--point-ssim", "color"], ["--point-ssim", "geometry", "--ties", "mean"]):
        out = CliRunner().invoke(cli, ["--ocloud", pa, "--pcloud", pb] + extra)
        assert out.exit_code != 0
        assert isinstance(out.exception, ValueError), out.exception
    for extra in (["--point-ssim", "texture"], ["--point-ssim", "geometry", "--ssim-neighbours", "65"]):
        out = CliRunner().invoke(cli, ["--ocloud", pa, "--pcloud", pb] + extra)
        assert out.exit_code == 2                                 # click rejects the value itself


def test_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "pccm.h")).read()
    for name, value in nat.METRIC_SSIM.items():
        assert re.search(rf"#define PCCM_METRIC_SSIM_{name.upper()} {value}\b", header)
    for name, value in nat.SSIM_ATTRS.items():
        assert re.search(rf"#define PCCM_SSIM_{name.upper()} {value}\b", header)
    assert "pccm_ssim_features" in nat.SYMBOLS and "pccm_get_ssim_features" in nat.SYMBOLS


# ---- the restatement's fixed points, on a hand-worked 5-point cloud ------------------------------------------------------
FIVE = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 3.0], [1.0, 0.0, 0.0]])


def test_five_point_neighbourhoods():
    nbr = ref.knn_rows(FIVE, 3)
    # point 0: itself, then rows 1 and 4 at d2 = 1 (tie: the smaller row first)
    assert nbr[0].tolist() == [0, 1, 4]
    # rows 1 and 4 coincide: each has the other at distance 0 behind itself (q_0 = p), the tie going to the smaller row
    assert nbr[1].tolist() == [1, 4, 0] and nbr[4].tolist() == [1, 4, 0]
    assert ref.knn_rows(FIVE, 64).shape == (5, 5)                 # n < k: the whole cloud


def test_five_point_features_by_hand():
    g = ref.features(FIVE, 3, "geometry")
    # point 0: distances 1, 1 -> variance 0; point 2: neighbours 0 (d 2) and 1 (d sqrt 5) -> ((2 - s5)^2 / 2) / 1
    assert g[0] == 0.0
    d = np.array([2.0, np.sqrt(5.0)])
    mu = (d[0] + d[1]) / 2.0
    assert g[2] == ((d[0] - mu) * (d[0] - mu) + (d[1] - mu) * (d[1] - mu)) / 1.0
    # m < 2: k = 2 leaves one geometry value per point -> 0
    assert np.all(ref.features(FIVE, 2, "geometry") == 0.0)
    # n < k: all five points, m = 4 other distances
    allg = ref.features(FIVE, 64, "geometry")
    v = np.sqrt(ref.sq_dist(FIVE[0], FIVE[[1, 4, 2, 3]]))
    mu = np.cumsum(v)[-1] / 4.0
    assert allg[0] == np.cumsum((v - mu) * (v - mu))[-1] / 3.0
    # colour counts q_0: m = k values; identical colours -> 0
    assert np.all(ref.features(FIVE, 3, "color", colors=np.full((5, 3), 0.5)) == 0.0)
    # curvature: collinear neighbourhoods have lambda_min = 0
    c = ref.curvatures(FIVE, ref.knn_rows(FIVE, 3))
    assert abs(c[0]) < 1e-15


def test_identical_clouds_give_exactly_one():
    rng = np.random.default_rng(3)
    x, col = rng.random((200, 3)), rng.random((200, 3))
    nrm = rng.standard_normal((200, 3))
    for attribute in ATTRS:
        f = ref.features(x, 12, attribute, normals=nrm, colors=col)
        s = ref.similarity_rows(f, f, ref.matched_rows(x, x))
        assert np.all(s == 1.0), attribute
    assert ref.similarity(np.array([0.0]), np.array([0.0]))[0] == 1.0        # zero features: the 2^-52 keeps it defined
    assert ref.similarity(np.array([2.0]), np.array([1.0]))[0] == 1.0 - 1.0 / (2.0 + 2.0 ** -52)
