"""Host-side contract of the colour and joint point-to-distribution rows (CalculateOptions(point_to_distribution=True,
p2d_color=True)): option validation, row order, labels and keys, reports without the option untouched, the command line flag, the
checks that run before any GPU context exists, the C constants, and the NumPy restatement itself on the flat and degenerate cases
it is there for.  No GPU needed."""
import itertools
import os
import re
import sys

import numpy as np
import pytest
from click.testing import CliRunner

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import CalculateResult, MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair, DeviceColumn
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import write_point_cloud
from open_pcc_metric_amd.metric import (ColorMahalanobisDistance, ColorMahalanobisDistances, JointMahalanobisDistance,
                                        JointMahalanobisDistances, MahalanobisDistances, MaxColorMahalanobisDistance,
                                        MaxJointMahalanobisDistance, SymmetricMetric)
from open_pcc_metric_amd.options import CalculateOptions, check_p2d_color, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import p2d_color_reference as cref  # noqa: E402
import p2d_reference as ref  # noqa: E402

COLOR, JOINT = "ColorMahalanobisDistance", "JointMahalanobisDistance"
MAXCOLOR, MAXJOINT = "MaxColorMahalanobisDistance", "MaxJointMahalanobisDistance"


def keys(opts):
    return [m._key() for m in transform_options(opts)]


def no_context(*a, **k):
    raise AssertionError("a GPU context was asked for")


# ---- options -------------------------------------------------------------------------------------------------------------------
def test_defaults_and_the_option_needs_the_geometry_rows():
    assert CalculateOptions().p2d_color is False
    assert CalculateOptions(point_to_distribution=True).p2d_color is False
    assert CalculateOptions(point_to_distribution=True, p2d_color=True).p2d_color is True
    with pytest.raises(ValueError, match="point_to_distribution"):
        CalculateOptions(p2d_color=True)
    with pytest.raises(ValueError, match="point_to_distribution"):
        CalculateOptions(point_to_distribution=False, p2d_color=True, p2d_neighbours=12)


@pytest.mark.parametrize("color, hd, p2plane, plane", itertools.product([None, "ycc"], [False, True], [False, True], [False, True]))
@pytest.mark.parametrize("ranks", [None, (0.5, 0.95)])
@pytest.mark.parametrize("ssim", [(), ("color", "curvature", "normal", "geometry")])
def test_rows_follow_every_existing_row(color, hd, p2plane, plane, ranks, ssim):
    kw = dict(color=color, hausdorff=hd, point_to_plane=p2plane, plane_to_plane=plane, hausdorff_rank=ranks, point_ssim=ssim,
              point_to_distribution=True, p2d_neighbours=9)
    base = keys(CalculateOptions(**kw))                           # MaxMahalanobisDistance rows included
    assert keys(CalculateOptions(p2d_color=False, **kw)) == base
    opts = CalculateOptions(p2d_color=True, **kw)
    got = keys(opts)
    assert got[:len(base)] == base                               # no existing row moves
    new = []
    for cls in (COLOR, JOINT, MAXCOLOR, MAXJOINT) if hd else (COLOR, JOINT):
        new += [(cls, True, 9), (cls, False, 9), ("SymmetricMetric", cls, True, 9, cls, False, 9)]
    assert got[len(base):] == new
    metrics = transform_options(opts)[len(base):]
    for m in metrics:
        m.value = 0.5
    want = []
    for cls in (COLOR, JOINT, MAXCOLOR, MAXJOINT) if hd else (COLOR, JOINT):
        want += [cls, cls, cls + "(symmetric)"]
    assert list(CalculateResult(metrics).as_df()["label"]) == want
    sym = [m for m in metrics if isinstance(m, SymmetricMetric)]
    assert len(sym) == (4 if hd else 2)
    assert not any(m.is_proportional for m in sym)               # lower is better: the larger side


def test_without_the_option_the_rows_are_todays():
    """Every option set without p2d_color gives the list it gave before the option existed: nothing in it names the new rows, and
    the p2d_color rows are a pure suffix (test_rows_follow_every_existing_row)."""
    for color, hd, p2plane, p2d in itertools.product([None, "ycc"], [False, True], [False, True], [False, True]):
        got = keys(CalculateOptions(color, hd, p2plane, point_to_distribution=p2d))
        assert not any("ColorMahalanobis" in str(k) or "JointMahalanobis" in str(k) for k in got)
        n_p2d = (6 if hd else 3) if p2d else 0
        assert sum("Mahalanobis" in str(k) for k in got) == n_p2d
        if n_p2d:
            assert all("Mahalanobis" in str(k) for k in got[-n_p2d:])


def test_dependencies_keys_and_prefetch_items():
    for cls, primary in ((ColorMahalanobisDistance, ColorMahalanobisDistances), (MaxColorMahalanobisDistance, ColorMahalanobisDistances),
                         (JointMahalanobisDistance, JointMahalanobisDistances), (MaxJointMahalanobisDistance, JointMahalanobisDistances)):
        m = cls(is_left=False, k=7)
        dep = m._get_dependencies()["mahalanobis_distances"]
        assert type(dep) is primary and (dep.is_left, dep.k) == (False, 7)
        assert cls(True)._key() == (cls.__name__, True, 30)
    # the three primaries are three memo entries
    assert len({c(True, 30)._key() for c in (MahalanobisDistances, ColorMahalanobisDistances, JointMahalanobisDistances)}) == 3
    assert DeviceColumn._METRIC["p2d_color"] == nat.METRIC_P2D_COLOR and DeviceColumn._METRIC["p2d_joint"] == nat.METRIC_P2D_JOINT

    class Recorder:                                               # what MetricCalculator hands to prefetch_reductions
        wanted = None

        def prefetch_reductions(self, wanted):
            self.wanted = list(wanted)
            raise KeyboardInterrupt                               # (nothing is evaluated in this test)

    pair = Recorder()
    opts = CalculateOptions(hausdorff=True, point_to_distribution=True, p2d_neighbours=11, p2d_color=True)
    with pytest.raises(KeyboardInterrupt):
        MetricCalculator(pair).calculate(transform_options(opts))
    for kind in ("p2d", "p2d_color", "p2d_joint"):
        assert (kind, True, 11) in pair.wanted and (kind, False, 11) in pair.wanted


# ---- the checks before any GPU work ----------------------------------------------------------------------------------------------
def cloud(n=20, seed=0, colors=True):
    rng = np.random.default_rng(seed)
    return PointCloud(rng.random((n, 3)), colors=rng.random((n, 3)) if colors else None)


def test_check_p2d_color(monkeypatch):
    monkeypatch.setattr(nat, "acquire_engine", no_context)
    monkeypatch.setattr(nat, "Engine", no_context)
    opts = CalculateOptions(point_to_distribution=True, p2d_color=True)
    check_p2d_color(opts, cloud(), cloud(seed=1))
    check_p2d_color(CalculateOptions(point_to_distribution=True), cloud(colors=False), cloud(colors=False), group=object())   # no such rows
    for a, b in ((cloud(colors=False), cloud()), (cloud(), cloud(colors=False)), (cloud(colors=False), cloud(colors=False))):
        with pytest.raises(ValueError, match="colours"):
            check_p2d_color(opts, a, b)
    with pytest.raises(ValueError, match="sharded"):
        check_p2d_color(opts, cloud(), cloud(seed=1), group=object())


def test_a_pair_checks_the_same_before_any_engine_call():
    """CloudPair's own check, on a pair that has no engine at all: any GPU work would raise AttributeError instead."""
    for clouds, sharded, match in (((cloud(colors=False), cloud()), False, "colours"), ((cloud(), cloud(seed=1)), True, "sharded")):
        pair = object.__new__(CloudPair)
        pair.clouds = clouds

        class Coll:
            group = object()
        Coll.sharded = sharded
        pair._coll = Coll()
        with pytest.raises(ValueError, match=match):
            pair.get_left_color_mahalanobis_distances()
        with pytest.raises(ValueError, match=match):
            pair.get_right_joint_mahalanobis_distances(12)
        with pytest.raises(ValueError, match=match):
            pair._check_p2d(30, True)


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_help_lists_the_flag():
    out = CliRunner().invoke(cli, ["--help"])
    assert out.exit_code == 0 and "--p2d-color" in out.output


def test_usage_errors_come_before_any_file_or_context(tmp_path, monkeypatch):
    monkeypatch.setattr(nat, "acquire_engine", no_context)
    monkeypatch.setattr(nat, "Engine", no_context)
    missing = str(tmp_path / "does_not_exist.ply")
    out = CliRunner().invoke(cli, ["--ocloud", missing, "--pcloud", missing, "--p2d-color"])
    assert out.exit_code == 2 and "point_to_distribution" in out.output      # without --point-to-distribution: a usage error
    out = CliRunner().invoke(cli, ["--ocloud", missing, "--pcloud", missing, "--p2d-color", "--hausdorff", "--p2d-neighbours", "8"])
    assert out.exit_code == 2
    pa, pb, pc = (str(tmp_path / f"{name}.ply") for name in "abc")
    write_point_cloud(pa, cloud())
    write_point_cloud(pb, cloud(seed=1))
    write_point_cloud(pc, cloud(seed=2, colors=False))
    out = CliRunner().invoke(cli, ["--ocloud", pa, "--pcloud", pc, "--point-to-distribution", "--p2d-color"])
    assert isinstance(out.exception, ValueError) and "colours" in str(out.exception)     # refused before the context
    out = CliRunner().invoke(cli, ["--ocloud", pa, "--pcloud", pb, "--point-to-distribution", "--p2d-color"])
    assert isinstance(out.exception, AssertionError)             # good flags and coloured clouds get as far as the context


def test_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "pccm.h")).read()
    assert re.search(rf"#define PCCM_METRIC_P2D_COLOR {nat.METRIC_P2D_COLOR}\b", header) and nat.METRIC_P2D_COLOR == 9
    assert re.search(rf"#define PCCM_METRIC_P2D_JOINT {nat.METRIC_P2D_JOINT}\b", header) and nat.METRIC_P2D_JOINT == 10
    assert re.search(rf"#define PCCM_P2D_GEOMETRY {nat.P2D_GEOMETRY}\b", header) and nat.P2D_GEOMETRY == 1
    assert re.search(rf"#define PCCM_P2D_COLOR {nat.P2D_COLOR}\b", header) and nat.P2D_COLOR == 2
    assert re.search(r"int pccm_p2d_build_attrs\(pccm_ctx \*ctx, int k, int attrs, int \*built\);", header)
    assert re.search(r"int pccm_p2d_build\(pccm_ctx \*ctx, int k, int \*built\);", header)       # the old call keeps its signature
    assert "pccm_p2d_build_attrs" in nat.SYMBOLS and "pccm_p2d_build" in nat.SYMBOLS
    lib = nat.load()
    assert hasattr(lib, "pccm_p2d_build_attrs")


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def parts(name, k, left=True):
    a, b, ca, cb = cref.FAMILIES[name]()
    if not left:
        a, b, ca, cb = b, a, cb, ca
    nbr = ref.knn_rows(a, b, k)
    my, m, raw = cref.color_mahalanobis(ca, cb, nbr, return_parts=True)
    return a, b, ca, cb, nbr, my, m, raw


def test_flat_neighbourhoods_round_below_zero_and_the_clamp_takes_them():
    """The reason for the clamp: where every neighbour has the same luma, V = S2 / kk - m * m is 0 up to rounding, on either
    side.  There M_Y is exactly |m| * 2^10 (v = 2^-20, its root 2^-10: a power of two), and |m| is the luma difference."""
    seen_negative = seen_zero = 0
    for name, k in (("surface_bytes", 30), ("surface_bytes", 64), ("constant_offset", 4), ("constant_offset", 30)):
        a, b, ca, cb, nbr, my, m, raw = parts(name, k)
        yb = cref.luma(cb)[nbr]
        flat = np.all(yb == yb[:, :1], axis=1)
        assert flat.sum() > len(a) // 3
        assert np.all(np.abs(raw[flat]) < 1e-15)
        seen_negative += int(np.sum(raw[flat] < 0))
        seen_zero += int(np.sum(raw[flat] == 0))
        clamped = raw <= 0
        assert np.all(flat[clamped])
        assert np.array_equal(my[clamped], np.abs(m[clamped]) * 2.0 ** 10)
        dy = np.abs(yb[:, 0] - cref.luma(ca))
        assert np.allclose(np.abs(m[flat]), dy[flat], rtol=1e-14, atol=0)
        assert np.all(my[flat & (dy > 0)] > 0)
    assert seen_negative > 100 and seen_zero > 100
    a, b, ca, cb, nbr, my, m, raw = parts("surface_bytes", 30)
    assert np.sum(raw < 0) > 100 and np.sum(raw == 0) > 50      # one family, one k: both signs of the rounding


@pytest.mark.parametrize("name", sorted(cref.FAMILIES))
def test_colour_values_are_finite_everywhere(name):
    for k in (4, 30):
        for left in (True, False):
            my = parts(name, k, left)[5]
            assert np.all(np.isfinite(my)) and np.all(my >= 0)


def test_joint_value():
    a, b, ca, cb = cref.FAMILIES["inf_geometry"]()
    mg, my, mj = cref.columns(a, b, ca, cb, 30)
    assert np.sum(np.isinf(mg)) >= 30 and np.sum(mg == 0) >= 1
    assert np.array_equal(np.isinf(mj), np.isinf(mg)) and not np.any(np.isnan(mj))
    assert np.all(mj[np.isfinite(mg)] >= np.maximum(mg, my)[np.isfinite(mg)])
    # both clouds of one identical constant colour: M_Y = 0 and the joint value IS the geometry value
    a, b = ref.uniform(1200, 51), ref.uniform(1000, 52)
    grey = (0.3, 0.6, 0.9)
    mg, my, mj = cref.columns(a, b, cref.constant_colors(len(a), grey), cref.constant_colors(len(b), grey), 30)
    assert np.all(my == 0.0) and np.array_equal(mj.view(np.uint64), mg.view(np.uint64))


def test_the_order_of_the_searched_cloud_does_not_matter_without_ties():
    a, b, ca, cb = cref.FAMILIES["surface_smooth"]()
    d2 = np.sort(ref.sq_dist(a[:, None, :], b[None, :, :]), axis=1)[:, :31]
    assert np.all(d2[:, 1:] > d2[:, :-1])                         # tie-free: the neighbourhood order is the distance order
    want = cref.columns(a, b, ca, cb, 30)
    perm = np.random.default_rng(7).permutation(len(b))
    got = cref.columns(a, b[perm], ca, cb[perm], 30)
    for w, g in zip(want, got):
        assert np.array_equal(w.view(np.uint64), g.view(np.uint64))


def test_luma_of_bytes_is_the_luma_of_their_quotients():
    """What lets the device gather packed bytes: k / 255.0 formed again from the byte is the double the colour array holds."""
    colors, u8 = cref.random_byte_colors(500, 3)
    assert np.array_equal(cref.to_bytes(colors), u8)
    assert np.array_equal(cref.luma(colors).view(np.uint64), cref.luma(u8.astype(np.float64) / 255.0).view(np.uint64))
