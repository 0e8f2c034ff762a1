"""The yardstick of tests/test_gpu_extent_kernels.py, checked without a GPU (tests/extent_reference.py).

On every input the GPU tests use, the oracle's fp64 NumPy restatements (tests/oracle_engine.py: obb_frames, extreme_rows,
rows_outside) must satisfy the very assertions the kernels are held to -- so the derived tolerances tau_frame and tau_k are
checked against the references, never against a kernel -- and the largest ratios of error to tolerance are printed.  Then every
defect the models of extent_reference can switch on must FAIL those assertions on at least one named case:

  obb      tile_last_vertex   frames nv = 1024, 1025, 2049 (vertex 1023 / 2047 is the unique end of an axis)
           partial_tile       frames nv = 4, 1023 (no vertex at all: the call raises), 1025, 2049 (vertex nv - 1)
           frame_index        frames nt = 1000 at t = 256 (the examined triangle is never read: the call raises); ties in the second workgroup
           not_normalised     every frame (edges of length != 1); ties
           argmin_last        ties, every order
           degenerate_zero    every isolated batch with nt > 1; ties behind a degenerate triangle
  extreme  last_slice         planted n = 5000, 257, 63: the spike at row n - 1
           dirs_from_64       planted ndirs = 65, 1006, 1024 (a planted direction >= 64 whose row is not 0)
           no_sign_fix        the cloud on the negative side (bound); planted spikes with negative coordinates' dot products
  outside  first_tile_only    nplanes = 513, 2000: row 'outside_512' / 'outside_last'
           last_plane         every nplanes: row 'outside_last'
           rows_past_n        every n that is no multiple of 256 (the origin is outside)
           greater_equal      row 'margin_inside_0' (margin > 0), rows 'on_0', 'on_last' (margin = 0)
           margin_sign        margin > 0: rows 'on_0', 'on_last'
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import extent_reference as er  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402


def fails(fn):
    try:
        fn()
    except (AssertionError, ValueError):
        return True
    return False


# ---- the reference against itself -------------------------------------------------------------------------------
def test_the_cases_are_the_issue_s():
    assert er.FRAME_NT == (1, 256, 257, 1000) and er.FRAME_NV == (4, 1023, 1024, 1025, 2049)
    assert er.frame_positions(1000) == [0, 63, 64, 255, 256, 257, 999] and er.frame_positions(256) == [0, 63, 64, 255]
    assert er.special_vertices(2049) == [0, 1023, 1024, 2047, 2048] and er.special_vertices(4) == [0, 3]
    assert er.EXTREME_N == (1, 63, 257, 5000, 262145) and er.EXTREME_NDIRS == (1, 63, 64, 65, 1006, 1024)
    assert er.slice_len(5000) == 63 and er.slice_len(262145) == 65
    assert {n for n, _ in er.extreme_cases()} == set(er.EXTREME_N) and {k for _, k in er.extreme_cases()} == set(er.EXTREME_NDIRS)
    assert er.OUTSIDE_N == (1, 255, 256, 257, 100003) and er.OUTSIDE_NPLANES == (1, 4, 511, 512, 513, 2000)
    assert {n for n, _ in er.outside_cases()} == set(er.OUTSIDE_N) and {k for _, k in er.outside_cases()} == set(er.OUTSIDE_NPLANES)
    assert er.EPS == 2.0 ** -53 and len(er.directions(1006)) == 1006 and len(er.directions(1024)) == 1024


def test_the_integer_path_is_the_fraction_path():
    """hull_reference (scaled integers, screened exact evaluation) gives frame_reference's value to 45 digits, frame by frame."""
    verts, tri = er.hull_case("blob")
    href = er.hull_reference(verts, tri[:12])
    for t in range(12):
        ref = er.frame_reference(tri[t], verts, keep_projections=False)
        assert all(abs(x - y) <= abs(y) * er._D("1e-45") for x, y in zip(href[t][0].ext, ref.ext))       # (50 digits, other roundings)
        assert abs(href[t][0].vol - ref.vol) <= ref.vol * er._D("1e-45") and href[t][0].sin == ref.sin
    assert er.frame_reference(er.degenerate_triangle(0), verts).ext is None
    assert er.frame_reference(er.degenerate_triangle(1), verts).ext is None
    assert er.hull_reference(verts, np.stack([er.degenerate_triangle(0), er.degenerate_triangle(1)])) == [None, None]


def test_a_known_box():
    """A 3-4-5 triangle in the plane z = 0 over the corners of a box: digits one can check by hand."""
    tri = [[0, 0, 0], [3, 0, 0], [0, 4, 0]]
    verts = [[0, 0, 0], [3, 0, 0], [0, 4, 0], [3, 4, 0.5], [1, 1, -0.25]]
    ref = er.frame_reference(tri, verts)
    assert [float(e) for e in ref.ext] == [3.0, 4.0, 0.75] and float(ref.vol) == 9.0 and ref.sin == 1.0
    assert np.allclose(er.tau_frame(tri, verts), 2 * np.sqrt(25.25) * 2.0 ** -53 * np.array([11.0, 18.0, 14.0]), rtol=1e-15)


# ---- k_obb_frames ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", er.FRAME_NV)
def test_frames_oracle_and_model_within_tau_frame(nv):
    tri, verts, ref, tau = er.frame_case(nv)
    worst = 0.0
    for nt in (1, 257):
        for t in er.frame_positions(nt):
            batch = er.isolated_batch(tri, nt, t)
            for name, fn in (("oracle", OracleEngine().obb_frames), ("model", er.model_obb_frames)):
                ext, vol = fn(verts, batch)
                worst = max(worst, er.check_frame(ext, vol, ref, tau, f"{name} nv={nv} nt={nt} t={t}"))
    print(f"obb frames nv={nv}: sin {ref.sin:.3f}, largest |ext - ext_ref| / tau_frame of the fp64 restatements {worst:.3f}")


@pytest.mark.parametrize("defect,nv,nt,t", [
    ("tile_last_vertex", 1024, 1, 0), ("tile_last_vertex", 1025, 257, 256), ("tile_last_vertex", 2049, 1, 0),
    ("partial_tile", 4, 1, 0), ("partial_tile", 1023, 256, 255), ("partial_tile", 1025, 1, 0), ("partial_tile", 2049, 257, 64),
    ("frame_index", 4, 1000, 256), ("frame_index", 1025, 1000, 256),
    ("not_normalised", 4, 1, 0), ("not_normalised", 2049, 1000, 999),
    ("degenerate_zero", 4, 256, 255), ("degenerate_zero", 1023, 257, 0), ("degenerate_zero", 1024, 1000, 63),
])
def test_frame_defects_are_caught(defect, nv, nt, t):
    tri, verts, ref, tau = er.frame_case(nv)
    batch = er.isolated_batch(tri, nt, t)
    er.check_frame(*er.model_obb_frames(verts, batch), ref, tau)
    assert fails(lambda: er.check_frame(*er.model_obb_frames(verts, batch, defect), ref, tau))


def test_ties_are_exact_and_the_first_wins():
    corners, tris = er.tie_box()
    assert sorted(tuple(e) for _, e in tris) == sorted({(a, b, c) for a in er.BOX_SIDES for b in er.BOX_SIDES for c in er.BOX_SIDES
                                                         if len({a, b, c}) == 3})
    for tri, want in tris:                       # the reference agrees, with a zero error: the frames are exact
        ref = er.frame_reference(tri, corners)
        assert [float(e) for e in ref.ext] == list(want) and float(ref.vol) == 1.25 and ref.sin == 1.0
    for name, batch, want in er.tie_batches():
        er.check_tie(OracleEngine().obb_frames(corners, batch), want)
        er.check_tie(er.model_obb_frames(corners, batch), want)
        caught = {d for d in er.DEFECTS["obb"] if fails(lambda: er.check_tie(er.model_obb_frames(corners, batch, d), want))}
        print("ties", name, sorted(caught))
        assert "argmin_last" in caught and "not_normalised" in caught
        if name in ("degenerate_first", "two_workgroups", "second_workgroup"):
            assert "degenerate_zero" in caught
        if name == "second_workgroup":
            assert "frame_index" in caught


@pytest.mark.parametrize("kind", er.HULLS)
def test_whole_hulls_oracle_and_model(kind):
    verts, tri = er.hull_case(kind)
    href = er.hull_case_reference(kind)
    ratio = {name: er.check_hull(*fn(verts, tri), href, f"{name} {kind}")
             for name, fn in (("oracle", OracleEngine().obb_frames), ("model", er.model_obb_frames))}
    print(f"hull {kind}: nv {len(verts)}, nt {len(tri)}, smallest sin {min(f[0].sin for f in href if f):.2e}, ratios {ratio}")
    # (a dropped tile or vertex need not move the winning frame of a whole hull: the frames one at a time are what sees those)
    assert fails(lambda: er.check_hull(*er.model_obb_frames(verts, tri, "not_normalised"), href))


# ---- k_extreme_rows -------------------------------------------------------------------------------------------------
def oracle_extreme_rows(points, dirs):
    eng = OracleEngine()
    eng.set_cloud(0, points)
    return np.concatenate([eng.extreme_rows(0, dirs[b:b + 128]) for b in range(0, len(dirs), 128)])     # (bounded temporaries)


@pytest.mark.parametrize("n,ndirs", er.extreme_cases())
def test_planted_extremes_oracle_and_model(n, ndirs):
    worst = 0.0
    for dtype in sorted({dtype for dtype, _ in er.extreme_settings(n, ndirs)}):
        pts, dirs, planted = er.planted_cloud(n, ndirs, dtype)
        worst = max(worst, er.check_extreme(pts, dirs, oracle_extreme_rows(pts, dirs), planted, f"oracle {n} {ndirs} {dtype}"))
        if n <= 5000:
            worst = max(worst, er.check_extreme(pts, dirs, er.model_extreme_rows(pts, dirs), planted, f"model {n} {ndirs} {dtype}"))
    print(f"extreme n={n} ndirs={ndirs}: planted {len(planted)}, largest (max - got) / tau_k {worst:.3g}")


def test_extreme_special_clouds_oracle_and_model():
    pts, dirs, planted = er.negative_side_cloud()
    dots = pts.astype(np.float64) @ dirs.astype(np.float64).T
    assert np.sum(np.all(dots < 0, axis=0)) >= len(dirs) // 3              # wholly on the negative side of a third of them
    for rows in (oracle_extreme_rows(pts, dirs), er.model_extreme_rows(pts, dirs)):
        print("negative side:", er.check_extreme(pts, dirs, rows, planted))
    pts, dirs, planted = er.duplicated_cloud()
    for rows in (oracle_extreme_rows(pts, dirs), er.model_extreme_rows(pts, dirs)):     # (the two pick different rows of a pair)
        er.check_extreme(pts, dirs, rows, planted)
    pts, dirs = er.georeferenced_cloud()
    for rows in (oracle_extreme_rows(pts, dirs), er.model_extreme_rows(pts, dirs)):
        print("georeferenced:", er.check_extreme(pts, dirs, rows))


@pytest.mark.parametrize("defect,n,ndirs", [
    ("last_slice", 5000, 1006), ("last_slice", 257, 1006), ("last_slice", 63, 64),
    ("dirs_from_64", 5000, 65), ("dirs_from_64", 5000, 1006), ("dirs_from_64", 5000, 1024), ("dirs_from_64", 257, 65),
    ("no_sign_fix", 5000, 64), ("no_sign_fix", 5000, 1006), ("no_sign_fix", 257, 1006),
])
def test_extreme_defects_are_caught(defect, n, ndirs):
    pts, dirs, planted = er.planted_cloud(n, ndirs, "float32")
    er.check_extreme(pts, dirs, er.model_extreme_rows(pts, dirs), planted)
    assert fails(lambda: er.check_extreme(pts, dirs, er.model_extreme_rows(pts, dirs, defect), planted))


def test_the_sign_fix_is_caught_by_the_bound_alone_on_the_negative_side():
    pts, dirs, _ = er.negative_side_cloud()
    assert fails(lambda: er.check_extreme(pts, dirs, er.model_extreme_rows(pts, dirs, "no_sign_fix")))


# ---- k_outside_planes -----------------------------------------------------------------------------------------------
def oracle_rows_outside(points, planes, margin):
    out = []
    for b in range(0, len(points), 8192):
        eng = OracleEngine()
        eng.set_cloud(0, points[b:b + 8192])
        out.append(eng.rows_outside(0, planes, margin) + b)
    return np.concatenate(out)


@pytest.mark.parametrize("with_margin", [True, False], ids=["margin", "nomargin"])
@pytest.mark.parametrize("n,nplanes", er.outside_cases())
def test_outside_exact_set_oracle_model_and_defects(n, nplanes, with_margin):
    case = er.outside_case(n, nplanes, with_margin)
    er.check_outside(case, oracle_rows_outside(case["points"], case["planes"], case["margin"]), "oracle")
    if n > 1000 and nplanes > 4:
        return
    er.check_outside(case, er.model_rows_outside(case["points"], case["planes"], case["margin"]), "model")
    caught = {d for d in er.DEFECTS["outside"]
              if fails(lambda: er.check_outside(case, er.model_rows_outside(case["points"], case["planes"], case["margin"], d)))}
    assert ("first_tile_only" in caught) == (nplanes > 512)
    assert "last_plane" in caught
    assert ("rows_past_n" in caught) == (n % 256 != 0)
    if n >= 255:                                              # (the rows on a plane and a margin inside it exist)
        assert "greater_equal" in caught and ("margin_sign" in caught) == with_margin


@pytest.mark.parametrize("kind", ["all", "none"])
def test_outside_all_rows_and_no_row(kind):
    case = er.outside_case(257, 513, True, kind)
    assert len(case["expected"]) == (257 if kind == "all" else 0)
    er.check_outside(case, oracle_rows_outside(case["points"], case["planes"], case["margin"]))
    er.check_outside(case, er.model_rows_outside(case["points"], case["planes"], case["margin"]))
    if kind == "all":
        assert fails(lambda: er.check_outside(case, er.model_rows_outside(case["points"], case["planes"], case["margin"], "rows_past_n")))
