"""k_obb_frames, k_extreme_rows and k_outside_planes (csrc/pccm_obb.hip) through pccm_obb_frames, pccm_extreme_rows and
pccm_rows_outside, each against its own reference at the sizes where its walk can go wrong: an exact frame reference with the
derived tolerance tau_frame, exact integer plane tests, and planted extremes whose row the fp32 bound tau_k leaves no choice
about.  References, inputs and assertion helpers are tests/extent_reference.py; tests/test_extent_reference_host.py shows,
without a GPU, that each of these assertions fails for a kernel (model) that is wrong in one of fourteen ways.  The ratios of
error to tolerance are printed (pytest -s); DESIGN.md, "Minimal OBB", records them."""
import numpy as np
import pytest

from conftest import same_bits
import extent_reference as er
import p2d_reference
from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd import extent as ext_mod
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.point_cloud import PointCloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = nat.Engine(0)
    yield e
    e.close()


# ---- k_obb_frames -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", er.FRAME_NV)
@pytest.mark.parametrize("nt", er.FRAME_NT)
def test_one_frame_at_a_time(engine, nt, nv):
    """Frame t of a batch is read by making every other triangle degenerate (equal corners, collinear corners, in turn)."""
    tri, verts, ref, tau = er.frame_case(nv)
    worst = 0.0
    for t in er.frame_positions(nt):
        ext, vol = engine.obb_frames(verts, er.isolated_batch(tri, nt, t))
        worst = max(worst, er.check_frame(ext, vol, ref, tau, f"nt={nt} nv={nv} t={t}"))
    print(f"k_obb_frames nt={nt} nv={nv}: largest |ext - ext_ref| / tau_frame = {worst:.3f}")


@pytest.mark.parametrize("name,batch,want", er.tie_batches(), ids=[b[0] for b in er.tie_batches()])
def test_exact_ties_return_the_first_frame(engine, name, batch, want):
    """Six frames of exactly the same volume 1.25: the first finite one in the list, bit for bit."""
    corners, _ = er.tie_box()
    er.check_tie(engine.obb_frames(corners, batch), want)


def test_no_finite_frame_is_an_error(engine):
    corners, _ = er.tie_box()
    with pytest.raises(ValueError):
        engine.obb_frames(corners, np.stack([er.degenerate_triangle(i) for i in range(257)]))


@pytest.mark.parametrize("kind", er.HULLS)
def test_whole_hulls(engine, kind):
    verts, tri = er.hull_case(kind)
    ext, vol = engine.obb_frames(verts, tri)
    ratio = er.check_hull(ext, vol, er.hull_case_reference(kind), kind)
    print(f"k_obb_frames hull {kind} (nv {len(verts)}, nt {len(tri)}): |ext - ext_ref| / tau_frame = {ratio:.3f}")


# ---- k_extreme_rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ndirs", er.extreme_cases())
def test_planted_extremes(engine, n, ndirs):
    worst = 0.0
    for dtype, slot in er.extreme_settings(n, ndirs):
        pts, dirs, planted = er.planted_cloud(n, ndirs, dtype)
        engine.set_cloud(slot, pts)
        rows = engine.extreme_rows(slot, dirs)
        worst = max(worst, er.check_extreme(pts, dirs, rows, planted, f"n={n} ndirs={ndirs} {dtype} slot {slot}"))
    print(f"k_extreme_rows n={n} ndirs={ndirs}: largest (max - got) / tau_k = {worst:.3g}")


def test_extremes_on_the_negative_side_duplicates_and_far_from_the_origin(engine):
    for dtype, slot in (("float32", 0), ("float64", 1)):
        pts, dirs, planted = er.negative_side_cloud(dtype)
        engine.set_cloud(slot, pts)
        print("k_extreme_rows negative side:", er.check_extreme(pts, dirs, engine.extreme_rows(slot, dirs), planted, f"negative {dtype}"))
    pts, dirs, planted = er.duplicated_cloud()
    engine.set_cloud(0, pts)
    er.check_extreme(pts, dirs, engine.extreme_rows(0, dirs), planted, "duplicates")
    pts, dirs = er.georeferenced_cloud()
    engine.set_cloud(1, pts)
    print("k_extreme_rows georeferenced (bound only):", er.check_extreme(pts, dirs, engine.extreme_rows(1, dirs), None, "georeferenced"))


def test_direction_counts_outside_1_to_1024_are_refused(engine):
    engine.set_cloud(0, er.planted_cloud(257, 65, "float32")[0])
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            engine.extreme_rows(0, np.ones((bad, 3), dtype=np.float32))


# ---- k_outside_planes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_margin", [True, False], ids=["margin", "nomargin"])
@pytest.mark.parametrize("n,nplanes", er.outside_cases())
def test_rows_outside_is_the_exact_set(engine, n, nplanes, with_margin):
    case = er.outside_case(n, nplanes, with_margin)
    slot = (n + nplanes) % 2
    engine.set_cloud(slot, case["points"])
    er.check_outside(case, engine.rows_outside(slot, case["planes"], case["margin"]), f"n={n} nplanes={nplanes}")


@pytest.mark.parametrize("kind", ["all", "none"])
def test_rows_outside_all_rows_and_no_row(engine, kind):
    case = er.outside_case(257, 513, True, kind)
    engine.set_cloud(0, case["points"])
    er.check_outside(case, engine.rows_outside(0, case["planes"], case["margin"]), kind)


# ---- thinning, end to end -----------------------------------------------------------------------------------------
def _thinning_cloud(kind):
    if kind == "georeferenced":
        return p2d_reference.georeferenced(60000, 11)
    cube = np.random.default_rng(21).random((60000, 3))
    return cube + (np.array([5e5, 5.6e6, 300.0]) if kind == "cube_far" else 0.0)


@pytest.mark.parametrize("kind", ["cube_far", "cube_origin", "georeferenced"])
def test_thinning_keeps_every_hull_vertex_and_thins(engine, kind):
    from scipy.spatial import ConvexHull
    pts = _thinning_cloud(kind)
    engine.set_cloud(0, pts)
    keep = ext_mod.hull_candidates(pts, engine)
    print(f"thinning {kind}: kept {len(keep)} of {len(pts)}")
    assert set(ConvexHull(pts).vertices.tolist()) <= set(keep.tolist())
    assert len(keep) < len(pts) // 3


def test_a_large_planar_cloud_raises_what_a_small_one_raises():
    rng = np.random.default_rng(5)
    def planar(n):
        uv = rng.integers(0, 2 ** 20, (n, 2)) / 2.0 ** 20             # (z below is exact: the cloud IS planar in fp64)
        return np.column_stack([uv[:, 0], uv[:, 1], 0.25 * uv[:, 0] + 0.5 * uv[:, 1]])
    assert 25000 >= ext_mod._THIN_ABOVE > 1000
    raised = []
    for n in (1000, 25000):
        pts = planar(n)
        with pytest.raises(Exception) as info:
            CloudPair(PointCloud(pts), PointCloud(pts + 0.01)).get_extent()
        raised.append(info.type)
    assert raised[0] is raised[1], raised


# ---- the scratch the three calls share with the colour pass -------------------------------------------------------
def test_extent_calls_between_colour_calls_leave_the_colours_alone():
    rng = np.random.default_rng(9)
    a, b = rng.random((3000, 3)), rng.random((2800, 3))
    ca, cb = rng.integers(0, 256, (3000, 3)) / 255.0, rng.integers(0, 256, (2800, 3)) / 255.0
    verts, tri = er.hull_case("sphere")                    # 13 doubles per triangle: more scratch than the colour columns
    assert (3 * len(verts) + 13 * len(tri)) > 3 * (len(a) + len(b))
    case = er.outside_case(257, 2000, True)

    def run(with_extent_calls):
        e = nat.Engine(0)
        try:
            e.set_cloud(0, a); e.set_cloud(1, b)
            e.set_colors(0, ca); e.set_colors(1, cb)
            e.nn_pair()
            out = [e.color_reduce(nat.DIR_LEFT, "ycc")]
            if with_extent_calls:
                dirs = er.directions(1006)
                er.check_extreme(a, dirs, e.extreme_rows(0, dirs), None, "between colour calls")
                planes = case["planes"]
                want = np.nonzero(np.any(a @ planes[:, :3].T + planes[:, 3] > -case["margin"], axis=1))[0]
                assert np.array_equal(np.sort(e.rows_outside(0, planes, case["margin"])), want)
                er.check_hull(*e.obb_frames(verts, tri), er.hull_case_reference("sphere"), "between colour calls")
            out.append(e.color_reduce(nat.DIR_RIGHT, "ycc"))
            rows = [e.color_rows(d, "ycc", nat.COLOR_SQUARE) for d in (nat.DIR_LEFT, nat.DIR_RIGHT)]
            return out, rows
        finally:
            e.close()

    (got, got_rows), (want, want_rows) = run(True), run(False)
    for g, w in zip(got, want):
        assert same_bits(g[0], w[0]) and same_bits(g[1], w[1])
    for g, w in zip(got_rows, want_rows):
        assert same_bits(g, w)
