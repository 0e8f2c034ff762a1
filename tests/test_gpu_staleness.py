"""What goes stale when a cloud's inputs change ("What goes stale when"; open_pcc_metric_amd/csrc/pccm_stale.h): every
case runs a sequence of calls on one context and compares each number it reads afterwards, bit for bit, with a fresh context that
was given the final inputs directly.  Both sides are this library on the same data, so there is no tolerance anywhere.

Clouds of 1500 and 1700 random points (more than one 128-row leaf, the last one ragged) with fp32-exact coordinates, random unit
normals, random byte colours; the grid engine is forced; PointSSIM k = 8, point-to-distribution k = 6, spacings K = 4."""
import functools

import numpy as np
import pytest

from open_pcc_metric_amd import _native as nat

pytestmark = pytest.mark.gpu

L, R, S = nat.DIR_LEFT, nat.DIR_RIGHT, nat.DIR_SELF
D1, D2 = nat.METRIC_D1, nat.METRIC_D2
K_SSIM, K_P2D, K_RES = 8, 6, 4
P2D_BOTH = nat.P2D_GEOMETRY | nat.P2D_COLOR


def unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def data():
    rng = np.random.default_rng(20)
    d = {"a": rng.random((1500, 3), dtype=np.float32), "b": rng.random((1700, 3), dtype=np.float32),
         "b2": rng.random((1700, 3), dtype=np.float32)}
    for k, n in (("na", 1500), ("na2", 1500), ("nb", 1700), ("nb2", 1700)):
        d[k] = unit(rng, n)
    for k, n in (("ca", 1500), ("ca2", 1500), ("cb", 1700)):
        d[k] = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    for v in d.values():
        v.setflags(write=False)
    return d


class Ctx:
    """An engine that is closed when the test is done with it."""
    def __init__(self, a=None, b=None, na=None, nb=None, ca=None, cb=None):
        self.eng = nat.Engine(0)
        for which, pts, nrm, rgb in ((0, a, na, ca), (1, b, nb, cb)):
            if pts is not None:
                self.eng.set_cloud(which, pts)
            if nrm is not None:
                self.eng.set_normals(which, nrm)
            if rgb is not None:
                self.eng.set_colors_u8(which, rgb)

    def __enter__(self):
        return self.eng

    def __exit__(self, *exc):
        self.eng.close()


def bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


def totals(eng, requests, mode="row"):
    return bits(eng.reduce_total_many(requests, mode))


# ---- 1. a projection fused into the search does not outlive the normals it was made from ------------------------------------

def new_normals(eng, how):
    d = data()
    if how == "uploaded":
        eng.set_normals(1, d["nb2"])
    elif how == "announced":
        eng.set_normals_deferred(1, d["nb2"])
    elif how == "estimated":
        eng.estimate_normals(1, 8)
    else:
        raise KeyError(how)


@pytest.mark.parametrize("want_idx", [True, False], ids=["rows", "no_rows"])
@pytest.mark.parametrize("mode", ["row", "neighbour"])
@pytest.mark.parametrize("how", ["uploaded", "announced", "estimated"])
def test_new_normals_void_a_fused_projection(how, mode, want_idx):
    """pccm_nn_fuse is "purely an optimisation: results are bit-identical either way" (include/pccm.h).  On fp32-exact clouds the
    row-indexed projection is left to the reduction (matched records), which reads the current normals; the neighbour-indexed
    one is stored by the search (pair records) and has to be forgotten with the normals."""
    d = data()
    with Ctx(d["a"], d["b"], d["na"], d["nb"]) as eng:
        eng.nn_fuse(L, mode)
        eng.nn_want_idx(want_idx)
        eng.nn_pair("grid")
        before = totals(eng, [(L, D2)], mode)
        new_normals(eng, how)
        after = totals(eng, [(L, D2)], mode)
        column = bits(eng.point_metric(L, D2, mode))
    for fuse in (mode, None):                                   # the final inputs given directly, fused and not
        with Ctx(d["a"], d["b"], d["na"]) as ref:
            new_normals(ref, how)
            ref.nn_fuse(L, fuse)
            ref.nn_want_idx(want_idx)
            ref.nn_pair("grid")
            want = totals(ref, [(L, D2)], mode)
            want_column = bits(ref.point_metric(L, D2, mode))
        print(f"{how} / {mode} / rows {want_idx} / reference fused {fuse}: after == fresh {after == want}, before == fresh {before == want}")
        assert after == want and column == want_column
    assert before != want                                       # (the new normals do change the column)


# ---- 2. new colours -------------------------------------------------------------------------------------------------------------

def test_new_colours_drop_the_memo_the_colour_features_and_the_colour_columns():
    d = data()
    p2d = [(L, nat.METRIC_P2D), (R, nat.METRIC_P2D), (L, nat.METRIC_P2D_COLOR), (R, nat.METRIC_P2D_COLOR), (L, nat.METRIC_P2D_JOINT),
           (R, nat.METRIC_P2D_JOINT)]
    with Ctx(d["a"], d["b"], ca=d["ca2"], cb=d["cb"]) as ref:
        ref.nn_pair("grid")
        want_right, want_left = ref.color_reduce(R, "rgb"), ref.color_reduce(L, "rgb")     # (RIGHT first: computed, not remembered)
        assert ref.ssim_features(0, K_SSIM, ["color"]) is True
        want_feature = bits(ref.get_ssim_features(0, "color"))
        assert ref.p2d_build(K_P2D, P2D_BOTH) is True
        want_p2d = totals(ref, p2d)
    with Ctx(d["a"], d["b"], ca=d["ca"], cb=d["cb"]) as eng:
        eng.nn_pair("grid")
        assert eng.ssim_features(0, K_SSIM, ["color"]) is True and eng.ssim_features(1, K_SSIM, ["color"]) is True
        other_feature = bits(eng.get_ssim_features(1, "color"))
        assert eng.p2d_build(K_P2D, P2D_BOTH) is True
        eng.color_reduce(L, "rgb")
        old_right = eng.color_reduce(R, "rgb")                  # (the memo's answer)
        eng.color_reduce(L, "rgb")                              # RIGHT rides along again: the memo holds it when the colours change
        eng.set_colors_u8(0, d["ca2"])
        for got, want in zip(eng.color_reduce(R, "rgb") + eng.color_reduce(L, "rgb"), want_right + want_left):
            assert bits(got) == bits(want)
        assert bits(old_right[0]) != bits(want_right[0])
        with pytest.raises(nat.PccmStateError):                 # the colour feature column needs a rebuild ...
            eng.get_ssim_features(0, "color")
        assert bits(eng.get_ssim_features(1, "color")) == other_feature                    # ... cloud 1's does not
        assert eng.ssim_features(1, K_SSIM, ["color"]) is False
        assert eng.ssim_features(0, K_SSIM, ["color"]) is True
        assert bits(eng.get_ssim_features(0, "color")) == want_feature
        assert eng.p2d_build(K_P2D, nat.P2D_GEOMETRY) is False  # the geometry columns stayed
        with pytest.raises(nat.PccmStateError):
            eng.reduce_total(L, nat.METRIC_P2D_COLOR)
        assert eng.p2d_build(K_P2D, P2D_BOTH) is True           # the colour and joint columns did not
        assert totals(eng, p2d) == want_p2d


# ---- 3. new normals -------------------------------------------------------------------------------------------------------------

def test_new_normals_keep_spacings_and_geometry_columns():
    d = data()
    with Ctx(d["a"], d["b"], d["na2"], d["nb"]) as ref:
        assert ref.resolution_build(0, K_RES) is True and ref.resolution_build(1, K_RES) is True
        want = [bits(ref.get_resolution(k)) for k in (0, 1)]
        assert ref.p2d_build(K_P2D) is True
        ref.nn_pair("grid")
        want_p2d = totals(ref, [(L, nat.METRIC_P2D), (R, nat.METRIC_P2D)])
    with Ctx(d["a"], d["b"], d["na"], d["nb"]) as eng:
        assert eng.resolution_build(0, K_RES) is True and eng.resolution_build(1, K_RES) is True
        assert eng.p2d_build(K_P2D) is True
        eng.nn_pair("grid")
        eng.set_normals(0, d["na2"])
        assert eng.resolution_build(0, K_RES) is False and eng.resolution_build(1, K_RES) is False
        assert eng.p2d_build(K_P2D) is False
        assert [bits(eng.get_resolution(k)) for k in (0, 1)] == want
        assert totals(eng, [(L, nat.METRIC_P2D), (R, nat.METRIC_P2D)]) == want_p2d


def test_new_normals_drop_what_was_carried_from_them_and_replace_what_was_carried_to_them():
    d = data()
    with Ctx(d["a"], d["b"], na=d["na"]) as eng:                 # carried from cloud 0: gone with cloud 0's normals
        eng.nn_pair("grid")
        assert eng.carry_normals(0) is True
        assert eng.get_normals(1).shape == (1700, 3)
        eng.set_normals(0, d["na2"])
        with pytest.raises(nat.PccmStateError):
            eng.get_normals(1)
        assert bits(eng.get_normals(0)) == bits(d["na2"])
    with Ctx(d["a"], d["b"], nb=d["nb"]) as eng:                 # carried to cloud 0: replaced, and cloud 1 keeps its own
        eng.nn_pair("grid")
        assert eng.carry_normals(1) is True
        eng.set_normals(0, d["na2"])
        assert bits(eng.get_normals(0)) == bits(d["na2"])
        assert bits(eng.get_normals(1)) == bits(d["nb"])
        with Ctx(d["a"], d["b"], d["na2"], d["nb"]) as ref:
            ref.nn_pair("grid")
            assert totals(eng, [(L, D2), (R, D2)], NBR) == totals(ref, [(L, D2), (R, D2)], NBR)


# ---- 4. new points for cloud 1 --------------------------------------------------------------------------------------------------

def test_new_points_for_cloud_1_keep_the_self_search_of_cloud_0():
    d = data()
    with Ctx(d["a"], d["b2"]) as ref:
        ref.nn(S, "grid")
        want = ref.fetch_nn(S)
    with Ctx(d["a"], np.concatenate([d["b"], d["b"][:100]])) as eng:
        assert eng.merge_duplicates(1, "drop") == 1700
        assert not np.array_equal(eng.get_merge_map(1), np.arange(1800))
        eng.nn(S, "grid")
        eng.nn_pair("grid")
        eng.set_cloud(1, d["b2"])
        got = eng.fetch_nn(S)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        for direction in (L, R):
            with pytest.raises(nat.PccmStateError):
                eng.fetch_nn(direction)
        assert np.array_equal(eng.get_merge_map(1), np.arange(1700))


# ---- 5. captured graphs ---------------------------------------------------------------------------------------------------------

GRAPH_REQ = [(L, D1), (R, D1), (L, D2), (R, D2)]
NBR = "neighbour"       # (the row-indexed projection of RIGHT would index 1500 normals with 1700 rows: the reference's IndexError)


def captured(eng):
    """-> graph id of {drop_caches, nn_pair, D1 / D2 prefetches} (run eagerly twice first: a capture allocates nothing)."""
    for _ in range(2):
        eng.drop_caches()
        eng.nn_pair("grid")
        eng.reduce_prefetch_many(GRAPH_REQ, NBR)
        eng.reduce_total_many(GRAPH_REQ, NBR)
    eng.graph_begin()
    eng.drop_caches()
    eng.nn_pair("grid")
    eng.reduce_prefetch_many(GRAPH_REQ, NBR)
    return eng.graph_end()


CHANGES = {
    "new_points": lambda eng: eng.set_cloud(1, data()["b2"]),
    "new_normals": lambda eng: eng.set_normals(1, data()["nb2"]),
    "shard_dir": lambda eng: eng.set_shard_dir(L, 0, 1),
    "ties": lambda eng: eng.set_ties("mean"),
}


@pytest.mark.parametrize("change", sorted(CHANGES))
def test_a_captured_graph_is_stale_after(change):
    d = data()
    with Ctx(d["a"], d["b"], d["na"], d["nb"], d["ca"], d["cb"]) as eng:
        gid = captured(eng)
        eng.graph_launch(gid)
        eng.reduce_total_many(GRAPH_REQ, NBR)
        CHANGES[change](eng)
        with pytest.raises(nat.PccmStateError):
            eng.graph_launch(gid)


def test_a_captured_graph_replays_after_new_colours():
    d = data()
    with Ctx(d["a"], d["b"], d["na"], d["nb"]) as ref:
        ref.nn_pair("grid")
        want = totals(ref, GRAPH_REQ, NBR)
    with Ctx(d["a"], d["b"], d["na"], d["nb"], d["ca"], d["cb"]) as eng:
        gid = captured(eng)
        assert totals(eng, GRAPH_REQ, NBR) == want
        eng.set_colors_u8(0, d["ca2"])
        eng.graph_launch(gid)
        assert totals(eng, GRAPH_REQ, NBR) == want


# ---- 6. pccm_ctx_reset ----------------------------------------------------------------------------------------------------------

def test_after_a_reset_every_getter_and_reduction_reports_a_state_error():
    d = data()
    with Ctx(np.concatenate([d["a"], d["a"][:50]]), d["b"], None, d["nb"], None, d["cb"]) as eng:
        assert eng.merge_duplicates(0, "drop") == 1500
        eng.set_normals(0, d["na"])
        eng.set_colors_u8(0, d["ca"])
        eng.nn_pair("grid")
        eng.nn(S, "grid")
        for which in (0, 1):
            eng.ssim_features(which, K_SSIM, ["geometry", "normal", "curvature", "color"])
            eng.resolution_build(which, K_RES)
        eng.p2d_build(K_P2D, P2D_BOTH)
        eng.reduce_total_many(GRAPH_REQ, NBR)
        eng.color_reduce(L, "rgb")
        eng.reset()
        eng._n = [1500, 1700]                                   # (the wrapper sizes its output arrays by what it was given)
        eng._p2d_k = K_P2D
        calls = [lambda w=w, f=f: f(w) for w in (0, 1)
                 for f in (eng.get_points, eng.get_normals, eng.get_colors, eng.get_resolution, eng.get_merge_map,
                           lambda w: eng.get_ssim_features(w, "geometry"), lambda w: eng.get_ssim_features(w, "color"))]
        calls += [lambda dr=dr: eng.fetch_nn(dr) for dr in (L, R, S)]
        calls += [lambda dr=dr: eng.get_p2d_neighbours(dr) for dr in (L, R)]
        calls += [lambda dr=dr, m=m: eng.reduce_total(dr, m) for dr in (L, R)
                  for m in (D1, D2, nat.METRIC_ANGULAR, nat.METRIC_SSIM["geometry"], nat.METRIC_P2D, nat.METRIC_P2D_COLOR,
                            nat.METRIC_RESOLUTION)]
        calls += [lambda: eng.reduce_total(S, D1), lambda: eng.color_reduce(L, "rgb"), lambda: eng.select_many([(L, D1, 10)]),
                  lambda: eng.carry_normals(0)]
        for k, call in enumerate(calls):
            with pytest.raises(nat.PccmStateError):
                call()
