"""Merged duplicate points on the GPU (include/pccm.h, pccm_merge_duplicates): the stored points, normals, colours and the map after
the call against the NumPy restatement of tests/merge_reference.py, compared as raw bytes (signed zeros count) in both modes; the
entry point's state rules and errors; and whole reports of ``CloudPair(..., duplicates=mode)`` against a pair that was GIVEN the
restated merged clouds.

Normals are ``standard_normal * 10**uniform(-3, 3)`` per row and colours ``random * 10**uniform(-6, 0)`` per row in every family,
so that the order of a sum shows in its last bits: a kernel that adds in arrival order cannot pass."""
import functools

import numpy as np
import pytest
from click.testing import CliRunner

from merge_reference import drawn_20000, merged, merged_reversed
from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import write_point_cloud
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud

pytestmark = pytest.mark.gpu

MODES = ["drop", "average"]


def wild_normals(rng, n):
    return rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))


def wild_colours(rng, n):
    return rng.random((n, 3)) * 10.0 ** rng.uniform(-6, 0, (n, 1))


PLANTED_COUNTS = np.array(list(range(1, 132)) + [1000, 5000])          # lists on both sides of kCarryLong (128), and the walk


@functools.lru_cache(maxsize=None)
def family(name):
    """-> (points, normals, colours)."""
    rng = np.random.default_rng(7)
    col = None
    if name in ("drawn_20000", "drawn_20000_f64"):
        pts, col = drawn_20000()
        if name.endswith("f64"):
            pts = pts.astype(np.float64)
    elif name == "planted":
        pos = rng.random((len(PLANTED_COUNTS), 3), dtype=np.float32)
        pts = np.repeat(pos, PLANTED_COUNTS, axis=0)
        pts = pts[rng.permutation(len(pts))]
    elif name == "all_identical":
        pts = np.repeat(rng.random((1, 3), dtype=np.float32), 20000, axis=0)
    elif name == "no_duplicates_5000":
        pts = rng.random((5000, 3), dtype=np.float32)
    elif name == "one_point":
        pts = rng.random((1, 3), dtype=np.float32)
    elif name == "two_same":
        pts = np.repeat(rng.random((1, 3), dtype=np.float32), 2, axis=0)
    elif name == "two_distinct":
        pts = rng.random((2, 3), dtype=np.float32)
    elif name == "signed_zeros":
        base = np.array([[0, 0, 0], [1, 0, 2], [0, 3, 0], [4, 5, 0], [0, 0, 6], [7, 0, 0], [0, 8, 9]], dtype=np.float64)
        pts = np.repeat(base, 40, axis=0)
        flip = (rng.random(pts.shape) < 0.5) & (pts == 0.0)
        pts = np.where(flip, -0.0, pts)
        pts = pts[rng.permutation(len(pts))]
    elif name == "one_ulp":
        first = rng.random((4000, 3))
        later = first.copy()
        axis = rng.integers(0, 3, 4000)
        later[np.arange(4000), axis] = np.nextafter(first[np.arange(4000), axis], 2.0)
        pts = np.concatenate([first, later])
    elif name == "georeferenced_f64":
        cells = np.unique(rng.integers(0, 64, (6000, 3)), axis=0)
        cells = cells[rng.permutation(len(cells))[:3000]]
        uniq = np.array([1.0e6, 2.0e6, 3.0e6]) + cells * 2.0 ** -20
        pts = np.concatenate([uniq, uniq[rng.integers(0, 3000, 2000)]])
        pts = pts[rng.permutation(len(pts))]
    elif name == "lattice_16":
        pts = rng.integers(0, 16, (50000, 3)).astype(np.float32)
    else:
        raise KeyError(name)
    n = len(pts)
    rng = np.random.default_rng(8)
    nrm = wild_normals(rng, n)
    if col is None:
        col = wild_colours(rng, n)
    return pts, nrm, col


@functools.lru_cache(maxsize=None)
def restated(name, mode):
    return merged(*family(name), mode)


@functools.lru_cache(maxsize=None)
def library(name, mode):
    """One merge through the ABI: (n', points, normals, colours, map) as the library holds them afterwards."""
    pts, nrm, col = family(name)
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, pts)
        eng.set_normals(0, nrm)
        eng.set_colors(0, col)
        n_new = eng.merge_duplicates(0, mode)
        assert eng.n_iter(nat.DIR_LEFT) == n_new
        got = (n_new, eng.get_points(0), eng.get_normals(0), eng.get_colors(0), eng.get_merge_map(0))
        eng.sync()
    finally:
        eng.close()
    return got


FAMILIES = ["drawn_20000", "planted", "all_identical", "no_duplicates_5000", "one_point", "two_same", "two_distinct", "signed_zeros",
            "one_ulp", "georeferenced_f64", "lattice_16"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FAMILIES)
def test_merged_cloud_equals_the_restatement_bit_for_bit(name, mode):
    want_p, want_n, want_c, want_m = restated(name, mode)
    n_new, got_p, got_n, got_c, got_m = library(name, mode)
    counts = np.bincount(want_m)
    print(f"{name} / {mode}: {len(want_m)} rows -> {len(want_p)}, longest group {counts.max()}, groups with m >= 3: {(counts >= 3).sum()}")
    assert n_new == len(want_p)
    assert got_m.dtype == np.int32 and got_m.tobytes() == want_m.tobytes()
    assert got_p.shape == want_p.shape and got_p.tobytes() == want_p.tobytes()
    assert got_n.shape == want_n.shape and got_n.tobytes() == want_n.tobytes()
    bad = np.flatnonzero(np.any(got_c.view(np.uint64) != want_c.view(np.uint64), axis=1))
    assert got_c.shape == want_c.shape and len(bad) == 0, (bad[:8], counts[bad[:8]])


def test_families_are_what_they_claim():
    assert len(restated("planted", "drop")[0]) == 133
    assert np.array_equal(np.sort(np.bincount(restated("planted", "drop")[3])), np.sort(PLANTED_COUNTS))
    assert len(restated("all_identical", "drop")[0]) == 1
    assert len(restated("one_ulp", "drop")[0]) == 8000
    pts = family("georeferenced_f64")[0]
    assert len(restated("georeferenced_f64", "drop")[0]) == 3000 and len(np.unique(pts.astype(np.float32), axis=0)) < 100
    assert len(restated("lattice_16", "drop")[0]) <= 4096
    pz, _, _, mz = restated("signed_zeros", "drop")
    assert len(pz) == 7 and np.signbit(family("signed_zeros")[0]).any()
    for g in range(7):                                                   # every group mixes both zeros
        rows = family("signed_zeros")[0][mz == g]
        assert len(np.unique(np.signbit(rows), axis=0)) > 1
    assert [len(restated(k, "drop")[0]) for k in ("one_point", "two_same", "two_distinct")] == [1, 1, 2]


def test_float32_and_float64_uploads_give_identical_bytes():
    for mode in MODES:
        a, b = library("drawn_20000", mode), library("drawn_20000_f64", mode)
        assert a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


def test_averages_follow_ascending_row_order_and_not_the_reverse():
    pts, nrm, col = family("drawn_20000")
    _, _, _, got_c, got_m = library("drawn_20000", "average")
    want = restated("drawn_20000", "average")[2]
    rev = merged_reversed(pts, nrm, col, "average")[2]
    counts = np.bincount(got_m)
    moved = np.any(rev.view(np.uint64) != got_c.view(np.uint64), axis=1)
    print("rows the reversed order moves:", int(moved.sum()), "of", int((counts >= 3).sum()), "with m >= 3")
    assert got_c.tobytes() == want.tobytes()
    assert moved.sum() >= 1000 and not moved[counts < 3].any()


def test_a_cloud_without_duplicates_is_left_untouched():
    pts, nrm, col = family("no_duplicates_5000")
    other = np.random.default_rng(9).random((3000, 3), dtype=np.float32)
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, pts)
        eng.set_cloud(1, other)
        eng.set_normals(0, nrm)
        eng.set_colors(0, col)
        eng.nn_pair("auto")
        idx, d2 = eng.fetch_nn(nat.DIR_LEFT)
        for mode in MODES:
            assert eng.merge_duplicates(0, mode) == 5000
            assert eng.get_points(0).tobytes() == pts.astype(np.float64).tobytes()
            assert eng.get_normals(0).tobytes() == nrm.tobytes() and eng.get_colors(0).tobytes() == col.tobytes()
            assert np.array_equal(eng.get_merge_map(0), np.arange(5000, dtype=np.int32))
            again = eng.fetch_nn(nat.DIR_LEFT)                           # (no rerun: the results are still there)
            assert again[0].tobytes() == idx.tobytes() and again[1].tobytes() == d2.tobytes()
            assert eng.fetch_nn(nat.DIR_RIGHT)[0].shape == (3000,)
    finally:
        eng.close()


# ---- state and errors through the ABI -----------------------------------------------------------------------------------------
@pytest.fixture
def small():
    """Cloud 0: 3000 rows over 2000 positions, with normals and colours; cloud 1: 1000 distinct rows."""
    rng = np.random.default_rng(11)
    keys = rng.random((2000, 3), dtype=np.float32)
    a = np.concatenate([keys, keys[rng.integers(0, 2000, 1000)]])[rng.permutation(3000)]
    b = rng.random((1000, 3), dtype=np.float32)
    eng = nat.Engine(0)
    eng.set_cloud(0, a)
    eng.set_cloud(1, b)
    yield eng, a, b, rng
    eng.close()


def test_argument_errors(small):
    eng, *_ = small
    for which in (-1, 2):
        with pytest.raises(ValueError):
            eng.merge_duplicates(which, "drop")
        with pytest.raises(ValueError):
            eng.get_merge_map(which)
    for mode in (0, 3, "keep", "bogus"):
        with pytest.raises(ValueError):
            eng.merge_duplicates(0, mode)
    assert eng.n_iter(nat.DIR_LEFT) == 3000                              # nothing happened


def test_state_errors(small):
    eng, a, b, rng = small
    fresh = nat.Engine(0)
    try:
        with pytest.raises(nat.PccmStateError):                         # the cloud is missing
            fresh.merge_duplicates(0, "drop")
        with pytest.raises(nat.PccmStateError):
            fresh.get_merge_map(0)
        with pytest.raises(nat.PccmStateError):
            fresh.get_points(0)
    finally:
        fresh.close()
    with pytest.raises(nat.PccmStateError):                             # no colours to fetch
        eng.get_colors(0)
    eng.set_normals(0, wild_normals(rng, 2999))                         # (the row-indexed quirk allows such normals elsewhere)
    with pytest.raises(nat.PccmStateError):
        eng.merge_duplicates(0, "drop")
    eng.set_normals(0, wild_normals(rng, 3000))
    eng.set_shard(0, 2)
    with pytest.raises(nat.PccmStateError):                             # sharded
        eng.merge_duplicates(0, "drop")
    eng.set_shard(0, 1)
    eng.graph_begin()
    try:
        with pytest.raises(nat.PccmStateError):                         # between graph_begin and graph_end
            eng.merge_duplicates(0, "drop")
    finally:
        eng.graph_abort()
    assert eng.n_iter(nat.DIR_LEFT) == 3000
    eng.set_ties("mean")                                                # the tie policy does not matter
    assert eng.merge_duplicates(0, "average") == 2000


def test_a_merge_that_drops_rows_invalidates_like_new_points(small):
    eng, a, b, rng = small
    nrm, col = wild_normals(rng, 3000), wild_colours(rng, 3000)
    eng.set_normals_deferred(0, nrm)                                    # announced only: the merge uploads them first
    eng.set_colors(0, col)
    eng.set_normals(1, wild_normals(rng, 1000))
    eng.nn_pair("auto")
    eng.nn(nat.DIR_SELF, "auto")
    eng.fetch_nn(nat.DIR_LEFT)
    assert eng.merge_duplicates(1, "average") == 1000                   # cloud 1 has none: everything stays
    eng.fetch_nn(nat.DIR_LEFT)
    eng.fetch_nn(nat.DIR_SELF)
    assert eng.merge_duplicates(0, "average") == 2000
    assert eng.n_iter(nat.DIR_LEFT) == 2000 and eng.n_iter(nat.DIR_RIGHT) == 1000
    for direction in (nat.DIR_LEFT, nat.DIR_RIGHT, nat.DIR_SELF):
        with pytest.raises(nat.PccmStateError):                         # the old results are gone until the search is rerun
            eng.fetch_nn(direction)
    want_p, want_n, want_c, want_m = merged(a, nrm, col, "average")
    assert eng.get_points(0).tobytes() == want_p.tobytes() and eng.get_normals(0).tobytes() == want_n.tobytes()
    assert eng.get_colors(0).tobytes() == want_c.tobytes() and eng.get_merge_map(0).tobytes() == want_m.tobytes()
    eng.nn_pair("auto")
    idx, d2 = eng.fetch_nn(nat.DIR_LEFT)
    assert idx.shape == (2000,) and eng.fetch_nn(nat.DIR_RIGHT)[0].max() < 2000
    # a second merge finds nothing and changes nothing: results, arrays and the first merge's map stay
    for mode in MODES:
        assert eng.merge_duplicates(0, mode) == 2000
        assert eng.fetch_nn(nat.DIR_LEFT)[1].tobytes() == d2.tobytes()
        assert eng.get_colors(0).tobytes() == want_c.tobytes() and eng.get_merge_map(0).tobytes() == want_m.tobytes()
    # the same state as the set_* calls with the merged arrays would have left: the same search results
    ref = nat.Engine(0)
    try:
        ref.set_cloud(0, want_p)
        ref.set_cloud(1, b)
        ref.nn_pair("auto")
        assert ref.fetch_nn(nat.DIR_LEFT)[1].tobytes() == d2.tobytes() and ref.fetch_nn(nat.DIR_LEFT)[0].tobytes() == idx.tobytes()
    finally:
        ref.close()
    eng.set_cloud(0, a)                                                 # new points: the map spoke of the old ones
    assert np.array_equal(eng.get_merge_map(0), np.arange(3000))


def test_ctx_reset_clears_the_map(small):
    eng, a, b, rng = small
    assert eng.merge_duplicates(0, "drop") == 2000
    assert len(eng.get_merge_map(0)) == 3000 and eng.get_merge_map(0).max() == 1999
    eng.reset()
    with pytest.raises(nat.PccmStateError):
        eng.get_merge_map(0)
    eng.set_cloud(0, b)
    assert np.array_equal(eng.get_merge_map(0), np.arange(1000))


def test_carried_normals_go_with_the_rows(small):
    eng, a, b, rng = small
    eng.set_normals(1, wild_normals(rng, 1000))
    eng.nn_pair("auto")
    assert eng.carry_normals(1) is True                                 # cloud 0 holds normals carried from cloud 1
    assert eng.get_normals(0).shape == (3000, 3)
    assert eng.merge_duplicates(0, "drop") == 2000
    with pytest.raises(nat.PccmStateError):                             # made from the old rows: gone, not merged
        eng.get_normals(0)


# ---- whole reports ------------------------------------------------------------------------------------------------------------
def with_duplicates(rng, uniq, extra):
    pts = np.concatenate([uniq, uniq[rng.integers(0, len(uniq), extra)]])
    return pts[rng.permutation(len(pts))]


@functools.lru_cache(maxsize=None)
def report_clouds():
    """Three clouds of 3000 to 6000 rows, about a third of them duplicates: (points, normals, byte colours) each."""
    rng = np.random.default_rng(21)
    base = rng.random((4000, 3), dtype=np.float32)
    out = []
    for uniq, extra in ((base, 2000), ((base[:3000] + rng.normal(0, 0.01, (3000, 3))).astype(np.float32), 1500),
                        ((base[500:2700] + rng.normal(0, 0.02, (2200, 3))).astype(np.float32), 1100)):
        pts = with_duplicates(rng, uniq, extra)
        out.append((pts, wild_normals(rng, len(pts)), rng.integers(0, 256, (len(pts), 3)) / 255.0))
    return out


def cloud(k, normals=True, colours=True):
    pts, nrm, col = report_clouds()[k]
    return PointCloud(pts, nrm if normals else None, col if colours else None)


def merged_cloud(k, mode, normals=True, colours=True):
    pts, nrm, col = report_clouds()[k]
    p, n, c, _ = merged(pts, nrm if normals else None, col if colours else None, mode)
    return PointCloud(p, n, c)


EXTENT = [1.0, 1.0, 1.0]
BASE = dict(color="ycc", hausdorff=True, point_to_plane=True)


def report_text(pair, **more):
    with np.errstate(divide="ignore", invalid="ignore"):
        return MetricCalculator(pair).calculate(transform_options(CalculateOptions(**{**BASE, **more}))).as_df().to_string()


def check_pair_bookkeeping(pair, ks):
    for which, k in enumerate(ks):
        pts = report_clouds()[k][0]
        want_map = merged(pts, None, None, "drop")[3]
        assert pair.duplicates_removed[which] == len(pts) - (int(want_map.max()) + 1) > 0
        assert np.array_equal(pair.merge_map(which), want_map)
    assert pair.clouds[0].points is not None and len(pair.clouds[0].points) == len(report_clouds()[ks[0]][0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["plain", "carry_normals", "point_ssim", "point_to_distribution", "use_graph", "ties_mean"])
def test_reports_on_merged_clouds_equal_reports_on_given_merged_clouds(case, mode):
    kw, more, nb = dict(normal_index="neighbour", extent=EXTENT), {}, True
    if case == "carry_normals":
        kw["carry_normals"], nb = True, False                           # normals on cloud 0 only
    elif case == "point_ssim":
        more["point_ssim"] = ("geometry", "color")
    elif case == "point_to_distribution":
        more["point_to_distribution"] = True
    elif case == "use_graph":
        kw["use_graph"] = True
    elif case == "ties_mean":
        kw["ties"] = "mean"
    with CloudPair(merged_cloud(0, mode), merged_cloud(1, mode, normals=nb), **kw) as given:
        want = report_text(given, **more)
    with CloudPair(cloud(0), cloud(1, normals=nb), duplicates=mode, **kw) as pair:
        for _ in range(4 if case == "use_graph" else 1):                # eager, capture, replays
            assert report_text(pair, **more) == want
            pair.recompute()
        check_pair_bookkeeping(pair, (0, 1))
        assert (pair._engine.n_iter(nat.DIR_LEFT), pair._engine.n_iter(nat.DIR_RIGHT)) == (4000, 3000)
        assert case != "use_graph" or pair._graph_id is not None
        assert case != "carry_normals" or pair._carried == [False, True]
    with CloudPair(cloud(0), cloud(1, normals=nb), **kw) as kept:       # the keyword matters: the unmerged pair reports otherwise
        assert report_text(kept, **more) != want and kept.duplicates_removed == (0, 0)


@pytest.mark.parametrize("mode", MODES)
def test_with_reconst_merges_every_decoded_cloud(mode):
    kw = dict(normal_index="neighbour", extent=EXTENT)
    want = []
    for k in (1, 2):
        with CloudPair(merged_cloud(0, mode), merged_cloud(k, mode), **kw) as given:
            want.append(report_text(given))
    assert want[0] != want[1]
    pair = CloudPair(cloud(0), cloud(1), duplicates=mode, **kw)
    assert report_text(pair) == want[0]
    pair = pair.with_reconst(cloud(2))
    assert report_text(pair) == want[1]
    check_pair_bookkeeping(pair, (0, 2))
    assert (pair._engine.n_iter(nat.DIR_LEFT), pair._engine.n_iter(nat.DIR_RIGHT)) == (4000, 2200)
    pair.close()


def write_xyzrgb(path, points, colours):
    with open(path, "w") as fh:
        for p, c in zip(np.asarray(points, dtype=np.float64), colours):
            fh.write(" ".join(repr(float(v)) for v in (*p, *c)) + "\n")


def test_cli_merges_what_the_files_hold(tmp_path):
    (pa, na, ca), (pb, nb, cb) = report_clouds()[0], report_clouds()[1]
    runner = CliRunner()
    common = ["--hausdorff", "--extent", "1", "1", "1"]
    # colours: the files hold bytes; the averaged colours of the restated clouds are no bytes, so those go into text files
    fa, fb, ma, mb = (str(tmp_path / f) for f in ("a.ply", "b.ply", "ma.xyzrgb", "mb.xyzrgb"))
    write_point_cloud(fa, PointCloud(pa, None, ca))
    write_point_cloud(fb, PointCloud(pb, None, cb))
    for path, (p, c) in ((ma, (pa, ca)), (mb, (pb, cb))):
        mp, _, mc, _ = merged(p, None, c, "average")
        write_xyzrgb(path, mp, mc)
    with np.errstate(divide="ignore"):
        got = runner.invoke(cli, ["--ocloud", fa, "--pcloud", fb, "--color", "ycc", "--duplicates", "average"] + common)
        want = runner.invoke(cli, ["--ocloud", ma, "--pcloud", mb, "--color", "ycc"] + common)
        kept = runner.invoke(cli, ["--ocloud", fa, "--pcloud", fb, "--color", "ycc"] + common)
    assert got.exit_code == 0 and want.exit_code == 0 and kept.exit_code == 0, (got.output, want.output)
    assert got.stdout == want.stdout and got.stdout != kept.stdout and len(got.stdout.splitlines()) > 10
    assert "2000 of 6000 rows merged away" in got.stderr and "1500 of 4500 rows merged away" in got.stderr
    assert "merged away" not in kept.stderr and "merged away" not in want.stderr
    # normals: a file holds them exactly, so the restated clouds go through the same writer
    fa, fb, ma, mb = (str(tmp_path / f) for f in ("an.ply", "bn.ply", "man.ply", "mbn.ply"))
    write_point_cloud(fa, PointCloud(pa, na))
    write_point_cloud(fb, PointCloud(pb, nb))
    for path, (p, n) in ((ma, (pa, na)), (mb, (pb, nb))):
        mp, mn, _, _ = merged(p, n, None, "average")
        write_point_cloud(path, PointCloud(mp, mn))
    d2 = ["--point-to-plane", "--normal-index", "neighbour"] + common
    with np.errstate(divide="ignore"):
        got = runner.invoke(cli, ["--ocloud", fa, "--pcloud", fb, "--pcloud", fb, "--duplicates", "average"] + d2)
        want = runner.invoke(cli, ["--ocloud", ma, "--pcloud", mb] + d2)
    assert got.exit_code == 0 and want.exit_code == 0, (got.output, want.output)
    assert got.stdout == want.stdout * 2                                # (two processed clouds: the report twice)
    assert got.stderr.count("merged away") == 3                         # the original once, every processed cloud once
