"""Carried normals on the GPU (include/pccm.h, pccm_carry_normals): ``pccm_get_normals(to)`` against the NumPy restatement of
tests/carry_reference.py fed the pair's own matched rows, compared as raw bytes (signed zeros count); the entry point's caching,
invalidation and errors; and every consumer of normals on carried ones against a pair that was GIVEN the restated normals.

Source normals are ``standard_normal * 10**uniform(-3, 3)`` per row in every family, so that the order of a sum shows in its
last bits: a kernel that adds in arrival order cannot pass."""
import functools

import numpy as np
import pytest
from click.testing import CliRunner

from carry_reference import carried_normals, carried_normals_reversed
from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import write_point_cloud
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud

pytestmark = pytest.mark.gpu


def wild_normals(rng, n):
    return rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))


def planted(seed=4):
    """133 targets on a unit lattice at z = 0; target j is the nearest one of m_j jittered source points, m = 0..130, 1000, 5000."""
    rng = np.random.default_rng(seed)
    counts = np.array(list(range(131)) + [1000, 5000])
    targets = np.array([[j % 12, j // 12, 0.0] for j in range(len(counts))], dtype=np.float32)
    src = np.repeat(targets, counts, axis=0) + rng.uniform(-0.125, 0.125, (int(counts.sum()), 3)).astype(np.float32)
    src = src[rng.permutation(len(src))].astype(np.float32)
    return src, targets, counts


@functools.lru_cache(maxsize=None)
def family(name):
    """-> (source points, target points, source normals); the carry goes source -> target."""
    rng = np.random.default_rng(0)
    if name == "uniform_20000_5000":
        src, dst = rng.random((20000, 3), dtype=np.float32), rng.random((5000, 3), dtype=np.float32)
    elif name == "uniform_5000_20000":
        src, dst = rng.random((5000, 3), dtype=np.float32), rng.random((20000, 3), dtype=np.float32)
    elif name == "three_points":
        src, dst = rng.random((20000, 3), dtype=np.float32), rng.random((3, 3), dtype=np.float32)
    elif name == "one_point":
        src, dst = rng.random((20000, 3), dtype=np.float32), rng.random((1, 3), dtype=np.float32)
    elif name == "planted":
        src, dst, _ = planted()
    elif name == "lattice":
        from test_gpu_ties_mean import lattice_pair
        a, b = lattice_pair()
        src, dst = np.asarray(a.points), np.asarray(b.points)
    elif name == "georeferenced_f64":
        base = np.array([1.0e6, 2.0e6, 3.0e6])
        src = base + rng.random((5000, 3)) * 10.0
        dst = src[rng.permutation(5000)] + rng.normal(0.0, 1e-3, (5000, 3))
    else:
        raise KeyError(name)
    return src, dst, wild_normals(rng, len(src))


@functools.lru_cache(maxsize=None)
def carried(name, frm=0):
    """One carry through the ABI: (normals the library holds for the target cloud, matched rows F, matched rows G)."""
    src, dst, nrm = family(name)
    eng = nat.Engine(0)
    try:
        eng.set_cloud(frm, src)
        eng.set_cloud(1 - frm, dst)
        eng.set_normals(frm, nrm)
        eng.nn_pair("auto")
        assert eng.carry_normals(frm) is True
        got = eng.get_normals(1 - frm)
        d_f, d_g = (nat.DIR_LEFT, nat.DIR_RIGHT) if frm == 0 else (nat.DIR_RIGHT, nat.DIR_LEFT)
        rows_f, rows_g = eng.fetch_nn(d_f, want_d2=False)[0], eng.fetch_nn(d_g, want_d2=False)[0]
    finally:
        eng.close()
    return got, rows_f.astype(np.int64), rows_g.astype(np.int64)


FAMILIES = ["uniform_20000_5000", "uniform_5000_20000", "three_points", "one_point", "planted", "lattice", "georeferenced_f64"]


@pytest.mark.parametrize("name", FAMILIES)
def test_carried_normals_equal_the_restatement_bit_for_bit(name):
    src, dst, nrm = family(name)
    got, rows_f, rows_g = carried(name)
    want = carried_normals(nrm, rows_f, rows_g, len(dst))
    bad = np.flatnonzero(np.any(got.view(np.uint64) != want.view(np.uint64), axis=1))
    counts = np.bincount(rows_f, minlength=len(dst))
    print(f"{name}: {len(dst)} targets, m = 0 / 1 / 2 / >= 3: {(counts == 0).sum()} / {(counts == 1).sum()} / {(counts == 2).sum()} / "
          f"{(counts >= 3).sum()}, longest {counts.max()}, rows that differ: {len(bad)}")
    assert got.shape == want.shape and len(bad) == 0, (bad[:8], counts[bad[:8]])
    assert got.tobytes() == want.tobytes()


def test_uniform_family_tells_the_summation_order():
    src, dst, nrm = family("uniform_20000_5000")
    got, rows_f, rows_g = carried("uniform_20000_5000")
    counts = np.bincount(rows_f, minlength=len(dst))
    assert (counts == 0).sum() > 50 and (counts == 1).sum() > 100 and (counts == 2).sum() > 100 and counts.max() > 8
    rev = carried_normals_reversed(nrm, rows_f, rows_g, len(dst))
    moved = np.any(rev.view(np.uint64) != got.view(np.uint64), axis=1)
    print("rows the reversed order moves:", int(moved.sum()), "of", int((counts >= 3).sum()), "with m >= 3")
    assert moved.sum() >= 1000 and not moved[counts < 3].any()


def test_fallback_dominates_when_the_target_is_the_larger_cloud():
    src, dst, nrm = family("uniform_5000_20000")
    got, rows_f, rows_g = carried("uniform_5000_20000")
    empty = np.bincount(rows_f, minlength=len(dst)) == 0
    assert empty.sum() > 15000
    assert got[empty].tobytes() == np.asarray(nrm, dtype=np.float64)[rows_g[empty]].tobytes()


def test_degenerate_targets_hold_long_lists():
    for name, longest in (("three_points", 3000), ("one_point", 20000)):
        _, rows_f, _ = carried(name)
        assert np.bincount(rows_f).max() >= longest


def test_planted_multiplicities_come_out_exactly_and_tell_the_order():
    src, dst, counts = planted()
    _, _, nrm = family("planted")
    got, rows_f, rows_g = carried("planted")
    assert len(src) == 14515 and np.array_equal(np.bincount(rows_f, minlength=len(dst)), counts)
    rev = carried_normals_reversed(nrm, rows_f, rows_g, len(dst))
    moved = np.any(rev.view(np.uint64) != got.view(np.uint64), axis=1)
    assert moved[counts >= 3].sum() >= 100 and not moved[counts < 3].any()


def test_lattice_family_has_exact_ties():
    from ties_reference import tie_sets
    src, dst, _ = family("lattice")
    assert max(len(s) for s in tie_sets(src, dst)[1]) > 1


def test_carry_towards_cloud_0():
    src, dst, nrm = family("uniform_20000_5000")
    got, rows_f, rows_g = carried("uniform_20000_5000", 1)           # cloud 1 holds the source, cloud 0 is the target
    assert got.tobytes() == carried_normals(nrm, rows_f, rows_g, len(dst)).tobytes()
    assert got.tobytes() == carried("uniform_20000_5000", 0)[0].tobytes()


# ---- behaviour through the ABI ------------------------------------------------------------------------------------------------
@pytest.fixture
def small():
    rng = np.random.default_rng(11)
    a, b = rng.random((3000, 3), dtype=np.float32), rng.random((1000, 3), dtype=np.float32)
    eng = nat.Engine(0)
    eng.set_cloud(0, a)
    eng.set_cloud(1, b)
    eng.set_normals(0, wild_normals(rng, 3000))
    yield eng, a, b, rng
    eng.close()


def test_second_call_builds_nothing_and_is_allowed_during_capture(small):
    eng, *_ = small
    eng.nn_pair("auto")
    assert eng.carry_normals(0) is True
    first = eng.get_normals(1)
    assert eng.carry_normals(0) is False
    eng.graph_begin()
    try:
        assert eng.carry_normals(0) is False
    finally:
        eng.graph_abort()
    eng.nn_pair("auto")                                     # (an abandoned capture invalidates the results)
    assert eng.carry_normals(0) is True                     # other search results: built again, to the same normals
    assert eng.get_normals(1).tobytes() == first.tobytes()


def test_first_build_during_capture_is_a_state_error(small):
    eng, *_ = small
    eng.nn_pair("auto")
    eng.graph_begin()
    try:
        with pytest.raises(nat.PccmStateError):
            eng.carry_normals(0)
    finally:
        eng.graph_abort()


def test_carried_normals_go_with_what_they_were_made_from(small):
    eng, a, b, rng = small
    eng.nn_pair("auto")
    eng.carry_normals(0)
    eng.set_normals(0, wild_normals(rng, 3000))             # new source normals
    with pytest.raises(nat.PccmStateError):
        eng.get_normals(1)
    assert eng.carry_normals(0) is True
    eng.set_cloud(0, a[::-1].copy())                        # new source points (its normals go too)
    with pytest.raises(nat.PccmStateError):
        eng.get_normals(1)
    eng.set_normals(0, wild_normals(rng, 3000))
    eng.nn_pair("auto")
    assert eng.carry_normals(0) is True
    eng.set_cloud(1, b[::-1].copy())                        # new target points
    with pytest.raises(nat.PccmStateError):
        eng.get_normals(1)
    eng.nn_pair("auto")
    assert eng.carry_normals(0) is True
    given = wild_normals(rng, 1000)
    eng.set_normals(1, given)                               # the target's own normals replace the carried ones
    assert eng.get_normals(1).tobytes() == given.tobytes()
    assert eng.get_normals(0).shape == (3000, 3)            # ... and the source keeps its own


def test_state_and_argument_errors(small):
    eng, a, b, rng = small
    with pytest.raises(nat.PccmStateError):                 # no search result
        eng.carry_normals(0)
    eng.nn_pair("auto")
    with pytest.raises(nat.PccmStateError):                 # cloud 1 has no normals to carry
        eng.carry_normals(1)
    with pytest.raises(ValueError):
        eng.carry_normals(2)
    eng.set_shard(0, 2)
    eng.nn_pair("auto")
    with pytest.raises(nat.PccmStateError):                 # sharded
        eng.carry_normals(0)
    eng.set_shard(0, 1)
    eng.set_ties("mean")
    eng.nn_pair("auto")
    with pytest.raises(nat.PccmStateError):                 # PCCM_TIES_MEAN
        eng.carry_normals(0)
    eng.set_ties("pick")
    eng.nn_pair("auto")
    assert eng.carry_normals(0) is True


def test_searches_without_matched_rows_are_repeated(small):
    eng, a, b, rng = small
    eng.nn_want_idx(False)
    eng.nn_pair("auto")
    assert eng.carry_normals(0) is True
    got = eng.get_normals(1)
    rows_f, rows_g = eng.fetch_nn(nat.DIR_LEFT, want_d2=False)[0], eng.fetch_nn(nat.DIR_RIGHT, want_d2=False)[0]
    assert got.tobytes() == carried_normals(eng_normals(eng), rows_f, rows_g, len(b)).tobytes()


def eng_normals(eng):
    return eng.get_normals(0)


# ---- every consumer at once ---------------------------------------------------------------------------------------------------
OPTIONS = dict(color=None, hausdorff=True, point_to_plane=True, plane_to_plane=True, point_ssim=("normal",), hausdorff_rank=(0.9,))


def report(pair):
    with np.errstate(divide="ignore", invalid="ignore"):
        res = MetricCalculator(pair).calculate(transform_options(CalculateOptions(**OPTIONS))).as_dict()
    return {k: np.asarray(v, dtype=np.float64).tobytes() for k, v in res.items()}


def restated_cloud(name):
    src, dst, nrm = family(name)
    _, rows_f, rows_g = carried(name)
    return PointCloud(dst, carried_normals(nrm, rows_f, rows_g, len(dst)))


@pytest.mark.parametrize("name", ["uniform_20000_5000", "planted"])
@pytest.mark.parametrize("use_graph", [False, True])
def test_reports_on_carried_normals_equal_reports_on_given_ones(name, use_graph):
    src, dst, nrm = family(name)
    extent = [12.0, 12.0, 1.0]
    with CloudPair(PointCloud(src, nrm), restated_cloud(name), normal_index="neighbour", extent=extent) as given:
        want = report(given)
    assert len(want) > 20
    with CloudPair(PointCloud(src, nrm), PointCloud(dst), normal_index="neighbour", extent=extent, carry_normals=True,
                   use_graph=use_graph) as pair:
        for _ in range(4 if use_graph else 1):              # eager, capture, replays
            got = report(pair)
            assert list(got) == list(want)
            assert [k for k in want if got[k] != want[k]] == []
            pair.recompute()
        assert pair._carried == [False, True] and pair._estimated == [False, False]
        assert not use_graph or pair._graph_id is not None


def test_with_reconst_carries_to_every_decoded_cloud():
    src, dst, nrm = family("uniform_20000_5000")
    dst2 = np.random.default_rng(21).random((4000, 3), dtype=np.float32)
    fresh = []
    for d in (dst, dst2):
        with CloudPair(PointCloud(src, nrm), PointCloud(d), normal_index="neighbour", extent=[1, 1, 1], carry_normals=True) as p:
            fresh.append(report(p))
    assert fresh[0] != fresh[1]
    pair = CloudPair(PointCloud(src, nrm), PointCloud(dst), normal_index="neighbour", extent=[1, 1, 1], carry_normals=True)
    assert report(pair) == fresh[0]
    pair = pair.with_reconst(PointCloud(dst2))
    assert report(pair) == fresh[1]
    assert pair._carried == [False, True]
    pair.close()


def test_cli_prints_the_in_process_report(tmp_path):
    src, dst, nrm = family("uniform_20000_5000")
    nrm32 = nrm.astype(np.float32)                           # (what the file holds)
    pa, pb = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    write_point_cloud(pa, PointCloud(src, nrm32))
    write_point_cloud(pb, PointCloud(dst))
    args = ["--ocloud", pa, "--pcloud", pb, "--hausdorff", "--point-to-plane", "--normal-index", "neighbour", "--carry-normals",
            "--extent", "1", "1", "1"]
    with np.errstate(divide="ignore"):
        out = CliRunner().invoke(cli, args)
        assert out.exit_code == 0, out.output
        with CloudPair(PointCloud(src, nrm32), PointCloud(dst), normal_index="neighbour", extent=[1.0, 1.0, 1.0], carry_normals=True) as p:
            text = MetricCalculator(p).calculate(transform_options(CalculateOptions(None, True, True))).as_df().to_string()
        with CloudPair(PointCloud(src, nrm32), PointCloud(dst), normal_index="neighbour", extent=[1.0, 1.0, 1.0]) as p:
            estimated = MetricCalculator(p).calculate(transform_options(CalculateOptions(None, True, True))).as_df().to_string()
    assert out.output == text + "\n"
    assert text != estimated                                 # the flag changes the decoded cloud's normals, hence the D2 rows
