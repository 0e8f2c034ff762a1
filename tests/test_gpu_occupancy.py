"""Voxel occupancy on the GPU (include/pccm.h, pccm_voxel_occupancy): the three counts of every case EQUAL the NumPy statement of
tests/occupancy_reference.py -- integers compared with ==, report rows with == on float64 -- and, for the planted families, the
triple each was built to have.  Ragged sizes on a full table, the one contended voxel, every point its own voxel, the boundary
arithmetic that tells a division from a multiplication by the reciprocal, several voxel sizes in one call, the way through
CloudPair, the calculator and the command line (graph replay, ``duplicates=``, ``transform=``), the entry point's errors, and the
merge of duplicates -- whose kernels the occupancy mode shares -- unharmed."""
import ctypes
import functools

import numpy as np
import pytest
from click.testing import CliRunner

import occupancy_reference as ref
from merge_reference import drawn_20000, merged
from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import write_point_cloud
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud

pytestmark = pytest.mark.gpu


def counted(a, b, voxels):
    """The triples of ``voxels`` for clouds a and b through the ABI, on a context of its own."""
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, a)
        eng.set_cloud(1, b)
        got = eng.voxel_occupancy(voxels)
        eng.sync()
    finally:
        eng.close()
    return got


@functools.lru_cache(maxsize=None)
def wanted(kind, *key):
    """The reference's triple of a ragged pair or a planted family, computed once."""
    a, b, voxel = ref.ragged(*key) if kind == "ragged" else ref.planted(*key)[:3]
    return ref.occupancy(a, b, voxel)


# ---- the counts through the ABI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n1, n2", ref.RAGGED)
def test_ragged_sizes_equal_the_reference(n1, n2, dtype):
    a, b, voxel = ref.ragged(n1, n2, dtype)
    want = wanted("ragged", n1, n2, dtype)
    got = counted(a, b, [voxel])
    print(f"{n1} + {n2} rows ({dtype}), voxel {voxel}: GPU {got[0]}, reference {want}")
    assert got == [want]
    assert all(type(c) is int for c in got[0])


@pytest.mark.parametrize("name", ref.PLANTED)
def test_planted_families_have_the_triples_they_were_built_with(name):
    a, b, voxel, built = ref.planted(name)
    got = counted(a, b, [voxel])
    print(f"{name}: GPU {got[0]}, built {built}, reference {wanted('planted', name)}")
    assert got == [built] and built == wanted("planted", name)
    assert counted(b, a, [voxel]) == [(built[1], built[0], built[2])]              # the clouds the other way round


def test_boundary_counts_are_the_division_s_and_not_the_reciprocal_s():
    for name in ref.BOUNDARY:
        a, b, voxel, built = ref.planted(name)
        wrong = ref.occupancy_by_reciprocal(a, b, voxel)
        got = counted(a, b, [voxel])[0]
        print(f"{name}: GPU {got}, division {built}, reciprocal {wrong}")
        assert got == built and got != wrong


def test_four_voxel_sizes_in_one_call_equal_four_calls():
    a, b, _ = ref.ragged(1000, 777, "float64")
    sizes = [0.2, 0.05, 0.4, 0.1]                                                 # out of order
    together = counted(a, b, sizes)
    assert together == [counted(a, b, [v])[0] for v in sizes]
    assert together == [ref.occupancy(a, b, v) for v in sizes]
    assert counted(a, b, [0.1, 0.1, 0.4, 0.1]) == [together[3], together[3], together[2], together[3]]     # a size may repeat
    assert len(set(together)) == 4


# ---- through CloudPair, the calculator and the command line --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def report_clouds():
    """A pair of 3000 and 2500 points in the unit cube, the second a noisy part of the first, with normals."""
    rng = np.random.default_rng(41)
    a = rng.random((3000, 3), dtype=np.float32)
    b = (a[300:2800] + rng.normal(0, 0.01, (2500, 3))).astype(np.float32)
    return a, b, rng.standard_normal((3000, 3)), rng.standard_normal((2500, 3))


BASE = dict(hausdorff=True, point_to_plane=True, fscore=(0.05,), chamfer=True, dcd=(40.0,))
SIZES = (0.25, 0.0625, 0.5, 0.25)                                                # out of order, one of them twice


def report(pair, **more):
    with np.errstate(divide="ignore", invalid="ignore"):
        return MetricCalculator(pair).calculate(transform_options(CalculateOptions(**{**BASE, **more}))).as_dict()


def reference_rows(a, b, sizes):
    want = {}
    for v in sorted(set(sizes)):
        want.update(ref.rows(ref.occupancy(a, b, v), v))
    return want


def same_bits(x, y):
    return np.float64(x).tobytes() == np.float64(y).tobytes()


class CountedCalls:
    """Counts the pccm_voxel_occupancy calls an engine object makes (the engine is pooled: the wrapper comes off again)."""
    def __init__(self, engine):
        self.engine, self.calls = engine, []
        inner = engine.voxel_occupancy

        def voxel_occupancy(voxels):
            self.calls.append(list(voxels))
            return inner(voxels)
        engine.voxel_occupancy = voxel_occupancy

    def remove(self):
        del self.engine.voxel_occupancy


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_report_rows_equal_the_reference_and_leave_the_others_alone(use_graph):
    a, b, na, nb = report_clouds()
    kw = dict(extent=[1.0, 1.0, 1.0], normal_index="neighbour", use_graph=use_graph)
    with CloudPair(PointCloud(a, na), PointCloud(b, nb), **kw) as plain:
        base = report(plain)
    want = reference_rows(a, b, SIZES)
    with CloudPair(PointCloud(a, na), PointCloud(b, nb), **kw) as pair:
        watch = CountedCalls(pair._engine)
        try:
            for step in range(4 if use_graph else 2):                            # eager, (capture, replays)
                got = report(pair, occupancy=SIZES)
                assert list(got)[:len(base)] == list(base) and list(got)[len(base):] == list(want)
                for key, value in base.items():                                  # every other row: bit-identical
                    assert same_bits(got[key], value), key
                for key, value in want.items():
                    assert got[key] == value and type(got[key]) is np.float64, (key, got[key], value)
                assert watch.calls == [[0.0625, 0.25, 0.5]]                      # ONE call for the report, none for a later one
                pair.recompute()
            assert not use_graph or pair._graph_id is not None
            assert pair.voxel_occupancy(0.25) == ref.occupancy(a, b, 0.25) and len(watch.calls) == 1
            assert pair.voxel_occupancy(0.125) == ref.occupancy(a, b, 0.125) and watch.calls[1:] == [[0.125]]
        finally:
            watch.remove()


def test_duplicates_do_not_change_the_counts_and_a_shift_by_whole_voxels_moves_them():
    rng = np.random.default_rng(43)
    # coordinates on a 2^-10 lattice in [0, 8): a shift by 4.0 -- eight voxels of 0.5 -- is exact in fp64
    uniq_a, uniq_b = (rng.integers(0, 8 * 1024, (n, 3)) / 1024.0 for n in (2000, 1500))
    a = np.concatenate([uniq_a, uniq_a[rng.integers(0, 2000, 700)]])[rng.permutation(2700)]
    b = np.concatenate([uniq_b, uniq_b[rng.integers(0, 1500, 400)]])[rng.permutation(1900)]
    want = ref.occupancy(a, b, 0.5)
    assert want == ref.occupancy(uniq_a, uniq_b, 0.5)
    with CloudPair(PointCloud(a), PointCloud(b), extent=[8.0, 8.0, 8.0]) as kept:
        assert kept.voxel_occupancy(0.5) == want and kept.duplicates_removed == (0, 0)
    with CloudPair(PointCloud(a), PointCloud(b), extent=[8.0, 8.0, 8.0], duplicates="drop") as dropped:
        assert dropped.duplicates_removed[0] > 0 and dropped.duplicates_removed[1] > 0
        assert dropped.voxel_occupancy(0.5) == want
    shift = np.eye(4)
    shift[:3, 3] = [4.0, -4.0, 0.0]
    moved = ref.occupancy(a, b + shift[:3, 3], 0.5)
    assert moved != want and moved[:2] == want[:2]                               # the same voxels per cloud, other ones shared
    with CloudPair(PointCloud(a), PointCloud(b), extent=[8.0, 8.0, 8.0], normal_index="neighbour", transform=shift) as pair:
        assert pair.voxel_occupancy(0.5) == moved
        rows = report(pair, occupancy=0.5)
        for key, value in ref.rows(moved, 0.5).items():
            assert rows[key] == value, key


def test_cli_rows_equal_the_reference(tmp_path):
    a, b, _, _ = report_clouds()
    fa, fb = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    write_point_cloud(fa, PointCloud(a[:800]))
    write_point_cloud(fb, PointCloud(b[:600]))
    common = ["--ocloud", fa, "--pcloud", fb, "--extent", "1", "1", "1", "--csv"]
    with np.errstate(divide="ignore"):
        got = CliRunner().invoke(cli, common + ["--occupancy", "0.25", "--occupancy", "0.0625", "--occupancy", "0.25"])
        plain = CliRunner().invoke(cli, common)
    assert got.exit_code == 0 and plain.exit_code == 0, (got.output, got.exception)
    lines, before = ([line for line in out.stdout.splitlines() if line] for out in (got, plain))    # (print ends the csv with a blank line)
    assert lines[:len(before)] == before and len(lines) == len(before) + 10       # the other rows as they were, then five per size
    want = reference_rows(a[:800].astype(np.float64), b[:600].astype(np.float64), (0.0625, 0.25))
    for line, (key, value) in zip(lines[len(before):], want.items()):
        _, label, is_left, _, text = line.split(",")
        assert label == f"{key[0]}[{key[-1]!r}]" and is_left == (str(key[1]) if len(key) == 3 else "")
        assert np.float64(text) == value, (line, value)


# ---- the entry point's errors --------------------------------------------------------------------------------------------------
@pytest.fixture
def small():
    a, b, _ = ref.ragged(300, 200)
    eng = nat.Engine(0)
    eng.set_cloud(0, a)
    eng.set_cloud(1, b)
    yield eng, a, b
    eng.close()


def test_argument_errors(small):
    eng, a, b = small
    want = ref.occupancy(a, b, 0.05)
    for sizes in ([], [1.0] * 5, [0.0], [-0.0], [-1.0], [float("nan")], [float("inf")], [-float("inf")], [0.05, 0.0], [1.0, 2.0, 3.0, float("nan")]):
        with pytest.raises(ValueError):
            eng.voxel_occupancy(sizes)
    lib, ctx = eng._lib, eng._ctx
    one = (ctypes.c_double * 1)(0.05)
    out = (ctypes.c_int64 * 3)()
    assert lib.pccm_voxel_occupancy(ctx, 1, None, out) == nat.E_ARG               # null pointers
    assert lib.pccm_voxel_occupancy(ctx, 1, one, None) == nat.E_ARG
    assert b"null" in lib.pccm_last_error()
    assert lib.pccm_voxel_occupancy(ctx, 1, one, out) == nat.OK and tuple(out) == want
    assert eng.voxel_occupancy([0.05]) == [want]                                  # nothing was left behind by the refusals


def test_state_errors(small):
    eng, a, b = small
    want = ref.occupancy(a, b, 0.05)
    fresh = nat.Engine(0)
    try:
        with pytest.raises(nat.PccmStateError, match="cloud 0 is not set"):
            fresh.voxel_occupancy([1.0])
        fresh.set_cloud(0, a)
        with pytest.raises(nat.PccmStateError, match="cloud 1 is not set"):
            fresh.voxel_occupancy([1.0])
    finally:
        fresh.close()
    eng.set_shard(0, 2)
    with pytest.raises(nat.PccmStateError, match="whole clouds on this GPU"):     # sharded
        eng.voxel_occupancy([0.05])
    eng.set_shard(0, 1)
    eng.graph_begin()
    try:
        with pytest.raises(nat.PccmStateError):                                  # between graph_begin and graph_end
            eng.voxel_occupancy([0.05])
    finally:
        eng.graph_abort()
    eng.set_ties("mean")                                                          # the tie policy does not matter
    assert eng.voxel_occupancy([0.05]) == [want]


# ---- the merge of duplicates, whose kernels the occupancy mode shares ----------------------------------------------------------
def test_merging_duplicates_is_unharmed_by_occupancy_calls():
    pts, col = drawn_20000()
    other = np.random.default_rng(9).random((3000, 3), dtype=np.float32)
    want_p, _, want_c, want_m = merged(pts, None, col, "average")
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, pts)
        eng.set_cloud(1, other)
        eng.set_colors(0, col)
        before = eng.voxel_occupancy([0.1, 0.01])
        assert before == [ref.occupancy(pts, other, v) for v in (0.1, 0.01)]
        n_new = eng.merge_duplicates(0, "average")                                # the shared kernels, in their own mode again
        assert n_new == len(want_p) < len(pts)
        assert eng.get_merge_map(0).tobytes() == want_m.tobytes()
        after = eng.voxel_occupancy([0.1, 0.01])                                  # merged rows occupy the voxels the given rows did
        assert after == before
        # ... and the occupancy workspace is not the merge's: the merged cloud, its colours and the map are what they were
        assert eng.get_points(0).tobytes() == want_p.tobytes() and eng.get_colors(0).tobytes() == want_c.tobytes()
        assert eng.get_merge_map(0).tobytes() == want_m.tobytes()
        assert eng.merge_duplicates(0, "average") == n_new                        # nothing left to merge, nothing changes
        assert eng.get_merge_map(0).tobytes() == want_m.tobytes()
        eng.sync()
    finally:
        eng.close()
