"""Host-side contract of the voxel-occupancy rows (CalculateOptions(occupancy=...)): option validation, row order, labels, keys and
dependencies, the default report untouched, the metrics' arithmetic on planted triples through a stand-in pair, the NumPy
restatement against the families' constructed triples (and against what a reciprocal multiplication would count), the checks that
run before any GPU work, the command line's usage errors, and the workspace layout.  No GPU needed."""
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from click.testing import CliRunner

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import CalculateResult, MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import write_point_cloud
from open_pcc_metric_amd.options import MAX_OCCUPANCY_VOXELS, CalculateOptions, check_occupancy, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import occupancy_reference as ref  # noqa: E402
from conftest import load_golden  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def same(x, y):
    return np.float64(x).tobytes() == np.float64(y).tobytes()


def keys(opts):
    return [m._key() for m in transform_options(opts)]


# ---- options -----------------------------------------------------------------------------------------------------------------
def test_options_are_normalised():
    assert MAX_OCCUPANCY_VOXELS == 4 and nat.MAX_OCCUPANCY == 4
    assert CalculateOptions().occupancy == () and CalculateOptions(occupancy=None).occupancy == ()
    assert CalculateOptions(occupancy=()).occupancy == () and CalculateOptions(occupancy=[]).occupancy == ()
    assert CalculateOptions(occupancy=2).occupancy == (2.0,)
    assert CalculateOptions(occupancy=[4, 0.5, 4.0, np.float64(16)]).occupancy == (0.5, 4.0, 16.0)            # duplicates, unsorted
    assert CalculateOptions(occupancy=(v for v in (2.0, 0.25))).occupancy == (0.25, 2.0)
    assert CalculateOptions(occupancy=[1e-300, 1e300]).occupancy == (1e-300, 1e300)
    assert all(type(v) is float for v in CalculateOptions(occupancy=[np.float32(0.5), 1]).occupancy)
    assert CalculateOptions(occupancy=[1, 2, 3, 4, 1]).occupancy == (1.0, 2.0, 3.0, 4.0)                      # four DISTINCT sizes
    assert CalculateOptions(fscore=0.5, dcd=40, occupancy=0.25).fscore == (0.5,)                              # each keeps its own


@pytest.mark.parametrize("bad", [True, False, np.True_, float("nan"), float("inf"), -float("inf"), 0, 0.0, -0.0, -0.5, -1e-300, "2",
                                 b"1", [2, "x"], [None], [1, 2, 3, 4, 5], [2, True], [1, float("nan")], [1, 0], object()])
def test_bad_voxel_sizes_raise(bad):
    with pytest.raises(ValueError, match="occupancy"):
        CalculateOptions(occupancy=bad)
    with pytest.raises(ValueError, match="occupancy"):
        CalculateOptions(None, True, True, chamfer=True, fscore=0.5, dcd=40, align="icp", occupancy=bad)


def expected_keys(voxels):
    out = []
    for v in sorted(set(float(v) for v in voxels)):
        out += list(ref.rows((1, 1, 1), v))
    return out


@pytest.mark.parametrize("voxels", [(2.0,), (4, 0.5, 1), (1e-3, 1, 2, 1024.0)], ids=["one", "three", "four"])
@pytest.mark.parametrize("align, dcd, fscore", list(itertools.product([None, "icp"], [None, (40.0, 5.0)], [None, (0.01,)])))
def test_rows_follow_every_existing_row(voxels, align, dcd, fscore):
    extra = dict(align=align, dcd=dcd, fscore=fscore, chamfer=bool(dcd), truncate=(0.5,) if fscore else None)
    for color, hd, p2plane in itertools.product([None, "ycc"], [False, True], [False, True]):
        base = keys(CalculateOptions(color, hd, p2plane, **extra))
        opts = CalculateOptions(color, hd, p2plane, occupancy=voxels, **extra)
        got = keys(opts)
        assert got[:len(base)] == base                            # every other row, alignment rows included, where it was
        assert got[len(base):] == expected_keys(voxels)
        assert len(got) - len(base) == 5 * len(voxels)
    if align is not None:
        assert base[-2:] == [("AlignmentFitness",), ("AlignmentRMSE",)]
    metrics = transform_options(opts)[len(base):]
    for m in metrics:
        m.value = 0.5
    df = CalculateResult(metrics).as_df()
    labels, sides = [], []
    for v in sorted(voxels):
        tag = f"[{float(v)!r}]"
        labels += ["OccupiedVoxels" + tag] * 2 + ["VoxelCoverage" + tag] * 2 + ["VoxelIoU" + tag]
        sides += [True, False, True, False, ""]
    assert list(df["label"]) == labels
    assert list(df["is_left"]) == sides and list(df["point-to-plane"]) == [""] * len(labels)
    assert not any("symmetric" in label for label in labels)      # (as for the F-score: the IoU is the symmetric row)


def test_without_the_option_the_rows_are_todays():
    for color, hd, p2plane in itertools.product([None, "ycc"], [False, True], [False, True]):
        base = keys(CalculateOptions(color, hd, p2plane))
        assert keys(CalculateOptions(color, hd, p2plane, occupancy=None)) == base
        assert keys(CalculateOptions(color, hd, p2plane, occupancy=())) == base
        assert not any("Voxel" in str(k) for k in base)
    assert len(keys(CalculateOptions("ycc", True, True))) == 32


def test_dependencies_and_keys():
    from open_pcc_metric_amd.metric import (DirectionalMetric, OccupiedVoxels, PrimaryMetric, SecondaryMetric, VoxelCounts, VoxelCoverage,
                                            VoxelIoU)
    import open_pcc_metric.metric as alias
    import open_pcc_metric.options as alias_options
    assert alias.VoxelIoU is VoxelIoU and alias.VoxelCounts is VoxelCounts and alias.OccupiedVoxels is OccupiedVoxels
    assert alias.VoxelCoverage is VoxelCoverage
    assert alias_options.CalculateOptions(occupancy=[2, 1]).occupancy == (1.0, 2.0)
    assert VoxelCounts(2)._key() == ("VoxelCounts", 2.0)
    assert OccupiedVoxels(True, 2)._key() == ("OccupiedVoxels", True, 2.0)
    assert VoxelCoverage(False, 0.5)._key() == ("VoxelCoverage", False, 0.5)
    assert VoxelIoU(4)._key() == ("VoxelIoU", 4.0)
    assert issubclass(VoxelCounts, PrimaryMetric) and VoxelCounts._pccm_waits is True
    for cls in (OccupiedVoxels, VoxelCoverage):
        assert issubclass(cls, SecondaryMetric) and issubclass(cls, DirectionalMetric)
    assert issubclass(VoxelIoU, SecondaryMetric) and not issubclass(VoxelIoU, DirectionalMetric)
    assert VoxelCounts(0.25)._pccm_request() == ("occupancy", 0.25)
    for m in (OccupiedVoxels(True, 0.25), VoxelCoverage(False, 0.25), VoxelIoU(0.25)):
        assert [d._key() for d in m._get_dependencies().values()] == [("VoxelCounts", 0.25)]
        assert m._pccm_request() is None
    assert "pccm_voxel_occupancy" in nat.SYMBOLS
    header = open(os.path.join(ROOT, "include", "pccm.h")).read()
    assert "int pccm_voxel_occupancy(pccm_ctx *ctx, int n, const double *voxels, int64_t *out);" in header


def test_the_calculator_tells_the_pair_about_occupancy_rows():
    class Recorder:
        def __init__(self):
            self.wanted = None

        def prefetch_reductions(self, wanted):
            self.wanted = list(wanted)

    pair = Recorder()
    MetricCalculator(pair)._plan(transform_options(CalculateOptions(occupancy=(4, 0.5))))
    assert sorted(w for w in pair.wanted if w[0] == "occupancy") == [("occupancy", 0.5), ("occupancy", 4.0)]
    pair = Recorder()
    MetricCalculator(pair)._plan(transform_options(CalculateOptions()))
    assert not any(isinstance(w, tuple) and w[0] == "occupancy" for w in pair.wanted)
    from open_pcc_metric_amd.cloud_pair import _FAMILIES, _GROUP, _by_family
    assert _GROUP["occupancy"] == "occupancy" and "occupancy" not in _FAMILIES      # (prepared eagerly, nothing is enqueued)
    assert _by_family([("occupancy", 2.0), (True, False), "boundary"]) == {"occupancy": [("occupancy", 2.0)],
                                                                           "column": [(True, False), "boundary"]}


# ---- the metrics' arithmetic through a stand-in pair ---------------------------------------------------------------------------
class StandIn:
    """A pair whose getters return plain ndarrays and whose voxel counts are planted."""
    def __init__(self, triples):
        self.triples = dict(triples)
        self.asked = []

    def voxel_occupancy(self, voxel):
        self.asked.append(voxel)
        return self.triples[voxel]

    def get_left_neighbour_distances(self):
        return np.array([0.25, 1.0, 4.0])

    def get_right_neighbour_distances(self):
        return np.array([1.0, 0.0625])

    def get_boundary_sqrt_distances(self):
        return np.array([0.5, 1.0])

    def get_extent(self):
        return np.array([1.0, 2.0, 3.0])


def test_rows_from_planted_triples():
    triples = {0.5: (7, 5, 0),                    # nothing shared
               1.0: (120, 120, 120),              # the same voxels: IoU exactly 1
               2.0: (3, 1000003, 2),
               1024.0: (2 ** 40 + 1, 2 ** 40 + 3, 2 ** 40)}
    pair = StandIn(triples)
    with np.errstate(divide="ignore"):
        res = MetricCalculator(pair).calculate(transform_options(CalculateOptions(occupancy=list(triples)))).as_dict()
    assert sorted(pair.asked) == sorted(triples)                   # one read per size, whatever the number of rows on it
    tail = list(res)[-20:]
    want = {}
    for v in sorted(triples):
        want.update(ref.rows(triples[v], v))
    assert tail == list(want)
    for key, value in want.items():
        assert same(res[key], value) and type(res[key]) is np.float64, key
    assert same(res[("VoxelIoU", 0.5)], 0.0) and same(res[("VoxelCoverage", True, 0.5)], 0.0) and same(res[("VoxelCoverage", False, 0.5)], 0.0)
    assert same(res[("VoxelIoU", 1.0)], 1.0) and same(res[("VoxelCoverage", True, 1.0)], 1.0) and same(res[("VoxelCoverage", False, 1.0)], 1.0)
    assert same(res[("OccupiedVoxels", True, 2.0)], 3.0) and same(res[("OccupiedVoxels", False, 2.0)], 1000003.0)
    assert same(res[("VoxelCoverage", True, 2.0)], np.float64(2) / np.float64(3))          # recall: of the original's voxels
    assert same(res[("VoxelCoverage", False, 2.0)], np.float64(2) / np.float64(1000003))   # precision: of the processed cloud's
    assert same(res[("VoxelIoU", 2.0)], np.float64(2) / np.float64(1000004))
    assert same(res[("VoxelIoU", 1024.0)], np.float64(2 ** 40) / np.float64(2 ** 40 + 4))  # (the union is formed in integers)


# ---- the restatement against the constructed triples ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.PLANTED)
def test_the_restatement_counts_what_the_families_were_built_to_have(name):
    a, b, voxel, want = ref.planted(name)
    assert ref.occupancy(a, b, voxel) == want
    assert ref.occupancy(b, a, voxel) == (want[1], want[0], want[2])
    assert ref.exact_occupancy(a, b, voxel) == want
    assert ref.occupancy(a.astype(np.float64)[::-1], b, voxel) == want                     # (no order in it)


def test_families_are_what_they_claim():
    assert ref.planted("one_voxel")[3] == (1, 1, 1) and len(ref.planted("one_voxel")[0]) == 1000 == len(ref.planted("one_voxel")[1])
    assert ref.planted("subset")[3] == (125, 210, 125) and ref.planted("disjoint")[3] == (125, 125, 0)
    a, b, _, want = ref.planted("multiplicities")
    assert want == (120, 120, 120) and len(a) == 360 and len(b) != len(a) and len(b) > 120
    a, b, _, _ = ref.planted("boundary_tenths")
    assert np.signbit(a[:, 1]).any() and not np.signbit(a[:, 1]).all() and np.signbit(b[:, 2]).any() and (a[:, 0] < 0).any()
    assert (a[:, 0] != b[:, 0]).any()                                                     # k * 0.1 is not k / 10 for every k
    a, b, voxel, _ = ref.planted("boundary_far")
    assert np.abs(a[:, 0]).min() >= 1e9 and (a[:, 0] < 0).any() and np.floor(a[:, 0] / voxel).max() > 2.0 ** 31
    assert ref.exact_voxel(0.3, 0.1) == 2 and np.floor(np.float64(0.3) * (np.float64(1) / np.float64(0.1))) == 3.0
    assert ref.exact_voxel(-0.0, 0.1) == 0 and ref.exact_voxel(-1e-300, 1.0) == -1


@pytest.mark.parametrize("name", ref.BOUNDARY)
def test_boundary_families_tell_division_from_reciprocal_multiplication(name):
    a, b, voxel, want = ref.planted(name)
    wrong = ref.occupancy_by_reciprocal(a, b, voxel)
    print(name, "division", want, "reciprocal", wrong)
    assert wrong != want
    # ... and both clouds on their own already disagree row by row, not just in the totals
    q, p = np.floor(a / voxel), np.floor(a * (np.float64(1.0) / np.float64(voxel)))
    assert (q != p).any()


@pytest.mark.parametrize("n1, n2", ref.RAGGED)
def test_ragged_pairs_fill_their_tables(n1, n2):
    for dtype in ("float32", "float64"):
        a, b, voxel = ref.ragged(n1, n2, dtype)
        assert a.shape == (n1, 3) and b.shape == (n2, 3) and a.dtype == np.dtype(dtype)
        n_a, n_b, n_ab = ref.occupancy(a, b, voxel)
        assert 1 <= n_a <= n1 and 1 <= n_b <= n2 and 0 <= n_ab <= min(n_a, n_b)
        if n1 + n2 > 100:
            assert n_a + n_b - n_ab > (n1 + n2) // 2 and n_ab > 0                          # many voxels, some of them shared


# ---- checks before any GPU work ------------------------------------------------------------------------------------------------
def golden_pair(name, **kw):
    g = load_golden(name)
    pair = CloudPair(PointCloud(g["a"], g["na"]), PointCloud(g["b"], g["nb"]), extent=list(g["extent"]), _engine=OracleEngine(), **kw)
    return g, pair


def test_sharded_pairs_are_refused_before_the_engine_is_touched():
    check_occupancy(CalculateOptions(), group=object())            # no such rows: nothing to check
    check_occupancy(CalculateOptions(occupancy=2))
    check_occupancy(CalculateOptions(occupancy=2), group=None)
    with pytest.raises(ValueError, match="sharded"):
        check_occupancy(CalculateOptions(occupancy=2), group=object())
    _, pair = golden_pair("uniform_300_color")

    class Peers:                                                  # what Collective(group) says of a group with two ranks
        sharded, group, rank, world = True, object(), 0, 2
    whole = pair._coll
    pair._coll = Peers()
    calls = list(pair._engine.calls)
    with pytest.raises(ValueError, match="sharded"):
        MetricCalculator(pair).calculate(transform_options(CalculateOptions(occupancy=2)))
    with pytest.raises(ValueError, match="sharded"):
        pair.voxel_occupancy(2.0)
    assert pair._engine.calls == calls
    pair._coll = whole
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, np.True_, "2", b"2", None, [2.0], object()):
        with pytest.raises(ValueError):
            pair.voxel_occupancy(bad)
    assert not hasattr(OracleEngine, "voxel_occupancy")
    with pytest.raises(ValueError, match="engine"):                # no quiet host fall-back: the count is the GPU's
        pair.voxel_occupancy(2.0)
    assert pair._engine.calls == calls


def test_a_pair_keeps_its_counts_and_asks_once_per_report():
    _, pair = golden_pair("uniform_300_color")

    class Counting:
        calls = []

        def voxel_occupancy(self, voxels):
            self.calls.append(list(voxels))
            return [(3, 4, int(v)) for v in voxels]
    counting = Counting()
    pair._engine.voxel_occupancy = counting.voxel_occupancy
    try:
        with np.errstate(divide="ignore"):
            res = MetricCalculator(pair).calculate(transform_options(CalculateOptions(occupancy=(2, 1, 3)))).as_dict()
        assert counting.calls == [[1.0, 2.0, 3.0]]                # every size of the report in ONE engine call
        assert same(res[("VoxelIoU", 2.0)], np.float64(2) / np.float64(5))
        assert pair.voxel_occupancy(2) == (3, 4, 2) and all(type(c) is int for c in pair.voxel_occupancy(2))
        with np.errstate(divide="ignore"):
            MetricCalculator(pair).calculate(transform_options(CalculateOptions(occupancy=(3, 4))))
        assert counting.calls == [[1.0, 2.0, 3.0], [4.0]]         # only what the pair does not hold yet
        pair.recompute()                                          # (the searches run again on the same resident points)
        assert pair.voxel_occupancy(4.0) == (3, 4, 4) and len(counting.calls) == 2
    finally:
        del pair._engine.voxel_occupancy


def test_cli_refuses_a_bad_voxel_size_before_any_context(tmp_path, monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a GPU context was asked for")
    monkeypatch.setattr(nat, "acquire_engine", no_context)
    monkeypatch.setattr(nat, "Engine", no_context)
    rng = np.random.default_rng(0)
    pa, pb = str(tmp_path / "a.xyz"), str(tmp_path / "b.xyz")
    write_point_cloud(pa, PointCloud(rng.random((20, 3))))
    write_point_cloud(pb, PointCloud(rng.random((20, 3))))
    for extra in (["--occupancy", "0"], ["--occupancy", "-0.1"], ["--occupancy", "nan"], ["--occupancy", "inf"], ["--occupancy", "x"],
                  ["--occupancy"], sum((["--occupancy", str(v)] for v in (1, 2, 3, 4, 5)), [])):
        out = CliRunner().invoke(cli, ["--ocloud", pa, "--pcloud", pb] + extra)
        assert out.exit_code == 2, (extra, out.output, out.exception)
    # (nothing was read either: the files of a refused call need not exist)
    out = CliRunner().invoke(cli, ["--ocloud", str(tmp_path / "none.ply"), "--pcloud", pb, "--occupancy", "2", "--occupancy", "-1"])
    assert out.exit_code == 2, (out.output, out.exception)
    out = CliRunner().invoke(cli, ["--help"])
    assert out.exit_code == 0 and "--occupancy" in out.output and "VOXEL" in out.output


# ---- the workspace layout ------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
def test_the_workspace_layout_holds_for_small_ragged_and_largest_sizes(tmp_path):
    exe = str(tmp_path / "occupancy_layout_host")
    build = subprocess.run(
        [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "open_pcc_metric_amd", "csrc"),
         os.path.join(ROOT, "tests", "occupancy_layout_host_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    lines = run.stdout.splitlines()
    assert len(lines) == 25 + 3 + 1 and lines[-1] == "kOccupancyMax 4"
    for line in lines[:-1]:
        head, tail = line.split(": ")
        f, g = head.split(), tail.split()
        n1, n2, cap, seen, tally, words = int(f[1]), int(f[3]), int(g[1]), int(g[3]), int(g[5]), int(g[7])
        assert g[8] == "ok", line
        assert cap >= max(64, 2 * (n1 + n2)) and cap & (cap - 1) == 0 and (cap == 64 or cap < 4 * (n1 + n2))
        assert seen == cap and seen + n1 <= tally <= seen + n1 + 1 and tally % 2 == 0 and words == tally + 6
    assert lines[0].startswith("n1 1 n2 1: cap 64 ") and "n1 2147483647 n2 2147483647: cap 8589934592 " in lines[25]
