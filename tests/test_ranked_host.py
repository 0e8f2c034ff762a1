"""Host-side contract of the ranked (generalized) Hausdorff rows (CalculateOptions(hausdorff_rank=...)): the nearest-rank index,
option validation, row order, labels and keys, the default report untouched, the metric nodes over plain arrays, the fallback
of an engine without the selection call, and the checks that run before any GPU work.  No GPU needed."""
import itertools
import os
import sys

import numpy as np
import pytest
from click.testing import CliRunner

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import CalculateResult, MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import write_point_cloud
from open_pcc_metric_amd.metric import (GeoHausdorffDistance, GeoRankedHausdorffDistance, GeoRankedHausdorffDistancePSNR,
                                        MaxSqrtDistance, SymmetricMetric, rank_index)
from open_pcc_metric_amd.options import CalculateOptions, check_hausdorff_rank, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ranked_reference as ref  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402

DIST, PSNR = "GeoRankedHausdorffDistance", "GeoRankedHausdorffDistancePSNR"


def keys(opts):
    return [m._key() for m in transform_options(opts)]


# ---- the index ---------------------------------------------------------------------------------------------------------------
def test_rank_index_fixed_points():
    assert ref.rank_index(0.07, 100) == 7                         # (ceil(0.07 * 100) is 8 in fp64)
    assert ref.rank_index(0.99, 1_000_000) == 990_000
    assert ref.rank_index(1e-9, 5) == 1
    for n in (1, 2, 127, 8193, 1_000_000, 32 * 1024 * 1024):
        assert ref.rank_index(1.0, n) == n
        assert ref.rank_index(1, n) == n


def test_product_index_agrees_with_the_restatement():
    assert rank_index(0.07, 100) == 7 and rank_index(0.99, 1_000_000) == 990_000 and rank_index(1e-9, 5) == 1
    rng = np.random.default_rng(5)
    for _ in range(4000):
        n = int(rng.integers(1, 40_000_000))
        r = float(rng.choice([rng.random(), round(rng.random(), int(rng.integers(1, 6))), 1.0 - rng.random() * 1e-6]))
        if r <= 0.0:
            continue
        k = rank_index(r, n)
        assert k == ref.rank_index(r, n) and 1 <= k <= n, (r, n)


# ---- options -----------------------------------------------------------------------------------------------------------------
def test_option_is_normalised():
    assert CalculateOptions().hausdorff_rank == ()
    assert CalculateOptions(hausdorff_rank=0.95).hausdorff_rank == (0.95,)
    assert CalculateOptions(hausdorff_rank=1).hausdorff_rank == (1.0,)
    assert CalculateOptions(hausdorff_rank=[0.99, 0.5, 0.99, np.float64(0.999)]).hausdorff_rank == (0.5, 0.99, 0.999)
    assert CalculateOptions(hausdorff_rank=(r for r in (1.0, 0.25))).hausdorff_rank == (0.25, 1.0)
    assert all(type(r) is float for r in CalculateOptions(hausdorff_rank=[np.float32(0.5), 1]).hausdorff_rank)


@pytest.mark.parametrize("bad", [0, 0.0, -0.5, 1.0000001, 2, float("nan"), float("inf"), True, False, "0.5", [0.5, "x"], [None],
                                 [0.1, 0.2, 0.3, 0.4, 0.5], [0.5, True], object()])
def test_bad_ranks_raise(bad):
    with pytest.raises(ValueError):
        CalculateOptions(hausdorff_rank=bad)


def ranked_keys(ranks, p2plane):
    out = []
    for r in ranks:
        for p in (False, True) if p2plane else (False,):
            out += [(DIST, True, p, r), (DIST, False, p, r), ("SymmetricMetric", DIST, True, p, r, DIST, False, p, r),
                    (PSNR, True, p, r), (PSNR, False, p, r), ("SymmetricMetric", PSNR, True, p, r, PSNR, False, p, r)]
    return out


@pytest.mark.parametrize("ranks", [(0.95,), (0.999, 0.5, 0.99)], ids=["one", "three"])
@pytest.mark.parametrize("color, hd, p2plane", list(itertools.product([None, "ycc"], [False, True], [False, True])))
def test_rows_follow_every_existing_row(ranks, color, hd, p2plane):
    extra = dict(plane_to_plane=hd, point_ssim=("geometry",) if color else ())
    base = keys(CalculateOptions(color, hd, p2plane, **extra))
    opts = CalculateOptions(color, hd, p2plane, hausdorff_rank=ranks, **extra)
    got = keys(opts)
    assert got[:len(base)] == base                                # PointSSIM and plane-to-plane rows included
    assert got[len(base):] == ranked_keys(sorted(ranks), p2plane)
    metrics = transform_options(opts)[len(base):]
    for m in metrics:
        m.value = 0.5
        if isinstance(m, SymmetricMetric):                       # the distance reports the larger side, the PSNR the smaller
            assert m.is_proportional == isinstance(m.metrics[0], GeoRankedHausdorffDistancePSNR)
    df = CalculateResult(metrics).as_df()
    labels = []
    for r in sorted(ranks):
        for _ in (False, True) if p2plane else (False,):
            labels += [f"{DIST}[{r!r}]"] * 2 + [f"{DIST}[{r!r}](symmetric)"] + [f"{PSNR}[{r!r}]"] * 2 + [f"{PSNR}[{r!r}](symmetric)"]
    assert list(df["label"]) == labels
    assert list(df["is_left"][:3]) == [True, False, ""] and list(df["point-to-plane"][:3]) == [False, False, ""]


def test_without_the_option_the_rows_are_todays():
    for color, hd, p2plane in itertools.product([None, "ycc"], [False, True], [False, True]):
        base = keys(CalculateOptions(color, hd, p2plane))
        assert keys(CalculateOptions(color, hd, p2plane, hausdorff_rank=None)) == base
        assert keys(CalculateOptions(color, hd, p2plane, hausdorff_rank=())) == base
        assert not any("Ranked" in str(k) for k in base)
    assert len(keys(CalculateOptions("ycc", True, True))) == 32
    metrics = transform_options(CalculateOptions("ycc", True, True))
    for m in metrics:
        m.value = 1.0
    labels = list(CalculateResult(metrics).as_df()["label"])
    assert not any("[" in label for label in labels) and labels.count("GeoHausdorffDistance(symmetric)") == 2


def test_dependencies_and_keys():
    m = GeoRankedHausdorffDistancePSNR(False, True, 0.99)
    deps = m._get_dependencies()
    assert isinstance(deps["max_sqrt"], MaxSqrtDistance)
    assert deps["ranked_distance"]._key() == (DIST, False, True, 0.99)
    euclid = deps["ranked_distance"]._get_dependencies()["euclidean_distance"]
    assert euclid._key() == GeoHausdorffDistance(False, True)._get_dependencies()["euclidean_distance"]._key()


# ---- the nodes over plain arrays ---------------------------------------------------------------------------------------------
class StandIn:
    """A pair whose getters return plain ndarrays (as the reference's unit tests inject them)."""
    def __init__(self, n=257, m=131, seed=0):
        rng = np.random.default_rng(seed)
        self.d = {True: rng.random(n) ** 3, False: np.round(rng.random(m) * 8) / 4}      # the right column is full of ties
        self.err = {True: rng.standard_normal((n, 3)), False: rng.standard_normal((m, 3))}
        self.nrm = {0: rng.standard_normal((max(n, m), 3)), 1: rng.standard_normal((max(n, m), 3))}
        self.spacing = rng.random(n) + 0.1

    def get_left_neighbour_distances(self):
        return self.d[True]

    def get_right_neighbour_distances(self):
        return self.d[False]

    def get_left_error_vector(self):
        return self.err[True]

    def get_right_error_vector(self):
        return self.err[False]

    def get_normals(self, which):
        return self.nrm[which]

    def get_boundary_sqrt_distances(self):
        return self.spacing

    def get_extent(self):
        return np.array([1.0, 2.0, 3.0])

    def d2(self, is_left):
        err, nrm = self.err[is_left], self.nrm[1 if is_left else 0]
        return np.square(np.array([np.dot(err[i], nrm[i]) for i in range(len(err))]))


RANKS = (1e-9, 0.07, 0.5, 0.95, 1.0)


@pytest.mark.filterwarnings("ignore:divide by zero")             # (a zero distance: PSNR inf, as the Hausdorff rows behave)
def test_nodes_over_plain_arrays_equal_the_restatement():
    pair = StandIn()
    res = MetricCalculator(pair).calculate(transform_options(CalculateOptions(None, True, True, hausdorff_rank=RANKS[:4]))).as_dict()
    res.update(MetricCalculator(pair).calculate(transform_options(CalculateOptions(None, True, True, hausdorff_rank=1.0))).as_dict())
    peak = np.max(pair.spacing)
    for r in RANKS:
        for p2p in (False, True):
            want = {s: ref.ranked(pair.d2(s) if p2p else pair.d[s], r) for s in (True, False)}
            for s in (True, False):
                assert res[(DIST, s, p2p, r)] == want[s]
                assert res[(PSNR, s, p2p, r)] == ref.ranked_psnr(peak, want[s])
            assert res[("SymmetricMetric", DIST, True, p2p, r, DIST, False, p2p, r)] == max(want[True], want[False])
            # (SymmetricMetric compares by np.linalg.norm, the reference's key: the PSNR of the smaller magnitude, left on ties)
            pl, pr = ref.ranked_psnr(peak, want[True]), ref.ranked_psnr(peak, want[False])
            assert res[("SymmetricMetric", PSNR, True, p2p, r, PSNR, False, p2p, r)] == (pr if abs(pr) < abs(pl) else pl)
    for p2p in (False, True):                                     # r = 1 is the classic row, bit for bit
        for s in (True, False):
            col = pair.d2(s) if p2p else pair.d[s]
            assert res[(DIST, s, p2p, 1.0)] == np.max(col) == res[("GeoHausdorffDistance", s, p2p)]
            assert res[(PSNR, s, p2p, 1.0)] == res[("GeoHausdorffDistancePSNR", s, p2p)]
            assert res[(DIST, s, p2p, 1e-9)] == np.min(col)


# ---- a CloudPair on an engine without the selection call ---------------------------------------------------------------------
def oracle_pair(n=300, m=280, **kw):
    rng = np.random.default_rng(11)
    a = PointCloud(rng.random((n, 3)), rng.standard_normal((max(n, m), 3))[:n])
    b = PointCloud(rng.random((m, 3)), rng.standard_normal((max(n, m), 3)))
    return CloudPair(a, b, extent=[1.0, 1.0, 1.0], _engine=OracleEngine(), normal_index="neighbour", **kw)


def test_engine_without_selection_falls_back_to_the_column():
    assert not hasattr(OracleEngine, "select_many")
    pair = oracle_pair()
    opts = CalculateOptions(None, True, True, hausdorff_rank=(0.5, 0.95, 1.0))
    res = MetricCalculator(pair).calculate(transform_options(opts)).as_dict()
    base = MetricCalculator(pair).calculate(transform_options(CalculateOptions(None, True, True))).as_dict()
    for key, value in base.items():                               # every earlier row is what it was
        assert res[key] == value
    cols = {(True, False): np.asarray(pair.get_left_neighbour_distances()), (False, False): np.asarray(pair.get_right_neighbour_distances()),
            (True, True): np.asarray(np.square(pair.point_to_plane_column(True))), (False, True): np.asarray(np.square(pair.point_to_plane_column(False)))}
    for (s, p2p), col in cols.items():
        for r in (0.5, 0.95, 1.0):
            assert res[(DIST, s, p2p, r)] == ref.ranked(col, r)
        assert res[(DIST, s, p2p, 1.0)] == base[("GeoHausdorffDistance", s, p2p)]
        assert res[(PSNR, s, p2p, 1.0)] == base[("GeoHausdorffDistancePSNR", s, p2p)]


def test_sharded_pairs_are_refused_before_the_engine_is_touched():
    check_hausdorff_rank(CalculateOptions(), group=object())      # no ranked rows: nothing to check
    check_hausdorff_rank(CalculateOptions(hausdorff_rank=0.5))
    with pytest.raises(ValueError, match="sharded"):
        check_hausdorff_rank(CalculateOptions(hausdorff_rank=0.5), group=object())
    pair = oracle_pair()

    class Peers:                                                  # what Collective(group) says of a group with two ranks
        sharded, group, rank, world = True, object(), 0, 2
    pair._coll = Peers()
    calls = list(pair._engine.calls)
    with pytest.raises(ValueError, match="sharded"):
        MetricCalculator(pair).calculate(transform_options(CalculateOptions(hausdorff_rank=0.5)))
    assert pair._engine.calls == calls


def test_cli_refuses_a_bad_rank_before_any_context(tmp_path, monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a GPU context was asked for")
    monkeypatch.setattr(nat, "acquire_engine", no_context)
    monkeypatch.setattr(nat, "Engine", no_context)
    rng = np.random.default_rng(0)
    pa, pb = str(tmp_path / "a.xyz"), str(tmp_path / "b.xyz")
    write_point_cloud(pa, PointCloud(rng.random((20, 3))))
    write_point_cloud(pb, PointCloud(rng.random((20, 3))))
    for extra in (["--hausdorff-rank", "0"], ["--hausdorff-rank", "1.5"], ["--hausdorff-rank", "-0.1"], ["--hausdorff-rank", "nan"],
                  ["--hausdorff-rank", "x"], sum((["--hausdorff-rank", str(r)] for r in (0.1, 0.2, 0.3, 0.4, 0.5)), [])):
        out = CliRunner().invoke(cli, ["--ocloud", pa, "--pcloud", pb] + extra)
        assert out.exit_code == 2, (extra, out.output, out.exception)
    out = CliRunner().invoke(cli, ["--help"])
    assert out.exit_code == 0 and "--hausdorff-rank" in out.output
