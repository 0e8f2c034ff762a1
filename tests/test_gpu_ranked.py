"""Ranked (generalized) Hausdorff rows on the GPU (include/pccm.h, pccm_select_many; CalculateOptions(hausdorff_rank=...)).

An order statistic has no rounding: every value here is compared with ``==`` on its float64 bits against the NumPy restatement
of tests/ranked_reference.py (np.partition), applied to the oracle's column and to the GPU's own fetched column."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
from click.testing import CliRunner

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair, DeviceColumn
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import read_point_cloud, write_point_cloud
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud
from open_pcc_metric_amd.sequence import evaluate_pairs
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ranked_reference as ref  # noqa: E402
import variant_rows as vr  # noqa: E402
from test_gpu_ties_mean import MeanOracleEngine, lattice_pair  # noqa: E402
from test_gpu_vox import shell  # noqa: E402

DIST, PSNR = "GeoRankedHausdorffDistance", "GeoRankedHausdorffDistancePSNR"
D1, D2, PR = nat.METRIC_D1, nat.METRIC_D2, nat.METRIC_PROJ
TINY = 1e-9
SIDES = [(True, False), (False, False), (True, True), (False, True)]      # (is_left, point_to_plane)


def same(x, y):
    return np.float64(x).tobytes() == np.float64(y).tobytes()


def report(pair, ranks, hausdorff=True, p2plane=True, color=None, frame=False, **kw):
    opts = CalculateOptions(color, hausdorff, p2plane, hausdorff_rank=ranks, **kw)
    with np.errstate(divide="ignore"):
        res = MetricCalculator(pair).calculate(transform_options(opts))
        return res.as_df() if frame else res.as_dict()


def oracle_columns(a, b, na, nb, mode):
    il, dl = orc.nn(a, b, method="kdtree")
    ir, dr = orc.nn(b, a, method="kdtree")
    cols = {(True, False): dl, (False, False): dr}
    if na is not None:
        pl = orc.point_to_plane(a, b, il, nb, normal_index=mode)
        pr = orc.point_to_plane(b, a, ir, na, normal_index=mode)
        cols.update({(True, True): pl * pl, (False, True): pr * pr})
    return cols


def gpu_columns(pair, p2plane=True):
    cols = {(True, False): np.asarray(pair.get_left_neighbour_distances()), (False, False): np.asarray(pair.get_right_neighbour_distances())}
    if p2plane:
        cols[(True, True)] = np.asarray(np.square(pair.point_to_plane_column(True)))
        cols[(False, True)] = np.asarray(np.square(pair.point_to_plane_column(False)))
    return cols


def check_rows(res, cols, ranks):
    """Every ranked row of a report against the restatement over `cols`."""
    peak = res[("MaxSqrtDistance",)]
    for r in ranks:
        for p2p in sorted({p for _, p in cols}):
            want = {s: ref.ranked(cols[(s, p2p)], r) for s in (True, False)}
            with np.errstate(divide="ignore"):
                psnr = {s: ref.ranked_psnr(peak, want[s]) for s in (True, False)}
            for s in (True, False):
                assert same(res[(DIST, s, p2p, r)], want[s]), (r, s, p2p, res[(DIST, s, p2p, r)], want[s])
                assert same(res[(PSNR, s, p2p, r)], psnr[s]), (r, s, p2p)
            assert same(res[("SymmetricMetric", DIST, True, p2p, r, DIST, False, p2p, r)],
                        want[False] if want[False] > want[True] else want[True])
            assert same(res[("SymmetricMetric", PSNR, True, p2p, r, PSNR, False, p2p, r)],
                        psnr[False] if abs(psnr[False]) < abs(psnr[True]) else psnr[True])


def uniform(n, m, seed, dtype=np.float32, offset=0.0, scale=1.0):
    rng = np.random.default_rng(seed)
    a = (offset + scale * rng.random((n, 3))).astype(dtype)
    b = (offset + scale * rng.random((m, 3))).astype(dtype)
    rows = max(n, m)
    return a, b, vr._unit(rows, seed + 1)[:n], vr._unit(rows, seed + 2)[:m]


# ---- reports over uniform pairs ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def uniform_case(n):
    a, b, na, nb = uniform(n, n, n)
    return a, b, na, nb, oracle_columns(a, b, na, nb, "row")


@pytest.mark.parametrize("engine", ["grid", "brute"])
@pytest.mark.parametrize("n", [1, 2, 127, 8191, 8193, 100_003, 1_000_000])
def test_uniform_pairs(n, engine):
    a, b, na, nb, want = uniform_case(n)
    with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0], nn_engine=engine) as pair:
        first = report(pair, (TINY, 0.5, 0.95, 0.999))
        last = report(pair, 1.0)
        own = gpu_columns(pair)
    for cols in (want, own):
        check_rows(first, cols, (TINY, 0.5, 0.95, 0.999))
        check_rows(last, cols, (1.0,))
    for s, p2p in SIDES:                       # r = 1 is the classic row of the same report; the smallest rank is the minimum
        assert same(last[(DIST, s, p2p, 1.0)], last[("GeoHausdorffDistance", s, p2p)])
        assert same(last[(PSNR, s, p2p, 1.0)], last[("GeoHausdorffDistancePSNR", s, p2p)])
        assert same(first[(DIST, s, p2p, TINY)], np.min(want[(s, p2p)]))


@pytest.mark.parametrize("mode", ["row", "neighbour"])
def test_georeferenced_fp64_clouds(mode):
    n, m = (20_011, 20_011) if mode == "row" else (20_011, 17_001)
    a, b, na, nb = uniform(n, m, 77, dtype=np.float64, offset=4_500_000.0, scale=50.0)
    na, nb = vr._unit(n, 5, True), vr._unit(m, 6, True)
    want = oracle_columns(a, b, na, nb, mode)
    with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[50.0, 50.0, 50.0], normal_index=mode) as pair:
        res = report(pair, (0.5, 0.95, 0.999, 1.0))
        own = gpu_columns(pair)
    for cols in (want, own):
        check_rows(res, cols, (0.5, 0.95, 0.999, 1.0))


@pytest.mark.parametrize("n, m", [(1, 1), (2, 3), (1, 50)])
def test_tiny_columns_through_the_engine(n, m):
    a, b, na, nb = uniform(n, m, 3 + n + m)
    want = oracle_columns(a, b, na, nb, "neighbour")
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, a); eng.set_cloud(1, b)
        eng.set_normals(0, na); eng.set_normals(1, nb)
        eng.nn_pair("grid")
        for (s, p2p), col in want.items():
            d, met = (0 if s else 1), (D2 if p2p else D1)
            ks = sorted({1, (len(col) + 1) // 2, len(col)})
            got = eng.select_many([(d, met, k) for k in ks], "neighbour")
            assert all(same(g, np.partition(col, k - 1)[k - 1]) for g, k in zip(got, ks)), (s, p2p, got)
    finally:
        eng.close()


# ---- every value path of the reducers ----------------------------------------------------------------------------------------
def test_every_reduction_value_path_is_ranked_as_it_is_reduced():
    """The loop of variants_check.run_reduce -- engine x normals x normal_index x matched rows kept x projection fused -- with
    select_many beside reduce_total_many: matched records with defer 1..5, 32- and 16-byte records, plain columns."""
    batches = [[(0, D1)], [(1, D2)], [(0, D1), (0, D2), (1, D1), (1, D2)], [(0, D1), (1, D2)], [(0, PR), (1, PR)],
               [(0, D1), (0, PR)], [(1, D2), (1, D1)]]
    paths, turn = set(), 0
    eng = nat.Engine(0)
    try:
        for n, m in ((8192 + 128, 8191), (128 * 41 + 1, 127 * 41)):
            a, b, _ = vr.make_pair(n, m, seed=0)
            want = {0: orc.nn(a, b, method="kdtree"), 1: orc.nn(b, a, method="kdtree")}
            eng.set_cloud(0, a); eng.set_cloud(1, b)
            for engine in ("grid", "brute"):
                for flavour in ("f32", "f64", None):
                    for mode in ("neighbour", "row"):
                        for want_idx in (True, False):
                            if flavour is None and mode == "row":
                                continue
                            na = nb = None
                            if flavour:
                                la, lb = (n, m) if mode == "neighbour" else (max(n, m),) * 2
                                na, nb = vr._unit(la, 7, flavour == "f64"), vr._unit(lb, 8, flavour == "f64")
                                eng.set_normals(0, na); eng.set_normals(1, nb)
                            for fuse in ((mode, None) if flavour else (None,)):
                                for d in (0, 1):
                                    eng.nn_fuse(d, fuse)
                                eng.nn_want_idx(want_idx)
                                cols = {}
                                for d, (it, se, nse) in enumerate(((a, b, nb), (b, a, na))):
                                    cols[(d, D1)] = want[d][1]
                                    if flavour:
                                        p = orc.point_to_plane(it, se, want[d][0], nse, normal_index=mode)
                                        cols[(d, D2)] = p * p
                                for batch in batches:
                                    if not flavour and any(met != D1 for _, met in batch):
                                        continue
                                    what = f"{engine} {flavour} {mode} idx={want_idx} fuse={fuse} batch={batch}"
                                    req = []
                                    for d, met in batch:
                                        if met != PR:
                                            rows = len(cols[(d, met)])
                                            req += [(d, met, ref.rank_index(0.5, rows)), (d, met, ref.rank_index(0.999, rows))]
                                    eng.drop_caches()
                                    eng.nn_pair(engine)
                                    turn += 1
                                    if turn % 2:                 # enqueued behind the batch's reductions, or on columns already consumed
                                        eng.reduce_prefetch_many(batch, mode)
                                        eng.select_prefetch_many(req, mode)
                                    got = eng.reduce_total_many(batch, mode)
                                    paths.update(eng.last_path(nat.PATH_REDUCE))
                                    sel = eng.select_many(req, mode)
                                    if req:
                                        assert "k_unit_jobs" in eng.last_path(nat.PATH_REDUCE), what
                                    for (d, met, k), v in zip(req, sel):
                                        col = cols[(d, met)]
                                        assert same(v, np.partition(col, k - 1)[k - 1]), (what, d, met, k, v)
                                    for (d, met), (total, mn, mx) in zip(batch, got):
                                        if met != PR:
                                            col = cols[(d, met)]
                                            assert same(total, np.sum(col)) and mn == np.min(col) and mx == np.max(col), what
    finally:
        eng.close()
    missing = [k for k in vr.ROWS["reduce_shapes"]["expect"] if k not in paths]
    assert not missing, (missing, sorted(paths))


# ---- heavy ties, degenerate columns, many binades ----------------------------------------------------------------------------
def rank_for(k, n):
    """A rank r with rank_index(r, n) == k."""
    for r in (k / n, float(np.nextafter(k / n, 0.0)), (k - 0.5) / n):
        if 0.0 < r <= 1.0 and ref.rank_index(r, n) == k:
            return r
    raise AssertionError((k, n))


def test_voxelised_pair_ranks_at_the_edges_of_runs():
    a, b = shell(40_000, 1, (40, -15, 7), 120, dup=300), shell(35_000, 2, (41, -15, 6), 121, 0.6, dup=200)
    want = oracle_columns(a, b, None, None, "row")
    with CloudPair(PointCloud(a), PointCloud(b), extent=[300.0, 300.0, 300.0]) as pair:
        assert any("k_vox_query" in k for k in pair._engine.last_path(0)), pair._engine.last_path(0)
        for s in (True, False):
            col = np.sort(want[(s, False)])
            n = len(col)
            values, first, counts = np.unique(col, return_index=True, return_counts=True)
            assert len(values) < 200 and counts.max() > 1000                  # a few dozen integers, long runs
            run = int(np.argmax(counts[:-1]))                                  # (not the last run: one past it exists)
            ks = [int(first[run]) + 1, int(first[run] + counts[run]), int(first[run] + counts[run]) + 1]
            ranks = tuple(rank_for(k, n) for k in ks)
            res = report(pair, ranks, hausdorff=True, p2plane=False)
            own = gpu_columns(pair, p2plane=False)
            check_rows(res, want, sorted(ranks))
            check_rows(res, own, sorted(ranks))
            got = [res[(DIST, s, False, r)] for r in ranks]
            assert got[0] == got[1] == values[run] and got[2] == values[run + 1]


def test_all_equal_and_all_zero_columns():
    g = np.arange(20, dtype=np.float32) * 4.0
    a = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    a = a[np.random.default_rng(0).permutation(len(a))]
    b = a + np.array([1.0, 0.0, 0.0], dtype=np.float32)
    nrm = vr._unit(len(a), 9)
    ranks = (TINY, 0.5, 0.999, 1.0)
    with CloudPair(PointCloud(a, nrm), PointCloud(b, nrm), extent=[80.0, 80.0, 80.0]) as pair:
        res = report(pair, ranks)
        own = gpu_columns(pair)
    assert np.all(own[(True, False)] == 1.0) and np.all(own[(False, False)] == 1.0)
    check_rows(res, oracle_columns(a, b, nrm, nrm, "row"), ranks)
    check_rows(res, own, ranks)
    assert all(res[(DIST, s, False, r)] == 1.0 for s in (True, False) for r in ranks)
    with CloudPair(PointCloud(a, nrm), PointCloud(a.copy(), nrm), extent=[80.0, 80.0, 80.0]) as pair:
        res = report(pair, ranks)
    for s, p2p in SIDES:
        for r in ranks:                        # value 0, PSNR inf: exactly as the Hausdorff rows behave there
            assert same(res[(DIST, s, p2p, r)], 0.0) and res[(PSNR, s, p2p, r)] == np.inf
            assert same(res[(DIST, s, p2p, r)], res[("GeoHausdorffDistance", s, p2p)])
            assert res[(PSNR, s, p2p, r)] == res[("GeoHausdorffDistancePSNR", s, p2p)]


def test_columns_over_sixty_binades_with_exact_zeros():
    """Points at offsets 0 and 2^-20 .. 2^10 from their partners, 4096 apart from everything else: every radix pass chooses
    among several occupied bins."""
    count = 3200
    i = np.arange(count)
    a = np.stack([4096.0 * (i % 64), np.zeros(count), 4096.0 * (i // 64)], axis=1).astype(np.float32)
    e = i % 32 - 21                                                       # -21: the partner coincides
    off = np.where(e < -20, 0.0, 2.0 ** e.astype(np.float64))
    b = a.copy()
    b[:, 1] = off.astype(np.float32)
    perm = np.random.default_rng(4).permutation(count)
    a, b = a[perm], b[np.random.default_rng(5).permutation(count)]
    na, nb = vr._unit(count, 1), vr._unit(count, 2)
    want = oracle_columns(a, b, na, nb, "neighbour")
    d1 = want[(True, False)]
    assert np.sum(d1 == 0.0) == count // 32 and np.log2(d1[d1 > 0].max() / d1[d1 > 0].min()) >= 40
    assert np.array_equal(np.sort(d1), np.sort(off * off))               # each point's partner is its nearest neighbour
    ranks = (0.02, 0.04, 0.5, 0.97)
    with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0], normal_index="neighbour") as pair:
        res = [report(pair, ranks), report(pair, (0.0315, 0.2, 0.8, 1.0))]
        own = gpu_columns(pair)
    for cols in (want, own):
        check_rows(res[0], cols, ranks)
        check_rows(res[1], cols, (0.0315, 0.2, 0.8, 1.0))
    assert res[0][(DIST, True, False, 0.02)] == 0.0 and res[0][(DIST, True, False, 0.04)] == 2.0 ** -40


# ---- tie policy, several decoded clouds, graphs ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["row", "neighbour"])
def test_ties_mean_ranks_the_tie_mean_column(mode):
    a, b = lattice_pair()
    ranks = (0.25, 0.5, 0.95, 1.0)
    with np.errstate(divide="ignore"):
        want = report(CloudPair(a, b, extent=[24.0, 24.0, 24.0], normal_index=mode, ties="mean", _engine=MeanOracleEngine()), ranks)
    with CloudPair(a, b, extent=[24.0, 24.0, 24.0], normal_index=mode, ties="mean", use_graph=True) as pair:
        for _ in range(3):                     # (eager every time: nothing is captured under "mean")
            got = report(pair, ranks)
            pair.recompute()
        assert pair._graph_id is None
        own = gpu_columns(pair)
    with CloudPair(a, b, extent=[24.0, 24.0, 24.0], normal_index=mode) as pick:
        picked = report(pick, ranks)
    ranked_keys = [k for k in want if "Ranked" in str(k)]
    assert len(ranked_keys) == 48
    for k in ranked_keys:
        assert same(got[k], want[k]), k
    check_rows(got, own, ranks)
    for r in ranks:                            # D1 is the same under either policy; D2 ranks another column
        for s in (True, False):
            assert same(got[(DIST, s, False, r)], picked[(DIST, s, False, r)])
    assert any(not same(got[(DIST, s, True, r)], picked[(DIST, s, True, r)]) for s in (True, False) for r in ranks)


def test_with_reconst_and_evaluate_pairs():
    n = 30_000
    a, b0, na, nb = uniform(n, n, 21)
    origin = PointCloud(a, na)
    decoded = [PointCloud((b0 + np.float32(0.001 * k)).astype(np.float32), nb) for k in range(3)]
    ranks = (0.5, 0.99)
    pair, got = CloudPair(origin, decoded[0], extent=[1.0, 1.0, 1.0]), []
    try:
        for k in range(3):
            if k:
                pair = pair.with_reconst(decoded[k])
            got.append(report(pair, ranks))
    finally:
        pair.close()
    for k in range(3):
        check_rows(got[k], oracle_columns(a, np.asarray(decoded[k].points), na, nb, "row"), ranks)
    opts = CalculateOptions(None, True, True, hausdorff_rank=ranks)
    for res, mine in zip(evaluate_pairs([(origin, d) for d in decoded], opts, workers=1, extent=[1.0, 1.0, 1.0]), got):
        assert list(res) == list(mine) and all(same(res[k], mine[k]) for k in res)


def test_graph_replays_recapture_and_new_points():
    n = 50_000
    a, b, na, nb = uniform(n, n, 31)
    ranks = (0.5, 0.95, 0.999)
    want = oracle_columns(a, b, na, nb, "row")
    with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0], use_graph=True) as pair:
        rows = []
        for _ in range(5):                     # eager, capture, three replays
            rows.append(report(pair, ranks))
            pair.recompute()
        assert pair._graph_id is not None
        check_rows(rows[0], want, ranks)
        for r in rows[1:]:
            assert list(r) == list(rows[0]) and all(same(r[k], rows[0][k]) for k in r)
        other = report(pair, (0.25, 1.0))      # a report with other ranks is another report: captured anew
        check_rows(other, want, (0.25, 1.0))
        for _ in range(3):
            pair.recompute()
            again = report(pair, (0.25, 1.0))
            assert all(same(again[k], other[k]) for k in other)
        assert pair._graph_id is not None
        b2 = (b * np.float32(0.97)).astype(np.float32)
        nxt = pair.with_reconst(PointCloud(b2, nb))
    try:
        want2 = oracle_columns(a, b2, na, nb, "row")
        for _ in range(4):
            check_rows(report(nxt, ranks), want2, ranks)
            nxt.recompute()
        assert nxt._graph_id is not None
    finally:
        nxt.close()


# ---- nothing leaves the GPU, nothing else moves ------------------------------------------------------------------------------
def test_no_column_is_materialised_and_earlier_rows_do_not_move(monkeypatch):
    n = 60_000
    a, b, na, nb = uniform(n, n, 41)
    rng = np.random.default_rng(42)
    ca, cb = rng.integers(0, 256, (n, 3)) / 255.0, rng.integers(0, 256, (n, 3)) / 255.0
    ranks = (0.9, 0.99, 0.999)
    with CloudPair(PointCloud(a, na, ca), PointCloud(b, nb, cb), extent=[1.0, 1.0, 1.0]) as pair:
        plain = report(pair, None, color="ycc", frame=True, plane_to_plane=True, point_ssim=("geometry",))
    with CloudPair(PointCloud(a, na, ca), PointCloud(b, nb, cb), extent=[1.0, 1.0, 1.0]) as pair:
        def never(self):
            raise AssertionError(f"{self!r} was copied to the host")
        monkeypatch.setattr(DeviceColumn, "_materialise", never)
        full = report(pair, ranks, color="ycc", frame=True, plane_to_plane=True, point_ssim=("geometry",))
        values = report(pair, ranks)
        monkeypatch.undo()
        check_rows(values, gpu_columns(pair), ranks)
    assert len(full) == len(plain) + 36
    assert full.iloc[:len(plain)].to_string() == plain.to_string()          # values and text of every earlier row
    assert all("Ranked" in label for label in full["label"][len(plain):])


# ---- command line and C ABI --------------------------------------------------------------------------------------------------
def test_command_line(tmp_path):
    n = 5000
    a, b, na, nb = uniform(n, n, 51)
    pa, pb = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    write_point_cloud(pa, PointCloud(a, na))
    write_point_cloud(pb, PointCloud(b, nb))
    args = ["--ocloud", pa, "--pcloud", pb, "--hausdorff", "--point-to-plane"]
    base = CliRunner().invoke(cli, args)
    out = CliRunner().invoke(cli, args + ["--hausdorff-rank", "0.99", "--hausdorff-rank", "0.95"])
    assert base.exit_code == 0 and out.exit_code == 0, (base.output, out.output, out.exception)
    base_lines, lines = base.output.rstrip("\n").split("\n"), out.output.rstrip("\n").split("\n")
    assert len(lines) == len(base_lines) + 24
    # today's rows, then the new ones (the frame is wider: compare the fields)
    assert [ln.split() for ln in lines[1:len(base_lines)]] == [ln.split() for ln in base_lines[1:]]
    fa, fb = read_point_cloud(pa), read_point_cloud(pb)
    with CloudPair(fa, fb) as pair:
        res = report(pair, (0.95, 0.99))
        check_rows(res, gpu_columns(pair), (0.95, 0.99))
    check_rows(res, oracle_columns(np.asarray(fa.points), np.asarray(fb.points), np.asarray(fa.normals), np.asarray(fb.normals), "row"),
               (0.95, 0.99))
    want = []
    for r in (0.95, 0.99):
        for p2p in (False, True):
            for name in (DIST, PSNR):
                want += [[f"{name}[{r!r}]", str(s), str(p2p), str(res[(name, s, p2p, r)])] for s in (True, False)]
                want.append([f"{name}[{r!r}](symmetric)", str(res[("SymmetricMetric", name, True, p2p, r, name, False, p2p, r)])])
    assert [ln.split()[1:] for ln in lines[len(base_lines):]] == want


def test_c_calls_and_their_error_codes():
    n, m = 5000, 4000
    a, b, na, nb = uniform(n, m, 61)
    lib = nat.load()
    eng = nat.Engine(0)

    def call(fn, reqs, modes=None, out=True):
        k = len(reqs)
        arr = ctypes.c_int * k
        args = [eng._ctx, k, arr(*[r[0] for r in reqs]), arr(*[r[1] for r in reqs]), arr(*(modes or [1] * k)),
                (ctypes.c_int64 * k)(*[r[2] for r in reqs])]
        buf = (ctypes.c_double * max(k, 1))()
        rc = fn(*args, buf) if out else fn(*args)
        return rc, list(buf)[:k]
    try:
        eng.set_cloud(0, a); eng.set_cloud(1, b)
        for fn, out in ((lib.pccm_select_prefetch_many, False), (lib.pccm_select_many, True)):
            assert call(fn, [(0, D1, 1)], out=out)[0] == nat.E_STATE                 # no search result yet
        eng.nn_pair("grid")
        want = oracle_columns(a, b, na, nb, "neighbour")
        for fn, out in ((lib.pccm_select_prefetch_many, False), (lib.pccm_select_many, True)):
            assert call(fn, [(2, D1, 1)], out=out)[0] == nat.E_ARG                   # PCCM_DIR_SELF
            assert call(fn, [(3, D1, 1)], out=out)[0] == nat.E_ARG
            assert call(fn, [(0, PR, 1)], out=out)[0] == nat.E_ARG                   # other metrics
            assert call(fn, [(0, nat.METRIC_ANGULAR, 1)], out=out)[0] == nat.E_ARG
            assert call(fn, [(0, D1, 0)], out=out)[0] == nat.E_ARG                   # k outside 1..n_iter
            assert call(fn, [(0, D1, n + 1)], out=out)[0] == nat.E_ARG
            assert call(fn, [(1, D1, m + 1)], out=out)[0] == nat.E_ARG
            assert call(fn, [(0, D1, 1)] * 9, out=out)[0] == nat.E_ARG               # n <= 8
            assert call(fn, [(0, D2, 1)], out=out)[0] == nat.E_STATE                 # D2 without normals
            assert call(fn, [], out=out)[0] == nat.OK
        assert lib.pccm_select_many(eng._ctx, 1, None, None, None, None, None) == nat.E_ARG
        eng.set_normals(0, na); eng.set_normals(1, nb)
        # row-indexed normals: the iterating cloud (5000 rows) is larger than the other cloud's normals (4000)
        assert call(lib.pccm_select_many, [(0, D2, 1)], modes=[0])[0] == nat.E_RANGE
        assert call(lib.pccm_select_many, [(1, D2, 1)], modes=[0])[0] == nat.OK
        reqs = [(0, D1, 1), (0, D1, n), (1, D1, m // 2), (0, D2, n // 3), (1, D2, m), (0, D1, 2500), (0, D1, 17), (0, D1, 4999)]
        assert call(lib.pccm_select_prefetch_many, reqs, out=False)[0] == nat.OK
        rc, got = call(lib.pccm_select_many, reqs)
        assert rc == nat.OK
        for (d, met, k), v in zip(reqs, got):
            col = want[(d == 0, met == D2)]
            assert same(v, np.partition(col, k - 1)[k - 1]), (d, met, k)
        rc, again = call(lib.pccm_select_many, reqs)                                  # consumed: selected again, same bits
        assert rc == nat.OK and all(same(x, y) for x, y in zip(got, again))
        eng.set_shard(0, 2)
        assert call(lib.pccm_select_many, [(0, D1, 1)])[0] == nat.E_STATE            # a sharded context
    finally:
        eng.close()
    assert lib.pccm_version() == 100
