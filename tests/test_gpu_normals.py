"""GPU normal estimation (the stand-in for Open3D's estimate_normals, cloud_pair.py:61-64) against the
oracle's restatement.  Open3D itself cannot be pinned, so this is the one place with a
tolerance: normals are eigenvectors, compared up to sign where the eigen-gap makes them well defined
(|cos| >= 1 - 1e-9), and the D2 report computed from them must agree to 1e-9 relative.

The second half of the file holds every point to the high-precision reference of tests/normals_reference.py instead: exact
brute-force neighbours, an extended-precision covariance, and a per-point tolerance tau = K 2^-52 (kappa + kappa^2) that follows
the conditioning of the point's own eigenproblem -- per k and family, per slot and grid choice, per stage of the search (shown by
classifying every point on the host: tests/knn_stages.py), over more than one trip of the wave kernel's loop, and on clouds of
fewer points than k."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_stages as stages  # noqa: E402
import normals_reference as nr  # noqa: E402


def surface(n, seed, noise=0.002):
    rng = np.random.default_rng(seed)
    u, v = rng.random(n) * 2 - 1, rng.random(n) * 2 - 1
    z = 0.3 * np.sin(2 * u) * np.cos(3 * v) + rng.normal(0, noise, n)
    return np.stack([u, v, z], 1)


def check_normals(pts, k=30):
    e = nat.Engine(0)
    e.set_cloud(0, pts)
    e.set_cloud(1, pts[: max(1, len(pts) // 2)])
    e.estimate_normals(0, k)
    got = e.get_normals(0)
    e.close()
    want, w = orc.estimate_normals(pts, k)
    assert got.shape == want.shape
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-12)
    lead = got[np.arange(len(got)), np.argmax(np.abs(got), axis=1)]
    assert np.all(lead > 0)                                   # documented sign convention
    gap_ok = (w[:, 1] - w[:, 0]) > 1e-6 * np.maximum(w[:, 2], 1e-300)
    cos = np.abs(np.sum(got * want, axis=1))
    assert gap_ok.mean() > 0.9
    assert np.all(cos[gap_ok] >= 1 - 1e-9), float(cos[gap_ok].min())
    return got


@pytest.mark.parametrize("n,seed", [(3000, 1), (20000, 2)])
def test_normals_of_a_noisy_surface(n, seed):
    got = check_normals(surface(n, seed))
    assert np.mean(np.abs(got[:, 2]) > 0.5) > 0.9             # the sheet is roughly horizontal


def test_normals_uniform_volume_and_outliers():
    rng = np.random.default_rng(3)
    pts = rng.random((5000, 3))
    pts[:5] += 40.0                                           # isolated points: exact full-scan path
    check_normals(pts)


def test_normals_on_voxelised_surfaces_with_exact_ties():
    """Integer coordinates: the k-th neighbour distance is tied almost everywhere, so the (d2, row) order of the
    selection decides the neighbour set."""
    rng = np.random.default_rng(8)
    v = rng.standard_normal((40000, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    check_normals(np.unique(np.round(64 + 50 * v * [1.0, 0.7, 0.5]), axis=0))
    u = rng.integers(0, 120, (15000, 2)).astype(np.float64)
    sheet = np.unique(np.column_stack([u, np.round(0.3 * u[:, 0] + 4 * np.sin(u[:, 1] / 9.0))]), axis=0)
    check_normals(sheet)


def test_normals_tiny_and_degenerate_clouds():
    e = nat.Engine(0)
    two = np.array([[0.0, 0, 0], [1, 1, 1]])
    e.set_cloud(0, two)
    e.set_cloud(1, two)
    e.estimate_normals(0, 30)
    assert np.array_equal(e.get_normals(0), [[0, 0, 1], [0, 0, 1]])      # fewer than 3 points: Open3D's default
    plane = np.random.default_rng(4).random((200, 3))
    plane[:, 2] = 5.0
    e.set_cloud(0, plane)
    e.estimate_normals(0, 30)
    assert np.allclose(np.abs(e.get_normals(0)), [0, 0, 1], atol=1e-12)
    e.close()


def test_point_to_plane_report_with_estimated_normals():
    a = surface(6000, 5)
    b = a + np.random.default_rng(6).normal(0, 0.003, a.shape)
    pair = CloudPair(PointCloud(a), PointCloud(b), extent=[2, 2, 1])          # no normals given
    res = MetricCalculator(pair).calculate(transform_options(CalculateOptions(None, True, True))).as_dict()
    assert not pair.clouds[0].has_normals() and not pair.clouds[1].has_normals()   # inputs untouched (quirk Q5 not copied)
    na, _ = orc.estimate_normals(a, 30)
    nb, _ = orc.estimate_normals(b, 30)
    want = orc.OraclePair(a, b, na, nb, method="kdtree").report(hausdorff=True, point_to_plane_=True, peak=2.0)
    for key, val in want.items():
        assert res[key] == pytest.approx(val, rel=1e-9), key
    strict = CloudPair(PointCloud(a), PointCloud(b), extent=[2, 2, 1], estimate_normals=False)
    with pytest.raises(ValueError, match="normals"):
        MetricCalculator(strict).calculate(transform_options(CalculateOptions(None, False, True)))


# ---- every point against the high-precision reference ----------------------------------------------------------------------------
def estimate(pts, k, partner=None, slot=0, geometry=False):
    """The normals of `pts` as cloud `slot` beside `partner` (default: its own first half), estimated twice in one context: the
    second estimate must give the bits of the first."""
    partner = pts[: max(1, len(pts) // 2)] if partner is None else partner
    e = nat.Engine(0)
    try:
        e.set_cloud(slot, pts)
        e.set_cloud(1 - slot, partner)
        e.estimate_normals(slot, k)
        got = e.get_normals(slot)
        geom = e.grid_geometry() if geometry else None
        e.estimate_normals(slot, k)
        again = e.get_normals(slot)
    finally:
        e.close()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    return (got, geom) if geometry else got


def assert_within_tau(got, pts, nbr, label, rows=None, min_examined=0.98):
    """Unit length, the sign convention, and every examined point (tau < 1e-6) of `rows` within its tau of the reference."""
    want, _, kappa, tau = nr.reference(pts, nbr)
    assert got.shape == want.shape
    assert np.all(np.abs(np.linalg.norm(got, axis=1) - 1.0) <= 1e-12)
    assert np.all(got[np.arange(len(got)), np.argmax(np.abs(got), axis=1)] > 0)
    rows = np.arange(len(pts)) if rows is None else np.asarray(rows)
    ok = nr.examined(tau[rows])
    assert ok.mean() >= min_examined, (label, float(ok.mean()))
    ang = nr.angle(got[rows], want[rows])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = ang[ok] / (nr.EPS * (kappa[rows][ok] + kappa[rows][ok] ** 2))
    worst = int(np.argmax(ratio)) if ok.any() else -1
    print(f"{label}: {int(ok.sum())} of {len(rows)} examined, largest angle {ang[ok].max() if ok.any() else 0.0:.3e} rad, "
          f"largest angle / (2^-52 (kappa + kappa^2)) {ratio.max() if ok.any() else 0.0:.3f} (K = {nr.K}) at kappa "
          f"{kappa[rows][ok][worst] if ok.any() else 0.0:.3e}")
    bad = np.flatnonzero(ang[ok] > tau[rows][ok])
    assert bad.size == 0, (f"{label}: {bad.size} points outside tau, first rows {rows[ok][bad[:5]]}: angles {ang[ok][bad[:5]]}, "
                           f"tau {tau[rows][ok][bad[:5]]}")
    return ok


@functools.lru_cache(maxsize=None)
def family(name):
    """(cloud, brute-force neighbour rows at k = 64): the first k columns are the rows at any smaller k."""
    pts = nr.FAMILIES[name][1]()
    return pts, nr.knn(pts, max(nr.KS))


@pytest.mark.parametrize("name,k", nr.cases())
def test_every_point_is_within_its_tolerance(name, k):
    pts, wide = family(name)
    got = estimate(pts, k)
    assert_within_tau(got, pts, wide[:, :k], f"{name} k={k}", min_examined=1.0 - nr.LEFT_OUT_CAP)


def test_both_slots_and_every_grid_choice():
    """One cloud P as cloud 0 and as cloud 1, beside a partner of half its size, of its size, of more than twice its size (P gets
    cells of its own: the solo branch) and one shifted by 0.75 of the box (the pair's grid is mostly the partner's).  The grid the
    search ran on is read back to show which branch ran."""
    k = 30
    rng = np.random.default_rng(33)
    pts = nr.volume(4000, 31)
    nbr = nr.knn(pts, k)
    partners = {
        "half": rng.random((2000, 3)),
        "same": rng.random((4000, 3)),
        "large": rng.random((9000, 3)) * 1.5 - 0.25,
        "shifted": rng.random((4000, 3)) + np.array([0.75, 0.0, 0.0]),
    }
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    results = []
    for name, partner in partners.items():
        for slot in (0, 1):
            got, (org, h, dim) = estimate(pts, k, partner=partner, slot=slot, geometry=True)
            top = org + h * dim
            both_lo, both_hi = np.minimum(lo, partner.min(axis=0)), np.maximum(hi, partner.max(axis=0))
            if name == "large":                                   # cells over P alone
                assert len(partner) > 2 * len(pts)
                assert np.array_equal(org, lo) and np.allclose(top, hi, rtol=1e-9)
                assert np.any(both_hi - both_lo > 1.4 * (hi - lo))
            else:                                                 # the pair's grid, over both clouds
                assert np.array_equal(org, both_lo) and np.allclose(top, both_hi, rtol=1e-9)
            if name == "shifted":
                assert top[0] - org[0] > 1.7 * (hi[0] - lo[0])
            assert_within_tau(got, pts, nbr, f"slot {slot}, partner {name}")
            results.append(got)
    assert len(results) == 8
    for first, second in zip(results[0::2], results[1::2]):       # same partner, same grid, either slot: the same bits (across
        assert np.array_equal(first.view(np.uint64), second.view(np.uint64))   # grids a point may change its stage, and its sums)


def test_every_stage_of_the_search_holds_the_tolerance():
    """FAMILIES["staged"] at k = 30: every point is classified on the host by the stop rule restated on the grid the search ran
    on, each stage must hold a minimum of points, and the tolerance is asserted stage by stage."""
    k = 30
    pts, wide = family("staged")
    got, (org, h, dim) = estimate(pts, k, geometry=True)
    stage = stages.classify(pts, pts, org, h, dim, k)
    counts = {s: int(np.sum(stage == s)) for s in stages.STAGES}
    print("grid", org, h, dim, {stages.STAGES[s]: c for s, c in counts.items()})
    assert counts[stages.WAVE2] >= 30 and counts[stages.WAVE3] >= 30
    assert counts[stages.THREAD_CAP] >= 30 and counts[stages.FULL] >= 20
    # the points meant for a stage are in it: the clump is handed on for its crowd, the isolated points are left to the full scan
    clump = np.linalg.norm(pts - 0.5, axis=1) <= 1e-4
    assert clump.sum() > stages.constant("kWCap") and np.all(stage[clump] == stages.THREAD_CAP)
    far = pts[:, 2] > 6.0
    assert 20 <= far.sum() < k and np.all(stage[far] == stages.FULL)
    for s, name in stages.STAGES.items():
        rows = np.flatnonzero(stage == s)
        if len(rows):
            ok = assert_within_tau(got, pts, wide[:, :k], name, rows=rows, min_examined=0.9)
            assert ok.sum() >= min(len(rows), 20)


def test_more_than_one_trip_of_the_wave_loop():
    """200 000 points: the wave kernel's 16384 blocks of 4 waves take 65536 points per trip of the grid-stride loop, so the
    cell-sorted records from 196608 on are settled in a fourth trip.  Neighbours by the blocked brute force of
    knn_stages.blocked_rows.  The rows of the last trip are found from the grid and examined on their own."""
    n, k = 200_000, 30
    pts = np.random.default_rng(71).random((n, 3))
    nbr = stages.blocked_rows(pts, pts, k)
    got, (org, h, dim) = estimate(pts, k, geometry=True)
    assert_within_tau(got, pts, nbr, f"n={n}")
    per_trip = 16384 * 4
    assert n > per_trip
    cells = stages.cells_of(pts, org, h, dim)
    dim = dim.astype(np.int64)
    linear = (cells[:, 2] * dim[1] + cells[:, 1]) * dim[0] + cells[:, 0]       # the order of the cell-sorted records
    population = np.bincount(linear, minlength=int(np.prod(dim)))
    before = np.cumsum(population) - population                                # records in front of each cell
    last = np.flatnonzero(before[linear] >= (n - 1) // per_trip * per_trip)    # whole cells behind the last trip's first record
    tail = n - (n - 1) // per_trip * per_trip
    assert (n - 1) // per_trip >= 1 and len(last) >= tail // 10
    ok = assert_within_tau(got, pts, nbr, f"n={n}, last trip", rows=last)
    assert ok.sum() >= tail // 10


@pytest.mark.parametrize("n,k", [(3, 30), (4, 30), (29, 30), (30, 30), (31, 30), (3, 3)])
def test_small_clouds(n, k):
    pts = np.random.default_rng(100 + n).random((n, 3))
    got = estimate(pts, k, partner=pts)
    assert_within_tau(got, pts, nr.knn(pts, k), f"n={n} k={k}", min_examined=1.0)
    if n <= k:                                                    # every point has the whole cloud: one normal
        assert np.all(nr.angle(got, np.tile(got[0], (n, 1))) < 2 * nr.TAU_MAX)


def test_collinear_points_and_the_bounds_of_k():
    e = nat.Engine(0)
    try:
        line = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
        e.set_cloud(0, line)
        e.set_cloud(1, line)
        for k in (3, 30):
            e.estimate_normals(0, k)
            assert np.array_equal(e.get_normals(0), np.tile([0.0, 0.0, 1.0], (3, 1)))   # degenerate covariance: the default
        lib = nat.load()
        for k in (2, 65):
            assert lib.pccm_estimate_normals(e._ctx, 0, k) == nat.E_ARG
            with pytest.raises(ValueError):
                e.estimate_normals(1, k)
        for k in (3, 64):
            assert lib.pccm_estimate_normals(e._ctx, 0, k) == nat.OK
    finally:
        e.close()


def test_point_to_plane_report_with_normals_of_twelve_neighbours():
    a = surface(6000, 15)
    b = a + np.random.default_rng(16).normal(0, 0.003, a.shape)
    pair = CloudPair(PointCloud(a), PointCloud(b), extent=[2, 2, 1], normals_knn=12)      # no normals given
    res = MetricCalculator(pair).calculate(transform_options(CalculateOptions(None, True, True))).as_dict()
    na, _ = orc.estimate_normals(a, 12)
    nb, _ = orc.estimate_normals(b, 12)
    want = orc.OraclePair(a, b, na, nb, method="kdtree").report(hausdorff=True, point_to_plane_=True, peak=2.0)
    for key, val in want.items():
        assert res[key] == pytest.approx(val, rel=1e-9), key
    n30, _ = orc.estimate_normals(a, 30)                          # k matters: the report at 30 is another one
    other = orc.OraclePair(a, b, n30, orc.estimate_normals(b, 30)[0], method="kdtree").report(hausdorff=True, point_to_plane_=True, peak=2.0)
    assert any(other[key] != pytest.approx(val, rel=1e-6) for key, val in want.items())
