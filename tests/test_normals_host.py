"""The yardstick of the normal-estimation tests, checked without a GPU: the high-precision reference of
tests/normals_reference.py against itself (how many points it leaves out, whether the fp64 restatement of the kernel's closed
form stays inside the tolerance with the recorded K, whether both brute-force neighbour sources agree), the tolerance's power to
see one wrong neighbour, and the stage classifier of tests/knn_stages.py on grids built by hand."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_stages as stages  # noqa: E402
import normals_reference as nr  # noqa: E402
import p2d_reference as ref  # noqa: E402
from oracle import oracle as orc  # noqa: E402


@functools.lru_cache(maxsize=None)
def family(name):
    """(cloud, neighbour rows at k = 65): the first k columns are the neighbourhood at k, column k the next one out."""
    p = nr.FAMILIES[name][1]()
    return p, nr.knn(p, max(nr.KS) + 1)


# ---- the reference checks itself ------------------------------------------------------------------------------------------------
def test_the_cases_are_the_issue_s():
    assert nr.KS == (3, 5, 12, 30, 64) and nr.K == 16.0 and nr.TAU_MAX == 1e-6 and nr.LEFT_OUT_CAP == 0.02
    assert set(nr.FAMILIES) == {"sheet", "volume", "lattice", "ellipsoid", "georeferenced", "duplicates", "staged"}
    for name, (kind, _) in nr.FAMILIES.items():
        assert nr.ks_of(name) == (nr.KS if kind == nr.CONTINUOUS else nr.KS[1:])
    assert nr.K >= 30 * nr.K_MEASURED                             # the margin over the measurement
    assert set(nr.MEASURED) == set(nr.FAMILIES)
    assert max(m[0] for m in nr.MEASURED.values()) == nr.K_MEASURED


@pytest.mark.parametrize("name,k", nr.cases())
def test_left_out_share_closed_form_and_detection(name, k):
    """Per (family, k), on the reference alone: at most 2 % of the points are left out; the fp64 restatement of the kernel's
    closed form is within tau at every examined point, by the margin K was given over the measurement; and one wrong neighbour
    moves the normal by more than 2 tau at the share of the points detection_floor() states."""
    kind = nr.FAMILIES[name][0]
    p, wide = family(name)
    r = nr.measure(name, k, wide[:, :k + 1], p)
    print(f"{name} k={k} n={len(p)}: ratio {r['ratio']:.3f} (K = {nr.K}), left out {r['left_out']:.4f}, "
          f"k-th swapped seen at {r['detect_kth']:.4f}, tied swapped at {r['detect_tied']}")
    assert r["left_out"] <= nr.LEFT_OUT_CAP
    assert r["ratio"] <= nr.K / 16.0                              # under tau with a factor 16 to spare for the device
    assert r["ratio"] <= 1.25 * nr.MEASURED[name][0]              # the recorded maxima are what this machine measures
    floor = nr.detection_floor(kind, k)
    assert r["detect_kth"] >= floor
    if kind == nr.LATTICE:
        assert r["detect_tied"] is not None and r["detect_tied"] >= floor
    if name == "georeferenced":
        assert np.abs(p).max() > 1e6 and np.ptp(p, axis=0).max() < 50


def test_a_wrong_sum_is_seen_too():
    """A covariance that drops one neighbour's contribution (a lane's partial sum lost) is outside tau almost everywhere."""
    p, wide = family("volume")
    for k in (5, 30):
        want, _, _, tau = nr.reference(p, wide[:, :k])
        short = nr.reference(p, wide[:, 1:k])[0]                  # the query itself left out of its neighbourhood
        ok = nr.examined(tau)
        assert np.mean(nr.angle(short, want)[ok] > 2 * tau[ok]) >= 0.98


def test_both_neighbour_sources_agree_where_distances_tie():
    p, wide = family("lattice")
    d2 = np.sort(ref.sq_dist(p[:200, None, :], p[None, :, :]), axis=1)
    for k in (5, 30):
        assert np.mean(d2[:, k - 1] == d2[:, k]) > 0.5            # the data has ties at the cut
        assert np.array_equal(orc.knn(p, k), wide[:, :k])
    p, wide = family("duplicates")
    assert np.array_equal(orc.knn(p, 12), wide[:, :12])
    assert np.array_equal(wide[:, 0] != np.arange(len(p)), wide[:, 0] < np.arange(len(p)))   # a copy with a smaller row comes first


def test_reference_by_hand():
    # a tilted plane x + 2y + 2z = 3 and one point off it: the normal is the plane's to first order in the offset
    rng = np.random.default_rng(1)
    uv = rng.random((40, 2))
    plane = np.column_stack([uv, (3.0 - uv[:, 0] - 2.0 * uv[:, 1]) / 2.0])
    nbr = np.tile(np.arange(40), (40, 1))
    n, w, kappa, tau = nr.reference(plane, nbr)
    assert np.all(nr.angle(n, np.tile([1 / 3, 2 / 3, 2 / 3], (40, 1))) < 1e-12)
    assert np.all(np.abs(w[:, 0]) < 1e-16) and np.all(nr.examined(tau))
    assert np.all(nr.angle(nr.closed_form_normals(plane, nbr), n) < tau)
    lead = nr.closed_form_normals(plane, nbr)
    assert np.all(lead[np.arange(40), np.argmax(np.abs(lead), axis=1)] > 0)
    # isotropic and rank-1 neighbourhoods have no normal: infinite kappa or a tau beyond TAU_MAX
    cube = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    assert not np.any(nr.examined(nr.reference(cube, np.tile(np.arange(8), (8, 1)))[3]))
    line = np.column_stack([np.arange(5.0), 2 * np.arange(5.0), -np.arange(5.0)])
    assert not np.any(nr.examined(nr.reference(line, np.tile(np.arange(5), (5, 1)))[3]))
    # (the closed form gives the default normal where the spread is EXACTLY rank 1 -- points along an axis -- and some vector
    # across the line, all of which are eigenvectors of the double eigenvalue 0, where rounding leaves a residue)
    along_x = np.column_stack([np.arange(3.0), np.zeros(3), np.zeros(3)])
    assert np.array_equal(nr.closed_form_normals(along_x, np.tile(np.arange(3), (3, 1))), np.tile([0.0, 0.0, 1.0], (3, 1)))
    across = nr.closed_form_normals(line[:3], np.tile(np.arange(3), (3, 1)))
    assert np.all(np.abs(across @ np.array([1.0, 2.0, -1.0])) < 1e-12)
    # fewer than three neighbours: the default normal, nothing examined
    n, _, _, tau = nr.reference(cube[:2], np.tile(np.arange(2), (2, 1)))
    assert np.array_equal(n, [[0, 0, 1], [0, 0, 1]]) and not np.any(nr.examined(tau))
    # the angle is taken on the line, not the arrow, and does not saturate the way 1 - cos does
    a = np.array([[1.0, 0.0, 0.0]])
    assert nr.angle(a, -a)[0] == 0.0 and nr.angle(a, np.array([[1.0, 1e-12, 0.0]]))[0] == pytest.approx(1e-12, rel=1e-9)


def test_swaps_by_hand():
    wide = np.array([[0, 1, 2, 3, 4], [1, 0, 2, 4, 3]])
    assert nr.swap_kth(wide, 3).tolist() == [[0, 1, 3], [1, 0, 4]]
    # rows 1..4 are all at distance 1 from row 0; k = 3 keeps rows 1, 2: the swap puts row 4 in place of row 1
    p = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [5, 5, 5], [5, 5, 6], [5, 6, 5]])
    nbr = nr.knn(p, 3)
    assert nbr[0].tolist() == [0, 1, 2]
    rows, lists = nr.swap_tied(p, nbr)
    assert 0 in rows and lists[list(rows).index(0)].tolist() == [0, 4, 2]
    assert 5 not in rows                                          # no tie across the cut there (its 3rd and 4th differ)


# ---- the stage classifier on grids built by hand ---------------------------------------------------------------------------------
def hand_grid():
    """A 20 x 20 x 20 grid of unit cells over [0, 20]^3 with one point in the middle of each cell of the slab z < 12, a crowd of
    600 points inside the cell (5, 5, 5), and nothing above z = 12 but one point in the cell (10, 10, 19)."""
    g = np.arange(20) + 0.5
    x, y, z = np.meshgrid(g, g, g[:12], indexing="ij")
    slab = np.column_stack([x.ravel(), y.ravel(), z.ravel()])
    rng = np.random.default_rng(0)
    crowd = np.array([5.5, 5.5, 5.5]) + (rng.random((600, 3)) - 0.5) * 0.2
    lone = np.array([[10.5, 10.5, 19.5]])
    return np.concatenate([slab, crowd, lone]), np.zeros(3), np.ones(3), np.array([20, 20, 20])


def test_stage_classifier_on_synthetic_grids():
    b, org, h, dim = hand_grid()
    kw = dict(wcap=512, max_ring=6)
    crowded = np.array([[5.5, 5.5, 5.5], [7.4, 5.5, 5.5]])        # the crowd is inside their 5^3 cubes: more than 512 candidates
    assert stages.classify(crowded, b, org, h, dim, 30, **kw).tolist() == [stages.THREAD_CAP] * 2
    # three cells away the crowd enters at r = 3 only: r = 2 (125 candidates, 30th at sqrt(3) < 2.5) has settled it before
    assert stages.classify(np.array([[8.5, 5.5, 5.5]]), b, org, h, dim, 30, **kw).tolist() == [stages.WAVE2]
    # ... unless k asks for more than r = 2 can prove: the 64th neighbour of a lattice point lies at d2 = 6 < 2.5^2, the 100th at
    # d2 = 9 > 2.5^2, so r = 2 cannot settle k = 100; (this classifier takes any k, the kernels stop at 64)
    assert stages.classify(np.array([[14.5, 14.5, 5.5]]), b, org, h, dim, 64, **kw).tolist() == [stages.WAVE2]
    assert stages.classify(np.array([[14.5, 14.5, 5.5]]), b, org, h, dim, 100, **kw).tolist() == [stages.WAVE3]
    # an empty neighbourhood: the lone point's cubes hold fewer than k points up to r = 6 (the slab ends at cell z = 11 = 19 - 8)
    assert stages.classify(b[-1:], b, org, h, dim, 30, **kw).tolist() == [stages.FULL]
    # 5 rings below it, the slab's top is 2 rings away: r = 2 and 3 see too little, r = 4 .. 6 settle
    assert stages.classify(np.array([[10.5, 10.5, 14.5]]), b, org, h, dim, 30, **kw).tolist() == [stages.THREAD_RINGS]
    # at the grid's face and corner the cube's outer faces are the grid's and do not count: the corner query has 27 points
    # in its r = 2 cube -- fewer than 30 -- and settles at r = 3 (64 points, 30th at d2 <= 9 < 3.5^2)
    assert stages.classify(np.array([[0.5, 0.5, 0.5]]), b, org, h, dim, 30, **kw).tolist() == [stages.WAVE3]
    assert stages.classify(np.array([[0.5, 0.5, 0.5]]), b, org, h, dim, 20, **kw).tolist() == [stages.WAVE2]
    assert stages.face_bound(np.array([0.5, 0.5, 0.5]), np.array([0, 0, 0]), 2, org, h, dim) == pytest.approx(2.5, abs=1e-9)
    assert stages.face_bound(np.array([0.5, 0.5, 0.5]), np.array([0, 0, 0]), 19, org, h, dim) == np.inf
    # a query outside the grid clamps into the boundary cell
    assert stages.cells_of(np.array([[-3.0, 25.0, 4.2]]), org, h, dim).tolist() == [[0, 19, 4]]


def test_a_grid_of_one_cube_settles_everything_at_once():
    rng = np.random.default_rng(2)
    b = rng.random((40, 3))
    got = stages.classify(b, b, np.zeros(3), np.full(3, 0.25 * (1 + 2.0 ** -40)), np.array([4, 4, 4]), 30, wcap=512, max_ring=6)
    # every cube [c - 2, c + 2] of a 4-cell axis leaves a face inside the grid unless c is 1 or 2 ... r = 3 always covers it
    assert set(got.tolist()) <= {stages.WAVE2, stages.WAVE3}
    fewer = stages.classify(b[:5], b[:5], np.zeros(3), np.full(3, 0.25 * (1 + 2.0 ** -40)), np.array([4, 4, 4]), 30, wcap=512, max_ring=6)
    assert set(fewer.tolist()) <= {stages.WAVE2, stages.WAVE3}    # fewer than k points in all: the covering cube takes them all


def test_settles_agrees_with_classify():
    b, org, h, dim = hand_grid()
    cells = stages.cells_of(b, org, h, dim)
    rng = np.random.default_rng(3)
    queries = np.concatenate([rng.random((30, 3)) * [20, 20, 12], rng.random((10, 3)) * 20])
    got = stages.classify(queries, b, org, h, dim, 30, wcap=10 ** 9, max_ring=6)      # (no cap: the rule alone)
    for q, s in zip(queries, got):
        assert stages.settles(q, b, cells, org, h, dim, 30, 2) == (s == stages.WAVE2)
        assert stages.settles(q, b, cells, org, h, dim, 30, 3) == (s in (stages.WAVE2, stages.WAVE3))
        assert stages.settles(q, b, cells, org, h, dim, 30, 6) == (s != stages.FULL)


def test_constants_are_read_from_the_kernel_source():
    assert stages.constant("kWCap") == 512 and stages.constant("kKnnMaxRing") == 6 and stages.constant("kKnnMax") == 64
