"""The yardstick of the PointSSIM normal and curvature tests, checked without a GPU: the high-precision reference of
tests/pointssim_tolerance.py against itself (how many points it leaves out, whether the recorded K_MEASURED is what this machine
measures), the fp64 restatement of the kernel's Jacobi curvature against the tolerance, the restatement of the closed form the
kernel used before -- which must be CAUGHT on collinear neighbourhoods --, and the tolerance's power to see wrong kernels."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import normals_reference as nr  # noqa: E402
import pointssim_reference as ref  # noqa: E402
import pointssim_tolerance as pt  # noqa: E402


@functools.lru_cache(maxsize=None)
def measured(name, k):
    return pt.measure(name, k)


def test_the_cases_are_the_issue_s():
    assert pt.KS == (2, 3, 5, 12, 64) and pt.TAU_MAX == 1e-6 and pt.LEFT_OUT_CAP == 0.02 and pt.T_N == 4 * 2.0 ** -52
    assert set(pt.FAMILIES) == {"uniform", "surface", "duplicates", "lattice", "wires", "rings", "shell", "georeferenced"}
    assert pt.K_C == 16.0 and pt.K_C >= 19 * pt.K_MEASURED              # the margin over the measurement
    assert pt.K_C >= 31 * sorted(m[0] for m in pt.MEASURED.values())[-2]  # ... and over every family but the rings
    assert set(pt.MEASURED) == set(pt.FAMILIES)
    assert max(m[0] for m in pt.MEASURED.values()) == pt.K_MEASURED
    assert np.finfo(np.longdouble).eps < 2.0 ** -60


def test_the_first_four_families_are_those_of_the_gpu_suite():
    """The points of test_gpu_pointssim.DATA and the file normals of its sheet, drawn again (that module needs the package)."""
    rng = np.random.default_rng(3)
    uv = rng.random((3000, 2))
    z = 0.1 * np.sin(6.0 * uv[:, 0]) * np.cos(4.0 * uv[:, 1]) + rng.normal(0, 0.01, 3000)
    nrm = np.column_stack([-0.6 * np.cos(6.0 * uv[:, 0]) * np.cos(4.0 * uv[:, 1]),
                           0.4 * np.sin(6.0 * uv[:, 0]) * np.sin(4.0 * uv[:, 1]), np.ones(3000)]) + rng.normal(0, 0.05, (3000, 3))
    (a, na), (b, nb) = pt.FAMILIES["surface"][1]()
    assert np.array_equal(a, np.column_stack([uv, z]).astype(np.float32).astype(np.float64)) and np.array_equal(na, nrm)
    assert len(b) == 2800 and nb.shape == (2800, 3)
    (u, none), _ = pt.FAMILIES["uniform"][1]()
    assert none is None and np.array_equal(u, np.random.default_rng(1).random((3000, 3), dtype=np.float32).astype(np.float64))


@pytest.mark.parametrize("name,k", pt.cases())
def test_left_out_share_measurement_and_restatements(name, k):
    """Per (family, k), on the reference alone: at most 2 % of the points are left out, per attribute; pointssim_reference's
    curvature needs no more of the tolerance than recorded; the restatement of the kernel's Jacobi curvature is within the
    tolerance with a factor 16 to spare on the values, and within it on features and similarities; and the closed form the
    kernel used before is outside it on the wires at every k and on every family at k = 2."""
    r = measured(name, k)
    print(name, k, r)
    for attribute in pt.ATTRIBUTES:
        assert r["left_out"][attribute] <= pt.LEFT_OUT_CAP
        assert r["left_out"][attribute] <= pt.MEASURED[name][2] + 1e-4 and r["tau_s"][attribute] <= 1.01 * pt.MEASURED[name][3]
        assert r[attribute]["feature"]["jacobi"] <= 1.0 and r[attribute]["similarity"]["jacobi"] <= 1.0
        assert r[attribute]["outside"]["jacobi"] == 0.0
    assert r["ratio"]["c64"] <= pt.MEASURED[name][0] + 5e-4 <= pt.K_MEASURED + 5e-4
    assert r["ratio"]["jacobi"] <= pt.MEASURED[name][1] + 5e-4 and r["ratio"]["jacobi"] <= pt.K_C / 16.0
    if name == "wires" or k == 2:                                        # the finding is caught
        assert r["ratio"]["closed"] > 1e4 * pt.K_C                        # a curvature of 1e-9 where the tolerance is 1e-14
        assert r["curvature"]["feature"]["closed"] > 1e4
        assert r["curvature"]["outside"]["closed"] > 0.03                 # similarities outside tau_s (wires, k >= 3: > 98 %)
        if name == "wires" and k >= 3:
            assert r["curvature"]["outside"]["closed"] > 0.98


def test_k_measured_is_reproduced():
    worst = {name: max(measured(name, k)["ratio"]["c64"] for k in pt.KS) for name in pt.FAMILIES}
    for name, w in worst.items():
        assert abs(w - pt.MEASURED[name][0]) <= 5e-4, (name, w)
    assert abs(max(worst.values()) - pt.K_MEASURED) <= 5e-4


@pytest.mark.parametrize("name,attribute,which", sorted(pt.DETECTED))
def test_wrong_kernels_are_seen(name, attribute, which):
    """Curvature features over j >= 1 / normal features with q_0 ("first"), a divisor of m, the k-th neighbour replaced by the
    (k+1)-th and, on the lattice kinds, the tied row at the cut replaced: each moves the feature by more than 2 tau_F at the
    recorded share of the examined points, which is at least pointssim_tolerance.detection_floor()."""
    kind = pt.FAMILIES[name][0]
    for k, recorded in zip(pt.KS, pt.DETECTED[(name, attribute, which)]):
        share = pt.measure_detection(name, k, attribute, which)
        print(name, attribute, which, k, share, recorded)
        assert share is not None and abs(share - recorded) <= 2e-3
        assert share >= pt.detection_floor(kind, k, attribute, which)


def test_every_wrong_kernel_is_recorded_for_every_family():
    for name, (kind, _) in pt.FAMILIES.items():
        for attribute in pt.ATTRIBUTES:
            for which in pt.WRONG:
                assert ((name, attribute, which) in pt.DETECTED) == (which != "tied" or kind == pt.LATTICE)
    # the floors are those of the normal-estimation tests wherever the data does not make the change a no-op
    assert pt.detection_floor(pt.CONTINUOUS, 12, "curvature", "kth") == nr.detection_floor(nr.CONTINUOUS, 12) == 0.98
    assert pt.detection_floor(pt.LATTICE, 12, "normal", "tied") == 0.95 and pt.detection_floor(pt.LATTICE, 5, "normal", "tied") == 0.85


def test_reference_by_hand():
    tile = lambda n: np.tile(np.arange(n), (n, 1))                       # noqa: E731  (every point's neighbourhood: the cloud)
    # all points equal: trace 0, c = 0, rho = 1
    same = np.tile([1.5, -2.0, 3.0], (4, 1))
    c, rho = pt.curvature_reference(same, tile(4))
    assert np.array_equal(c, np.zeros(4)) and np.array_equal(rho, np.ones(4))
    assert np.array_equal(pt.curvatures_jacobi(same, tile(4)), np.zeros(4))
    # the corners of a cube: isotropic, c = 1/3; rho = 1 + |mean d|^2 / trace = 2 for a corner
    cube = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    c, rho = pt.curvature_reference(cube, tile(8))
    assert np.allclose(c, 1.0 / 3.0, rtol=0, atol=1e-15) and np.allclose(rho, 2.0)
    assert np.all(np.abs(pt.curvatures_jacobi(cube, tile(8)) - c) <= pt.curvature_tolerance(rho, 8) / 16)
    # a straight line that is not exact in fp64: c = 0 to the tolerance by Jacobi, some 1e-9 by the closed form
    t = np.random.default_rng(1).random(12)
    line = np.column_stack([0.1 + t / 3.0, 0.7 * t, -t / 7.0])
    c, rho = pt.curvature_reference(line, tile(12))
    tol = pt.curvature_tolerance(rho, 12)
    assert np.all(np.abs(c) <= tol) and np.all(np.abs(pt.curvatures_jacobi(line, tile(12)) - c) <= tol)
    assert np.max(np.abs(pt.curvatures_closed_form(line, tile(12)))) > 1e-10 > 100 * tol.max()
    # ... while on an isotropic plane, the existing suite's case, the closed form is accurate
    plane = np.column_stack([np.random.default_rng(2).random((40, 2)), np.zeros(40)])
    c, rho = pt.curvature_reference(plane, tile(40))
    assert np.all(np.abs(pt.curvatures_closed_form(plane, tile(40)) - c) <= pt.curvature_tolerance(rho, 40))
    # a feature: the values 1, 2, 3, 4 have variance 5/3; errors of 1e-3 each give T = 4e-6 / 3
    F, tF = pt.feature_reference(np.array([[1.0, 2.0, 3.0, 4.0]], dtype=np.longdouble), np.full((1, 4), 1e-3))
    T = 4e-6 / 3
    assert F[0] == pytest.approx(5.0 / 3.0, rel=1e-15)
    assert tF[0] == pytest.approx(2 * np.sqrt(F[0] * T) + T + 7 * pt.EPS * F[0], rel=1e-12)
    moved = np.var(np.array([1.0, 2.0, 3.0, 4.0]) + 1e-3 * np.array([-1, -1, 1, 1]), ddof=1)      # the worst signs
    assert 0.5 * tF[0] < abs(moved - F[0]) <= tF[0]
    assert pt.feature_reference(np.ones((3, 1), dtype=np.longdouble), np.ones((3, 1)))[1].tolist() == [0.0, 0.0, 0.0]
    # a similarity: s = 1 - 1/3, tau_s = 2 (0.1 + 0.2) / (3 + eps) + 4 eps
    s, ts = pt.similarity_reference(np.array([2.0]), np.array([0.1]), np.array([7.0, 3.0]), np.array([0.5, 0.2]), [1])
    assert s[0] == ref.similarity(np.array([2.0]), np.array([3.0]))[0] and ts[0] == pytest.approx(0.2 + 4 * pt.EPS, rel=1e-12)
    # normal values: the longdouble acos against np.arccos, within t_n; perpendicular 0, parallel and antiparallel 1
    nrm = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.6, 0.0, 0.8], [0.0, 0.0, 0.0]])
    v = pt.normal_values_reference(nrm, tile(5))[0]
    assert [float(x) for x in v[:2]] == [1.0, 0.0] and float(v[3]) == 0.0
    assert abs(float(v[2]) - (1 - 2 * np.arccos(0.8) / np.pi)) <= pt.T_N
    got = ref.features(np.zeros((5, 3)), 5, "normal", nrm, nbr=tile(5))
    want, tol = pt.reference_features(np.zeros((5, 3)), tile(5), "normal", nrm)
    assert np.all(np.abs(got - want) <= tol)


def test_the_new_families_are_what_they_are_for():
    (w, _), _ = pt.FAMILIES["wires"][1]()
    assert w.dtype == np.float64 and np.array_equal(w, w.astype(np.float32))
    nbr = pt.neighbours(w[:3000], 64)
    c, _ = pt.curvature_reference(w, nbr)
    assert np.max(np.abs(c)) < 1e-10                                     # collinear to the rounding of fp32, at k = 64 too
    (r, _, wide), _, _, _ = pt.load("rings")
    lam = np.linalg.eigvalsh(np.einsum("nki,nkj->nij", *(2 * [r[wide[:, :6]] - r[wide[:, :6]].mean(axis=1, keepdims=True)])))
    assert np.median(lam[:, 1] / lam[:, 2]) < 0.05 and np.median(lam[:, 0] / lam[:, 1]) > 0.05   # a line, noise of one size across
    (s, _), _ = pt.FAMILIES["shell"][1]()
    assert np.array_equal(s, np.round(s)) and len(s) <= 5000
    (g, _), _ = pt.FAMILIES["georeferenced"][1]()
    assert np.abs(g).max() > 1e6 and np.ptp(g, axis=0).max() < 50


def test_sampled_features_are_the_rows_of_the_full_reference():
    (x, normals, wide), _, _, _ = pt.load("lattice")
    rows = np.sort(np.random.default_rng(5).choice(len(x), 200, replace=False))
    for attribute in pt.ATTRIBUTES:
        F, tF = pt.reference_features(x, wide[:, :12], attribute, normals)
        Fs, ts = pt.sampled_features(x, rows, 12, attribute, normals, lambda r: ref.tree_rows(x[r], x, 12))
        assert np.array_equal(Fs, F[rows]) and np.array_equal(ts, tF[rows])
