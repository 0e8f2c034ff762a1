"""Density-aware Chamfer rows on the GPU (include/pccm.h: pccm_match_counts, pccm_reduce_density_total_many;
CalculateOptions(dcd=..., dcd_squared=...)): the match counts made by the carry's count pass, the terms gathered and mapped by the
density mode of the general reduction kernel, no column stored.

Comparison rule.  The two sides -- the device and the NumPy restatement of tests/dcd_reference.py -- differ only through exp.  At
alpha 0 and 1e300 exp is exactly 1 or 0 on both, so those rows are compared with ``==`` on float64 bits; at 1 / max(d) and
1 / median(d) (d: the unsquared left column -- they keep exp away from 0 and 1, so that a wrong count or a wrong row moves a row
by far more than the tolerance) within ATOL = 2^-40, derived in dcd_reference.py.  Every comparison is made twice: against the
restatement on the oracle's kd-tree idx and d2, and on the GPU's own fetched idx and d2.  The largest deviation each test meets is
printed (pytest -s shows it)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
from click.testing import CliRunner

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair, DeviceColumn, DeviceRows
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import write_point_cloud
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dcd_reference as ref  # noqa: E402
import variant_rows as vr  # noqa: E402
from test_gpu_ties_mean import lattice_pair  # noqa: E402

EXACT = (0.0, 1e300)
WORST = [0.0]       # the largest deviation of an inexact row seen so far in this process


def same(x, y):
    return np.float64(x).tobytes() == np.float64(y).tobytes()


def close(got, want, alpha, what):
    """The comparison rule: bits at the exact alphas, ATOL elsewhere."""
    if alpha in EXACT:
        assert same(got, want), (what, alpha, got, want)
        return
    dev = abs(float(got) - float(want))
    WORST[0] = max(WORST[0], dev)
    assert dev <= ref.ATOL, (what, alpha, got, want, dev)


def report(pair, alphas, squared=False, **kw):
    opts = CalculateOptions(kw.pop("color", None), kw.pop("hausdorff", False), kw.pop("p2plane", False), dcd=alphas or None,
                            dcd_squared=squared, **kw)
    with np.errstate(divide="ignore"):
        return MetricCalculator(pair).calculate(transform_options(opts)).as_dict()


def oracle_nn(a, b):
    """((left idx, left d2), (right idx, right d2)) of the kd-tree oracle."""
    return orc.nn(a, b, method="kdtree"), orc.nn(b, a, method="kdtree")


def own_nn(pair):
    eng = pair._engine
    return eng.fetch_nn(nat.DIR_LEFT), eng.fetch_nn(nat.DIR_RIGHT)


def alphas_of(left_d2):
    """0, 1 / max(d), 1 / median(d), 1e300 for the unsquared left column d (fewer where two of them coincide)."""
    d = np.sqrt(np.asarray(left_d2, dtype=np.float64))
    top, mid = float(np.max(d)), float(np.median(d))
    return ref.alphas_of([0.0, 1e300] + [1.0 / x for x in (top, mid) if x > 0])


def check_rows(res, nn, n0, n1, alphas, squared, what):
    """The new rows of a report -- the last ones, in the stated order -- against the restatement over a pair of search results."""
    (li, ld), (ri, rd) = nn
    want = ref.rows(ld, rd, li, ri, n0, n1, alphas, squared)
    assert list(res)[-len(want):] == list(want)
    for key, value in want.items():
        close(res[key], value, key[-2], (what, key))
        assert 0.0 <= res[key] <= 1.0, key


def check_counts(pair, own, n0, n1):
    for is_left, (idx, _), n_it, n_se in ((True, own[0], n0, n1), (False, own[1], n1, n0)):
        got = pair.match_counts(is_left)
        assert got.dtype == np.uint32 and got.shape == (n_se,)
        assert np.array_equal(got, np.bincount(idx, minlength=n_se)) and int(got.sum(dtype=np.int64)) == n_it


def uniform(n, m, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3)).astype(np.float32), rng.random((m, 3)).astype(np.float32)


# ---- uniform fp32 pairs, both engines -----------------------------------------------------------------------------------------
# one wave and one wave plus one row onto a single target (64, 65 against 1), the 128-row leaf edge, the 8192-row chunk edge,
# unequal sizes, several chunks.  The seeds are tie-free: the GPU's smallest-row pick and the kd-tree's agree (asserted below);
# up to 20000 points that was also checked on the CPU against the oracle's brute-force search.
@functools.lru_cache(maxsize=16)
def uniform_case(n, m):
    a, b = uniform(n, m, 11 * n + m)
    return a, b, oracle_nn(a, b)


@pytest.mark.parametrize("engine", ["grid", "brute"])
@pytest.mark.parametrize("n, m", [(1, 1), (2, 2), (64, 1), (65, 1), (127, 127), (129, 129), (8191, 8191), (8193, 8193), (300, 200),
                                  (5000, 4097), (20000, 20000), (100_003, 100_003)])
def test_uniform_pairs(n, m, engine):
    a, b, nn = uniform_case(n, m)
    alphas = alphas_of(nn[0][1])
    with CloudPair(PointCloud(a), PointCloud(b), extent=[1.0, 1.0, 1.0], nn_engine=engine) as pair:
        res = report(pair, alphas)
        sq = report(pair, alphas, squared=True)
        own = own_nn(pair)
        check_counts(pair, own, n, m)
    assert np.array_equal(own[0][0], nn[0][0]) and np.array_equal(own[1][0], nn[1][0])      # tie-free: one idx
    for got, squared in ((res, False), (sq, True)):
        check_rows(got, nn, n, m, alphas, squared, "oracle")
        check_rows(got, own, n, m, alphas, squared, "own")
    for is_left in (True, False):                                  # at alpha = 0 the two conventions are the same bits
        assert same(res[(ref.SIDE, is_left, 0.0, False)], sq[(ref.SIDE, is_left, 0.0, True)])
    print(f"dcd deviation uniform {n} {m} {engine}: {WORST[0]!r}")


# ---- every record form, through the engine (ABI) -------------------------------------------------------------------------------
def density_requests(alphas, squared):
    return [(d, a, squared) for d in (0, 1) for a in alphas]


def check_totals(got, reqs, nn, n0, n1, what):
    for g, (d, alpha, squared) in zip(got, reqs):
        idx, d2 = nn[d]
        want = ref.totals(d2, idx, n1 if d == 0 else n0, alpha, squared)
        if alpha in EXACT:
            assert all(same(x, y) for x, y in zip(g, want)), (what, d, alpha, squared, g, want)
        else:              # the tolerance is the rows': the sum over n is compared as the mean it becomes, min and max as they are
            close(g[0] / len(d2), want[0] / len(d2), alpha, (what, d, alpha, squared))
            close(g[1], want[1], alpha, (what, d, alpha, squared, "min"))
            close(g[2], want[2], alpha, (what, d, alpha, squared, "max"))
        assert 0.0 <= g[1] <= g[2] <= 1.0, (what, g)               # min and max of the terms lie in [0, 1]


@pytest.mark.parametrize("f64", [False, True], ids=["fp32-exact", "fp64"])
def test_every_record_form_is_gathered_as_it_is_reduced(f64):
    """fp32-exact clouds leave matched records whose rows are read in place; fp64 clouds that are not fp32-exact 32-byte pair
    records; nn_want_idx(False) 16-byte pair records without rows, so the search repeats; the brute-force engine plain columns.
    With and without the projection fused; eight requests per call; prefetched behind the caller's own reductions and not."""
    n, m = 20_011, 17_001
    rng = np.random.default_rng(3)
    a, b = rng.random((n, 3)), rng.random((m, 3))
    if not f64:
        a, b = a.astype(np.float32), b.astype(np.float32)
    else:
        assert not np.array_equal(a, a.astype(np.float32).astype(np.float64))
    nn = oracle_nn(a, b)
    alphas = [x for x in alphas_of(nn[0][1]) if x not in EXACT] + [0.0, 1e300]
    assert len(alphas) == 4
    req, req_sq = density_requests(alphas, False), density_requests(alphas, True)
    assert len(req) == 8
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, a); eng.set_cloud(1, b)
        eng.set_normals(0, vr._unit(n, 7, f64)); eng.set_normals(1, vr._unit(m, 8, f64))
        for engine in ("grid", "brute"):
            for want_idx in (True, False):
                for turn, fuse in enumerate(("neighbour", None)):
                    what = f"{engine} f64={f64} idx={want_idx} fuse={fuse}"
                    for d in (0, 1):
                        eng.nn_fuse(d, fuse)
                    eng.nn_want_idx(want_idx)
                    eng.drop_caches()
                    eng.nn_pair(engine)
                    if turn:                                       # behind reductions enqueued by the caller, or on its own
                        eng.reduce_prefetch_many([(0, nat.METRIC_D1), (0, nat.METRIC_D2), (1, nat.METRIC_D1), (1, nat.METRIC_D2)], "neighbour")
                        eng.reduce_density_prefetch_many(req)
                    got, got_sq = eng.reduce_density_total_many(req), eng.reduce_density_total_many(req_sq)
                    assert "k_unit_jobs" in eng.last_path(nat.PATH_REDUCE), what
                    own = (eng.fetch_nn(0), eng.fetch_nn(1))
                    assert np.array_equal(own[0][0], nn[0][0]) and np.array_equal(own[1][0], nn[1][0]), what
                    assert np.array_equal(own[0][1], nn[0][1]) and np.array_equal(own[1][1], nn[1][1]), what
                    for d, n_se in ((0, m), (1, n)):
                        counts = eng.match_counts(d)
                        assert counts.dtype == np.uint32 and np.array_equal(counts, np.bincount(own[d][0], minlength=n_se)), what
                    check_totals(got, req, nn, n, m, what)
                    check_totals(got_sq, req_sq, nn, n, m, what)
                    # the plain totals of the columns the maps read are what they are without them
                    plain = eng.reduce_total_many([(0, nat.METRIC_D1), (1, nat.METRIC_D1)])
                    assert same(plain[0][0], np.sum(nn[0][1])) and same(plain[1][0], np.sum(nn[1][1])), what
    finally:
        eng.close()
    print(f"dcd deviation record forms f64={f64}: {WORST[0]!r}")


def test_voxelised_integer_pair():
    """Exact ties are everywhere on this pair and the oracle's tie order is nanoflann's, not the smallest row: d2 is compared with
    the oracle, the counts and the rows with the restatement on the GPU's own idx only."""
    n = 20000
    rng = np.random.default_rng(29)
    a = np.unique(rng.integers(0, 64, (n, 3)), axis=0).astype(np.float32)
    b = np.unique(rng.integers(0, 64, (n, 3)), axis=0).astype(np.float32)
    nn = oracle_nn(a, b)
    alphas = alphas_of(nn[0][1])
    with CloudPair(PointCloud(a), PointCloud(b), extent=[64.0, 64.0, 64.0]) as pair:
        res = report(pair, alphas)
        sq = report(pair, alphas, squared=True)
        own = own_nn(pair)
        check_counts(pair, own, len(a), len(b))
    assert np.array_equal(own[0][1], nn[0][1]) and np.array_equal(own[1][1], nn[1][1])
    check_rows(res, own, len(a), len(b), alphas, False, "own")
    check_rows(sq, own, len(a), len(b), alphas, True, "own")
    print(f"dcd deviation voxelised: {WORST[0]!r}")


# ---- planted, by hand -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["grid", "brute"])
def test_planted_piles(engine):
    """B: three far-apart points.  A: 256 + 128 + 64 distinct points around them.  At alpha = 0 the left terms are 1 - 1/256,
    1 - 1/128 and 1 - 1/64 -- every partial sum is dyadic, so the sum is 255 + 127 + 63 = 445 in whatever order -- and every
    point of B is matched by no other: right is 0."""
    rng = np.random.default_rng(5)
    b = np.array([[0.0, 0.0, 0.0], [100.0, 0.0, 0.0], [0.0, 100.0, 0.0]], dtype=np.float32)
    owner = rng.permutation(np.repeat([0, 1, 2], [256, 128, 64]))
    a = (b[owner] + rng.random((448, 3)).astype(np.float32)).astype(np.float32)
    assert len(np.unique(a, axis=0)) == 448
    alphas = (0.0, 0.5, 1e300)
    with CloudPair(PointCloud(a), PointCloud(b), extent=[100.0, 100.0, 1.0], nn_engine=engine) as pair:
        res = report(pair, alphas)
        sq = report(pair, alphas, squared=True)
        own = own_nn(pair)
        counts = pair.match_counts(True)
        back = pair.match_counts(False)
    assert counts.tolist() == [256, 128, 64] and np.array_equal(own[0][0], owner)
    assert back.sum() == 3 and back.max() == 1
    for r, squared in ((res, False), (sq, True)):
        assert same(r[(ref.SIDE, True, 0.0, squared)], np.float64(445) / 448)
        assert same(r[(ref.SIDE, False, 0.0, squared)], 0.0)
        assert same(r[(ref.BOTH, 0.0, squared)], np.float64(445) / 448 / 2)
        assert same(r[(ref.SIDE, True, 1e300, squared)], 1.0) and same(r[(ref.SIDE, False, 1e300, squared)], 1.0)
        check_rows(r, own, 448, 3, alphas, squared, "own")


def test_a_cloud_against_itself():
    a, _ = uniform(10_000, 1, 77)
    assert len(np.unique(a, axis=0)) == len(a)                     # no duplicates: every point is matched once, by itself
    alphas = (0.0, 3.5, 40.0, 1e300)
    with CloudPair(PointCloud(a), PointCloud(a.copy()), extent=[1.0, 1.0, 1.0]) as pair:
        for squared in (False, True):
            res = report(pair, alphas, squared=squared)
            for key in list(res)[-3 * len(alphas):]:
                assert key[0] in (ref.SIDE, ref.BOTH) and same(res[key], 0.0), key
        assert np.array_equal(pair.match_counts(True), np.ones(len(a), dtype=np.uint32))


def test_planted_lattice_under_pick():
    a, b = lattice_pair()
    n0, n1 = len(a.points), len(b.points)
    with CloudPair(a, b, extent=[24.0, 24.0, 24.0], ties="pick") as pair:
        own_first = own_nn(pair)
        alphas = alphas_of(own_first[0][1])
        res = report(pair, alphas)
        sq = report(pair, alphas, squared=True)
        own = own_nn(pair)
        check_counts(pair, own, n0, n1)
    assert np.array_equal(own[0][0], own_first[0][0]) and np.array_equal(own[1][0], own_first[1][0])
    assert np.max(np.bincount(own[0][0])) > 1                      # points do share their matched point here
    check_rows(res, own, n0, n1, alphas, False, "own")
    check_rows(sq, own, n0, n1, alphas, True, "own")
    print(f"dcd deviation lattice: {WORST[0]!r}")


def test_mean_ties_are_refused():
    a, b = lattice_pair()
    with CloudPair(a, b, extent=[24.0, 24.0, 24.0], ties="mean") as pair:
        with pytest.raises(ValueError, match="mean"):
            report(pair, (40.0,))
        with pytest.raises(ValueError, match="mean"):
            pair.match_counts()


# ---- identities -----------------------------------------------------------------------------------------------------------------
def test_identities():
    """On data with every d2 <= 1 the distance d is >= d2, so exp(-alpha d) <= exp(-alpha d2) and the unsquared term
    1 - exp(-alpha d) / m is >= the squared one, strictly where 0 < d2 < 1: the squared rows lie BELOW the unsquared ones at the
    same alpha.  min and max of the terms lie in [0, 1]; at alpha = 0 the squared and the unsquared request are the same bits."""
    n, m = 5000, 4097
    a, b, nn = uniform_case(n, m)
    assert max(np.max(nn[0][1]), np.max(nn[1][1])) <= 1.0 and np.min(nn[0][1]) < np.max(nn[0][1])
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, a); eng.set_cloud(1, b)
        eng.nn_pair("grid")
        alphas = [0.0, 2.0, 40.0, 1000.0]
        plain = eng.reduce_density_total_many(density_requests(alphas, False))
        squared = eng.reduce_density_total_many(density_requests(alphas, True))
        for (d, alpha, _), p, s in zip(density_requests(alphas, False), plain, squared):
            assert 0.0 <= p[1] <= p[2] <= 1.0 and 0.0 <= s[1] <= s[2] <= 1.0
            if alpha == 0.0:
                assert all(same(x, y) for x, y in zip(p, s))
            else:
                assert s[0] < p[0] and s[1] <= p[1] and s[2] <= p[2], (d, alpha, p, s)
        # the same request twice in a call is answered twice
        twice = eng.reduce_density_total_many([(0, 40.0, False), (0, 40.0, False), (1, 2.0, True)])
        assert twice[0] == twice[1] == plain[2] and twice[2] == squared[5]
    finally:
        eng.close()


# ---- reports: the other rows, reuse, graphs, the command line ---------------------------------------------------------------------
def test_other_rows_unchanged_and_nothing_is_copied(monkeypatch):
    n = 8193
    a, b = uniform(n, n, 41)
    na, nb = vr._unit(n, 1), vr._unit(n, 2)
    nn = oracle_nn(a, b)
    alphas = alphas_of(nn[0][1])
    assert len(alphas) == 4
    kw = dict(hausdorff=True, p2plane=True, plane_to_plane=True, hausdorff_rank=(0.9,), fscore=(0.01, 0.02), chamfer=True,
              truncate=(0.004, 0.05), resolution_psnr=True)
    with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0]) as pair:
        plain = report(pair, (), **kw)
    with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0]) as pair:
        def never(self):
            raise AssertionError(f"{self!r} was copied to the host")
        monkeypatch.setattr(DeviceColumn, "_materialise", never)
        monkeypatch.setattr(DeviceRows, "_materialise", never)
        calls = []
        total_many = pair._engine.reduce_density_total_many
        monkeypatch.setattr(pair._engine, "reduce_density_total_many", lambda reqs, mode="row": calls.append(len(reqs)) or total_many(reqs, mode))
        full = report(pair, alphas, **kw)
        monkeypatch.undo()
        own = own_nn(pair)
    requests = 2 * len(alphas)
    assert sum(calls) == requests and len(calls) == -(-requests // 8), calls       # fetched in ceil(requests / 8) calls
    assert list(full)[:len(plain)] == list(plain) and len(full) == len(plain) + 3 * len(alphas)
    for key, value in plain.items():               # every earlier row is byte-identical to the report without dcd
        assert np.asarray(full[key], dtype=np.float64).tobytes() == np.asarray(value, dtype=np.float64).tobytes(), key
    check_rows(full, nn, n, n, alphas, False, "oracle")
    check_rows(full, own, n, n, alphas, False, "own")


def test_with_reconst_under_graph_replay():
    """Three decoded clouds under one pair with use_graph: per cloud an eager report, the capture and two replays.  Replayed rows
    equal an eager pair's bit for bit, and the alpha = 0 row -- counts alone -- equals the oracle restatement on every replay:
    counts left stale across a replay would show there."""
    n = 30_000
    a, b0 = uniform(n, n, 21)
    origin = PointCloud(a)
    decoded = [(b0 * np.float32(1.0 - 0.01 * k)).astype(np.float32) for k in range(3)]
    alphas = (0.0, 5.0, 40.0, 1e300)
    pair = CloudPair(origin, PointCloud(decoded[0]), extent=[1.0, 1.0, 1.0], use_graph=True)
    try:
        for k in range(3):
            if k:
                pair = pair.with_reconst(PointCloud(decoded[k]))
            rows = []
            for _ in range(4):                     # eager, capture, two replays
                rows.append(report(pair, alphas, hausdorff=True))
                pair.recompute()
            assert pair._graph_id is not None
            with CloudPair(PointCloud(a), PointCloud(decoded[k]), extent=[1.0, 1.0, 1.0]) as eager:
                want = report(eager, alphas, hausdorff=True)
            nn = oracle_nn(a, decoded[k])
            exact = ref.rows(nn[0][1], nn[1][1], nn[0][0], nn[1][0], n, n, (0.0, 1e300))
            for r in rows:
                assert list(r) == list(want) and all(same(r[key], want[key]) for key in want)
                assert all(same(r[key], value) for key, value in exact.items())
            check_rows(rows[-1], nn, n, n, alphas, False, "oracle")
    finally:
        pair.close()


def test_c_calls_and_their_error_codes():
    n, m = 5000, 4000
    a, b = uniform(n, m, 61)
    lib = nat.load()
    eng = nat.Engine(0)

    def call(fn, reqs, out=True):
        k = len(reqs)
        arr = ctypes.c_int * max(k, 1)
        args = [eng._ctx, k, arr(*[r[0] for r in reqs]), arr(*[r[2] for r in reqs]), (ctypes.c_double * max(k, 1))(*[r[1] for r in reqs])]
        buf = (ctypes.c_double * max(3 * k, 1))()
        rc = fn(*args, buf) if out else fn(*args)
        return rc, [tuple(buf[3 * i:3 * i + 3]) for i in range(k)]

    def counts_rc(d, rows):
        buf = (ctypes.c_uint32 * rows)()
        return lib.pccm_match_counts(eng._ctx, d, buf), np.frombuffer(buf, dtype=np.uint32).copy()
    both = ((lib.pccm_reduce_density_prefetch_many, False), (lib.pccm_reduce_density_total_many, True))
    try:
        eng.set_cloud(0, a); eng.set_cloud(1, b)
        for fn, out in both:
            assert call(fn, [(0, 40.0, 0)], out=out)[0] == nat.E_STATE                     # no search result yet
        assert counts_rc(0, m)[0] == nat.E_STATE
        eng.nn_pair("grid")
        nn = oracle_nn(a, b)
        for fn, out in both:
            assert call(fn, [(2, 40.0, 0)], out=out)[0] == nat.E_ARG                       # PCCM_DIR_SELF
            assert call(fn, [(-1, 40.0, 0)], out=out)[0] == nat.E_ARG
            for alpha in (float("nan"), -1.0, -1e-300, float("inf"), -float("inf")):
                assert call(fn, [(0, alpha, 0)], out=out)[0] == nat.E_ARG, alpha
            for squared in (2, -1):
                assert call(fn, [(0, 40.0, squared)], out=out)[0] == nat.E_ARG
            assert call(fn, [(0, 40.0, 0)] * 9, out=out)[0] == nat.E_ARG                   # n <= 8
            assert call(fn, [], out=out)[0] == nat.OK                                      # n == 0
        assert lib.pccm_reduce_density_prefetch_many(eng._ctx, -1, None, None, None) == nat.E_ARG
        assert lib.pccm_reduce_density_prefetch_many(eng._ctx, 1, None, None, None) == nat.E_ARG          # null arrays with n > 0
        assert lib.pccm_reduce_density_total_many(eng._ctx, 1, None, None, None, (ctypes.c_double * 3)()) == nat.E_ARG
        one = (ctypes.c_int * 1)(0)
        assert lib.pccm_reduce_density_total_many(eng._ctx, 1, one, one, (ctypes.c_double * 1)(40.0), None) == nat.E_ARG   # a null out
        assert lib.pccm_match_counts(eng._ctx, 0, None) == nat.E_ARG
        assert counts_rc(2, n)[0] == nat.E_ARG and counts_rc(-1, n)[0] == nat.E_ARG
        # the mapped-reduction calls keep refusing the density map
        k1 = ctypes.c_int * 1
        assert lib.pccm_reduce_map_prefetch_many(eng._ctx, 1, k1(0), k1(nat.METRIC_D1), k1(0), k1(nat.MAP_DENSITY), (ctypes.c_double * 1)(1.0)) == nat.E_ARG
        rc, got = call(lib.pccm_reduce_density_total_many, [(0, 0.0, 0), (1, 1e300, 1)])
        assert rc == nat.OK
        assert all(same(x, y) for x, y in zip(got[0], ref.totals(nn[0][1], nn[0][0], m, 0.0))) \
            and all(same(x, y) for x, y in zip(got[1], ref.totals(nn[1][1], nn[1][0], n, 1e300, True)))
        rc, counts = counts_rc(0, m)
        assert rc == nat.OK and np.array_equal(counts, ref.counts(nn[0][0], m))
        # staleness: a density reduction enqueued on a search whose cloud was replaced is never consumed, nor are its counts
        assert call(lib.pccm_reduce_density_prefetch_many, [(0, 0.0, 0)], out=False)[0] == nat.OK
        b2 = (b * np.float32(0.9)).astype(np.float32)
        eng.set_cloud(1, b2)
        assert call(lib.pccm_reduce_density_total_many, [(0, 0.0, 0)])[0] == nat.E_STATE
        assert counts_rc(0, m)[0] == nat.E_STATE
        eng.nn_pair("grid")
        nn2 = oracle_nn(a, b2)
        rc, got = call(lib.pccm_reduce_density_total_many, [(0, 0.0, 0), (1, 0.0, 0)])
        assert rc == nat.OK and all(same(p, q) for p, q in zip(got[0], ref.totals(nn2[0][1], nn2[0][0], m, 0.0)))
        assert all(same(p, q) for p, q in zip(got[1], ref.totals(nn2[1][1], nn2[1][0], n, 0.0)))
        assert not same(got[0][0], ref.totals(nn[0][1], nn[0][0], m, 0.0)[0])
        rc, counts = counts_rc(1, n)
        assert rc == nat.OK and np.array_equal(counts, ref.counts(nn2[1][0], n))
        # a search under PCCM_TIES_MEAN: a virtual neighbour has no row
        eng.set_ties("mean")
        eng.nn_pair("grid")
        for fn, out in both:
            assert call(fn, [(0, 40.0, 0)], out=out)[0] == nat.E_STATE
        assert counts_rc(0, m)[0] == nat.E_STATE
        eng.set_ties("pick")
        eng.nn_pair("grid")
        assert call(lib.pccm_reduce_density_total_many, [(0, 40.0, 0)])[0] == nat.OK
        eng.set_shard(0, 2)
        for fn, out in both:
            assert call(fn, [(0, 40.0, 0)], out=out)[0] == nat.E_STATE                     # a sharded context
        assert counts_rc(0, m)[0] == nat.E_STATE
    finally:
        eng.close()


def test_command_line(tmp_path):
    n = 5000
    a, b = uniform(n, n, 51)
    b = (a + np.float32(0.02) * (b - np.float32(0.5))).astype(np.float32)
    c = (a + np.float32(0.05) * (b - np.float32(0.5))).astype(np.float32)
    pa, pb, pc = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "c.ply")
    write_point_cloud(pa, PointCloud(a))
    write_point_cloud(pb, PointCloud(b))
    write_point_cloud(pc, PointCloud(c))
    args = ["--ocloud", pa, "--pcloud", pb, "--pcloud", pc, "--hausdorff"]
    alphas = (5.0, 40.0)
    added = 3 * len(alphas)

    def expect(decoded, squared):
        nn = oracle_nn(a, decoded)
        want = ref.rows(nn[0][1], nn[1][1], nn[0][0], nn[1][0], n, n, alphas, squared)
        out = []
        for k, v in want.items():
            tag = f"[{k[-2]!r}, squared]" if squared else f"[{k[-2]!r}]"
            out.append(([k[0] + tag] + ([str(k[1])] if k[0] == ref.SIDE else []), float(v)))
        return out

    def check(fields, want):
        assert len(fields) == len(want)
        for got, (head, value) in zip(fields, want):
            assert got[:-1] == head, (got, head)
            close(float(got[-1]), value, 40.0, got)
    base = CliRunner().invoke(cli, args)
    assert base.exit_code == 0, (base.output, base.exception)
    base_lines = base.output.rstrip("\n").split("\n")
    per = len(base_lines) // 2
    for squared in (False, True):
        flags = ["--dcd", "40", "--dcd", "5"] + (["--dcd-squared"] if squared else [])
        text = CliRunner().invoke(cli, args + flags)
        csv = CliRunner().invoke(cli, args + flags + ["--csv"])
        assert text.exit_code == 0 and csv.exit_code == 0, (text.output, text.exception, csv.exception)
        lines = text.output.rstrip("\n").split("\n")
        assert len(base_lines) == 2 * per and len(lines) == 2 * (per + added)
        for k, decoded in enumerate((b, c)):       # one report per processed cloud: today's rows, then the new ones
            mine, theirs = lines[k * (per + added):(k + 1) * (per + added)], base_lines[k * per:(k + 1) * per]
            assert [ln.split() for ln in mine[1:per]] == [ln.split() for ln in theirs[1:]]
            # (a label with ", squared" in it prints as two words)
            fields = [ln.split()[1:] for ln in mine[per:]]
            fields = [[" ".join(f[:2])] + f[2:] if squared else f for f in fields]
            check(fields, expect(decoded, squared))
        rows = [ln for ln in csv.output.split("\n") if ln]             # (to_csv ends its text with a newline of its own)
        assert len(rows) == 2 * (per + added)
        import csv as csv_module
        parsed = [r for r in csv_module.reader(rows[-added:])]
        check([[r[1]] + [f for f in r[2:] if f] for r in parsed], expect(c, squared))
