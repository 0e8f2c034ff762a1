"""The per-point columns the getters fetch (pccm_point_metric, pccm_error_vectors): one-job launches of k_point_jobs, with a
non-zero q_begin when the context owns a shard that does not start at row 0.

Small clouds on purpose (1000 against 1100 points): a row-offset mistake shows at the first shard boundary.  Every column is held
to the host restatement the suite of its family uses, at that suite's tolerance -- error vectors, projections and their squares
bit for bit (tests/oracle_engine.py, tests/ties_reference.py), the PointSSIM similarity bit for bit (tests/pointssim_reference.py),
the angular similarity within 2^-50 (tests/angular_reference.py: only acos may differ, in its last bit) -- then the two shards of
a two-rank split must concatenate to the unsharded column, and the reductions of the same requests must be NumPy's of the
fetched column, bit for bit."""
import numpy as np
import pytest

import pointssim_reference as ssim_ref
from angular_reference import angular_rows, angular_tie_mean
from open_pcc_metric_amd import _native as nat
from ties_reference import MeanOracleEngine, tie_sets
from variant_rows import make_pair

pytestmark = pytest.mark.gpu

N_A, N_B = 1000, 1100
SSIM_K = 12
ANGULAR_TOL = 2.0 ** -50            # tests/test_gpu_angular.py
DIRS = (nat.DIR_LEFT, nat.DIR_RIGHT)
MODES = ("row", "neighbour")
SSIM_GEOMETRY = nat.METRIC_SSIM["geometry"]


def clouds():
    """fp32 clouds with exact ties (four points of B at one distance from each tie base of A, duplicate rows of B, copies of
    them in A) and normals that include non-unit and zero-length rows."""
    a, b, rows = make_pair(N_A, N_B, seed=5, surface=True, ties=True)
    assert a.dtype == np.float32 and b.dtype == np.float32 and "tie_a" in rows
    rng = np.random.default_rng(77)
    normals = []
    for n in (N_A, N_B):
        v = rng.standard_normal((n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        v *= np.where(rng.random((n, 1)) < 0.25, 10.0 ** rng.uniform(-3, 3, (n, 1)), 1.0)      # non-unit
        v[rng.random(n) < 0.05] = 0.0                                 # zero-length
        normals.append(v)
    return a, b, normals[0], normals[1]


def requests(ties):
    """(name, metric, normal_mode) of every column with a reduction; the error vectors come on top."""
    out = [(f"{name}/{mode}", metric, mode) for name, metric in (("proj", nat.METRIC_PROJ), ("d2", nat.METRIC_D2)) for mode in MODES]
    out += [(f"angular/{mode}", nat.METRIC_ANGULAR, mode) for mode in MODES]           # (normal_mode does not apply)
    if ties == "pick":                                                                 # undefined under "mean"
        out += [(f"ssim_geometry/{mode}", SSIM_GEOMETRY, mode) for mode in MODES]
    return out


def load(eng, ties, data):
    a, b, na, nb = data
    eng.set_cloud(0, a)
    eng.set_cloud(1, b)
    eng.set_normals(0, na)
    eng.set_normals(1, nb)
    eng.set_ties(ties)


def fetch(eng, ties, with_totals):
    """Every column of this context's rows: {(name, d): array, or IndexError for row-indexed normals that do not reach}, and
    (unsharded only) the reductions of the same requests."""
    eng.nn_pair("auto")
    if ties == "pick":
        for which in (0, 1):
            eng.ssim_features(which, SSIM_K, ["geometry"])
    cols, totals = {}, {}
    for d in DIRS:
        cols["err", d] = eng.error_vectors(d)
        for name, metric, mode in requests(ties):
            try:
                cols[name, d] = eng.point_metric(d, metric, mode)
                if with_totals:
                    totals[name, d] = eng.reduce_total(d, metric, mode)
            except IndexError:
                cols[name, d] = IndexError
                if with_totals:
                    with pytest.raises(IndexError):
                        eng.reduce_total(d, metric, mode)
    return cols, totals


@pytest.fixture(scope="module")
def data():
    return clouds()


@pytest.fixture(scope="module", params=["pick", "mean"])
def run(request, data):
    """One context per tie policy: the unsharded columns and reductions, the matched rows, then the columns of both ranks of a
    two-way split of both directions."""
    ties = request.param
    eng = nat.Engine(0)
    try:
        load(eng, ties, data)
        whole, totals = fetch(eng, ties, True)
        idx = {d: eng.fetch_nn(d)[0] for d in DIRS}
        shards, ranges = [], []
        for rank in (0, 1):
            for d in DIRS:
                eng.set_shard_dir(d, rank, 2)
            ranges.append({d: eng.shard_range(d) for d in DIRS})
            shards.append(fetch(eng, ties, False)[0])
    finally:
        eng.close()
    return dict(ties=ties, whole=whole, totals=totals, idx=idx, shards=shards, ranges=ranges)


@pytest.fixture(scope="module")
def restated(data):
    """The host restatements, per tie policy: the CPU test double for error vectors, projections and squares; the matched rows
    it searched; the tie sets."""
    a, b, na, nb = data
    out = {}
    for ties in ("pick", "mean"):
        ref = MeanOracleEngine()
        load(ref, ties, data)
        for d in DIRS:
            ref.nn(d)
        out[ties] = ref
    out["sets"] = {nat.DIR_LEFT: tie_sets(a, b)[1], nat.DIR_RIGHT: tie_sets(b, a)[1]}
    out["features"] = (ssim_ref.features(a, SSIM_K, "geometry"), ssim_ref.features(b, SSIM_K, "geometry"))
    return out


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def test_the_data_has_what_it_is_here_for(data, restated):
    a, b, na, nb = data
    for nrm in (na, nb):
        length = np.linalg.norm(nrm, axis=1)
        assert np.sum(length == 0.0) > 10 and np.sum(np.abs(length - 1.0) > 0.1) > 100
    for d in DIRS:
        assert sum(len(s) > 1 for s in restated["sets"][d]) >= 5


def test_unsharded_columns_match_the_restatements(run, restated, data):
    a, b, na, nb = data
    ties, whole, ref = run["ties"], run["whole"], restated[run["ties"]]
    for d in DIRS:
        own, other = (na, nb) if d == nat.DIR_LEFT else (nb, na)
        assert np.array_equal(run["idx"][d], ref.fetch_nn(d)[0])
        assert same_bits(whole["err", d], ref.error_vectors(d)), ("err", d)
        for name, metric, mode in requests(ties):
            got = whole[name, d]
            if metric in (nat.METRIC_PROJ, nat.METRIC_D2):
                if mode == "row" and d == nat.DIR_RIGHT:        # 1100 rows index 1000 normals: the reference's IndexError (quirk Q1)
                    with pytest.raises(IndexError):
                        ref.point_metric(d, metric, mode)
                    assert got is IndexError
                    continue
                assert same_bits(got, ref.point_metric(d, metric, mode)), (name, d)
            elif metric == nat.METRIC_ANGULAR:
                want = angular_tie_mean(own, other, restated["sets"][d]) if ties == "mean" else angular_rows(own, other, run["idx"][d])
                assert got.shape == want.shape and not np.any(np.abs(got - want) > ANGULAR_TOL), (name, d)
            else:
                f_own, f_other = restated["features"][::1 if d == nat.DIR_LEFT else -1]
                assert same_bits(got, ssim_ref.similarity_rows(f_own, f_other, run["idx"][d])), (name, d)
    if ties == "mean":                                          # the tie rows move the columns: "mean" is not the pick here
        assert not same_bits(whole["err", nat.DIR_LEFT], restated["pick"].error_vectors(nat.DIR_LEFT))


def test_shards_concatenate_to_the_unsharded_columns(run):
    # 128-row leaves at this size: rows 0-512 and 512-1000 of A -- the second shard starts at q_begin 512 and has 488 rows,
    # no multiple of the 256 rows of a workgroup
    assert [r[nat.DIR_LEFT] for r in run["ranges"]] == [(0, 512), (512, N_A)]
    assert [r[nat.DIR_RIGHT] for r in run["ranges"]] == [(0, 512), (512, N_B)]
    for key, want in run["whole"].items():
        parts = [s[key] for s in run["shards"]]
        if want is IndexError:                                  # the whole iterating cloud decides: every rank raises
            assert parts == [IndexError, IndexError], key
            continue
        for part, r in zip(parts, run["ranges"]):
            assert len(part) == r[key[1]][1] - r[key[1]][0], key
        assert same_bits(np.concatenate(parts), want), key


def test_reductions_are_numpys_of_the_fetched_columns(run):
    assert len(run["totals"]) == sum(v is not IndexError for k, v in run["whole"].items() if k[0] != "err")
    for key, (s, mn, mx) in run["totals"].items():
        col = run["whole"][key]
        assert s.tobytes() == np.sum(col).tobytes(), key
        assert mn.tobytes() == np.min(col).tobytes() and mx.tobytes() == np.max(col).tobytes(), key
