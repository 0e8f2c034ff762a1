"""Filed tails (open_pcc_metric_amd/csrc/pccm_tail_wave.h): a captured step whose brick search files the queries ring 1 did not settle
by blocks of 4096 rows and leaves the tail launch out, the reduction workgroup of each block settling its own entries before it
reduces.  Every case of tests/tail_filed_cases.py runs eager step -> capture -> two replays on a fresh context; every step's rows and
squared distances of both directions are compared bit for bit with the kd-tree oracle, and the totals, the columns and nn_stats with
the same steps of a child process under PCCM_TAIL_FILED=0 (the classic graph).  The filing search overwrites every filed row with a
record no search produces (NaN coordinates, row -1), so the records an earlier step left at those rows cannot stand in for a settle
that is missing or whose store does not reach the reduction: it would show as NaN totals and rows of -1 here.  Which graph was
captured is read from graph_tail_filed(), never from a time.  What decides it -- a flagged query, a block over the capacity -- is planted; the capture rule
itself is proved on the host (tests/test_tailfile_host.py), and no kernel is ever run in a state known to overflow."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_planted as gp
import tail_filed_cases as tc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def nat():
    from open_pcc_metric_amd import _native
    return _native


@pytest.fixture(scope="module")
def classic(tmp_path_factory):
    """Every case on the classic graph, run once in a child process (the switch is latched per process)."""
    out = str(tmp_path_factory.mktemp("tail_filed") / "classic.npz")
    env = dict(os.environ, PCCM_TAIL_FILED="0", PCCM_NO_TORCH="1")
    run = subprocess.run([sys.executable, os.path.join(HERE, "tail_filed_child.py"), out], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "tail filed child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return np.load(out)


def test_the_cases_are_what_they_claim():
    """On the host, from the model of the stop rule: tails exist, nothing is flagged in the positive cases, the outlier is."""
    for name in tc.CASES:
        case = tc.build(name)
        for d in (0, 1):
            p = gp.predict(case, d)
            assert p.lo >= 20, (name, d, p.lo)                               # ~1e-3 of the rows fail ring 1
            want_flagged = 1 if (name == "outlier" and d == 0) else 0
            assert p.flagged == want_flagged, (name, d, p.flagged)
    assert len(tc.build("edges").a) % tc.BLOCK != 0


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_filed_steps_are_exact_and_equal_the_classic_graph(nat, classic, name):
    case = tc.build(name)
    got = tc.run(case, nat)
    print(name, "filed", got.filed, "geometry as predicted", gp.same_geom(got.geom, case.geom),
          "tail", [s["tail_queries"] for s in got.steps[0].stats], "flagged", [s["fallback_queries"] for s in got.steps[0].stats])
    assert got.filed == tc.FILED[name], f"{name}: the captured graph {'left out' if got.filed else 'kept'} the tail launch"
    assert len(got.steps) == 4
    for k, s in enumerate(got.steps):
        for d in (0, 1):
            rows, d2 = gp.truth(case, d)
            bad = np.flatnonzero((s.idx[d] != rows) | (s.d2[d] != d2))
            assert len(bad) == 0, f"{name} step {k} direction {d}: {len(bad)} rows differ from the oracle, first {bad[:4].tolist()}"
            assert np.array_equal(s.idx[d], classic[f"{name}/{k}/idx{d}"]) and s.d2[d].tobytes() == classic[f"{name}/{k}/d2{d}"].tobytes()
            assert [s.stats[d]["fallback_queries"], s.stats[d]["tail_queries"]] == classic[f"{name}/{k}/stats{d}"].tolist(), (name, k, d)
            assert s.stats[d]["tail_queries"] > 0
        assert s.totals.tobytes() == classic[f"{name}/{k}/totals"].tobytes(), f"{name} step {k}: totals differ from the classic graph"
        assert s.totals.tobytes() == got.steps[0].totals.tobytes(), f"{name} step {k}: totals differ from the eager step"
    if name == "outlier":
        assert got.steps[0].stats[0]["fallback_queries"] == 1


def _report(pair):
    from open_pcc_metric_amd.calculator import MetricCalculator
    from open_pcc_metric_amd.options import CalculateOptions, transform_options
    return MetricCalculator(pair).calculate(transform_options(CalculateOptions(None, True, True))).as_dict()


@pytest.mark.parametrize("name", ["plain", "edges"])
def test_reports_through_a_filed_graph_equal_the_oracle(nat, name):
    """The package's own path: CloudPair.recompute() captures behind an eager step; every report row of every step is the oracle's,
    also with a getter between the replayed search and the report."""
    from open_pcc_metric_amd.cloud_pair import CloudPair
    from open_pcc_metric_amd.point_cloud import PointCloud
    from oracle import oracle as orc
    case = tc.build(name)
    want = orc.OraclePair(case.a, case.b, case.na, case.nb, method="kdtree").report(hausdorff=True, point_to_plane_=True, peak=1.0)
    pair = CloudPair(PointCloud(case.a, case.na), PointCloud(case.b, case.nb), extent=[1.0, 1.0, 1.0], device=0, use_graph=True)
    try:
        for k in range(4):                                   # eager, capture, replay, replay
            pair.recompute()
            if k == 3:
                dist = np.asarray(pair.get_left_neighbour_distances(), dtype=np.float64)      # (the squared distances)
                assert dist.tobytes() == gp.truth(case, 0)[1].tobytes()
            got = _report(pair)
            for key, val in want.items():
                assert got[key] == val, f"{name} step {k}: {key}: {got[key]!r} != oracle {val!r}"
        assert pair._graph_id is not None and pair._engine.graph_tail_filed(pair._graph_id)
    finally:
        pair.close()


def test_a_reader_that_is_no_reduction_gets_the_classic_tail(nat):
    """A capture that files its tails and then reduces nothing: pccm_graph_end finds the lists unconsumed and ends the graph with
    the classic tail launch; so does a capture whose first reader is a single-column reduction."""
    case = tc.build("plain")
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, case.a)
        eng.set_cloud(1, case.b)
        eng.set_normals(0, case.na)
        eng.set_normals(1, case.nb)
        req = tc.requests(case, nat)
        eng.drop_caches()
        eng.nn_pair("grid")
        eng.reduce_prefetch_many(req)
        eager = np.asarray(eng.reduce_total_many(req)).tobytes()
        for follow in ((), [(0, nat.METRIC_D1)]):
            eng.graph_begin()
            eng.drop_caches()
            eng.nn_pair("grid")
            if follow:
                eng.reduce_prefetch_many(follow)
            gid = eng.graph_end()
            assert not eng.graph_tail_filed(gid)
            eng.graph_launch(gid)
            for d in (0, 1):
                idx, d2 = eng.fetch_nn(d)
                rows, want = gp.truth(case, d)
                assert np.array_equal(idx, rows) and d2.tobytes() == want.tobytes()
            eng.reduce_prefetch_many(req)
            assert np.asarray(eng.reduce_total_many(req)).tobytes() == eager
            eng.graph_destroy(gid)
    finally:
        eng.close()


def test_filing_switched_off_or_without_the_eager_facts_keeps_the_tail_launch(nat):
    """pccm_set_tail_filing(0) inside a capture keeps the tail launch in that capture; so does a capture that searches a direction
    the eager step in front of it did not (no flagged count, no block counts to decide from).  Both stay exact."""
    case = tc.build("plain")
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, case.a)
        eng.set_cloud(1, case.b)
        eng.set_normals(0, case.na)
        eng.set_normals(1, case.nb)
        req = tc.requests(case, nat)
        left = [r for r in req if r[0] == nat.DIR_LEFT]

        def sweep():
            eng.drop_caches()
            eng.nn_pair("grid")
            eng.reduce_prefetch_many(req)

        def exact():
            for d in (0, 1):
                idx, d2 = eng.fetch_nn(d)
                rows, want = gp.truth(case, d)
                assert np.array_equal(idx, rows) and d2.tobytes() == want.tobytes()

        # (a capture allocates nothing: the whole sequence once, so that every buffer and slot exists)
        sweep()
        eager = np.asarray(eng.reduce_total_many(req)).tobytes()
        # the same points again: both directions' results are void.  Only the left one is searched and reduced eagerly, then
        # the pair is captured
        eng.set_cloud(1, case.b)
        eng.set_normals(1, case.nb)
        eng.drop_caches()
        eng.nn(nat.DIR_LEFT, "grid")
        eng.reduce_prefetch_many(left)
        eng.reduce_total_many(left)
        eng.graph_begin()
        sweep()
        gid = eng.graph_end()
        assert not eng.graph_tail_filed(gid)
        assert np.asarray(eng.reduce_total_many(req)).tobytes() == eager
        exact()
        eng.graph_destroy(gid)
        # the whole pair eagerly, then a capture with filing switched off, then one with it left on
        sweep()
        assert np.asarray(eng.reduce_total_many(req)).tobytes() == eager
        for on in (False, True):
            eng.graph_begin()
            if not on:
                eng.set_tail_filing(False)
            sweep()
            gid = eng.graph_end()
            assert eng.graph_tail_filed(gid) == on
            eng.graph_launch(gid)
            assert np.asarray(eng.reduce_total_many(req)).tobytes() == eager
            exact()
            eng.graph_destroy(gid)
        with pytest.raises(nat.PccmStateError):
            eng.set_tail_filing(True)                       # speaks of a capture in progress only
    finally:
        eng.close()


def test_a_stale_filed_graph_is_refused_and_captured_anew(nat):
    case, other = tc.build("plain"), tc.build("edges")
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, case.a)
        eng.set_cloud(1, case.b)
        eng.set_normals(0, case.na)
        eng.set_normals(1, case.nb)
        req = tc.requests(case, nat)

        def sweep():
            eng.drop_caches()
            eng.nn_pair("grid")
            eng.reduce_prefetch_many(req)

        sweep()
        eng.reduce_total_many(req)
        eng.graph_begin()
        sweep()
        gid = eng.graph_end()
        assert eng.graph_tail_filed(gid)
        eng.set_cloud(1, other.b)                            # other points under the captured graph
        eng.set_normals(1, case.nb)
        with pytest.raises(nat.PccmStateError):
            eng.graph_launch(gid)
        mixed = gp.SimpleNamespace(a=case.a, b=other.b, truth={})
        sweep()                                              # a fresh eager step on the new pair, then a new capture
        eng.reduce_total_many(req)
        eng.graph_begin()
        sweep()
        gid2 = eng.graph_end()
        assert eng.graph_tail_filed(gid2)
        eng.graph_launch(gid2)
        for d in (0, 1):
            idx, d2 = eng.fetch_nn(d)
            rows, want = gp.truth(mixed, d)
            assert np.array_equal(idx, rows) and d2.tobytes() == want.tobytes()
    finally:
        eng.close()
