"""The uniform-grid engine (k_grid_query<REC, SELF>, k_grid_query_coop<SELF>, k_brick_query's ring-1 rule, k_grid_tail<REC, SELF>:
open_pcc_metric_amd/csrc/pccm_grid.hip, pccm_grid.h, pccm_brick.hip) on the planted families of tests/grid_planted.py: rows and d2
against the kd-tree oracle bit for bit in directions 0, 1 and 2, nn_stats()["fallback_queries"] against the count the host model
of the stop rule flags (zeros included), nn_stats()["tail_queries"] inside [lo, lo + band] on the paths with a tail, and
last_path() naming the kernels the case is meant for.

  F  the true neighbour h 2^-10 behind each of the 6 faces of the ring-1, -2 and -3 cubes with a decoy inside (a rule that is wrong
     on one side of one axis returns the decoy's row), and the neighbour just under L_r inside (a rule that settles late returns the
     oracle's rows -- only the counts show it);
  B  corner, edge and face cells, planar and collinear pairs, grids every cube covers;
  T  exact ties across rings and across the lanes of wave_tail, duplicates in the self search;
  R  flagged queries whose decoy and true neighbour swap order in the rescan's fp32 filter, in every mix of fp32-exact and fp64
     clouds; every scenario query is flagged with nothing found in the self search;
  X  a trimmed box: stray points on every side clamp into boundary cells (test_trimmed_box_...);
  long tail  more than 2^18 tail entries per direction: the thread-per-query half of k_grid_tail.

Every case is built on the geometry the library reports for it (pccm_grid_geometry): the frame decides the geometry, the probes are
placed in its cell units, and the geometry is read again after the last search.  tests/test_grid_planted_host.py proves the cases."""
import json

import numpy as np
import pytest

import brute_planted as bp
import grid_planted as gp

pytestmark = pytest.mark.gpu

FRAME_CASES = {
    "flat-11": ("flat", (True, True), "thread", "Rec32"),
    "flat-00": ("flat", (False, False), "thread", "GridRec"),
    "flat-10": ("flat", (True, False), "thread", "GridRec"),
    "flat-01": ("flat", (False, True), "thread", "GridRec"),
    "long-00": ("long", (False, False), "coop", "GridRec"),
    "long-11": ("long", (True, True), "brick", "Rec32"),
}


@pytest.fixture()
def eng():
    from open_pcc_metric_amd import _native as nat
    e = nat.Engine(0)
    e.nn_want_idx(True)
    yield e
    e.close()


def _geometry(eng):
    return gp.make_geom(*eng.grid_geometry())


def _check_path(eng, d, kind, rec):
    """The search of direction d went through the kernels the case is meant for, and through no other query kernel."""
    self_ = "true" if d == 2 else "false"
    path = eng.last_path(d)
    query = [k for k in path if k.startswith(("k_grid_query", "k_brick_query", "k_grid_tail", "k_vox_query", "k_lattice_query", "k1_scan", "k2b_fallback"))]
    if kind == "thread":
        assert query == [f"k_grid_query<pccm::{rec}, {self_}>", f"k2b_fallback<{self_}>"], (d, path)
    elif kind == "coop":
        assert query == [f"k_grid_query_coop<{self_}>", f"k_grid_tail<pccm::GridRec, {self_}>"], (d, path)
    else:
        assert len(query) == 2 and query[0].startswith(f"k_brick_query<{self_}, ") and query[1] == f"k_grid_tail<pccm::Rec32, {self_}>", (d, path)
    return query


def _check_rows(eng, case, d):
    b, e = eng.shard_range(d)
    rows, d2 = gp.truth(case, d)
    idx, got = eng.fetch_nn(d)
    bad = np.flatnonzero((idx != rows[b:e]) | (got != d2[b:e]))
    assert len(bad) == 0, (f"{case.name} direction {d} [{b}, {e}): {len(bad)} of {e - b} differ, first at query {b + bad[0]}: row {idx[bad[0]]} "
                           f"d2 {got[bad[0]]!r}, oracle row {rows[b + bad[0]]} d2 {d2[b + bad[0]]!r}")
    return b, e


def _place(eng, builder):
    """Build the case on the predicted geometry, search, read the geometry back and rebuild on it until the two agree."""
    g = None
    for _ in range(4):
        case = builder(g)
        eng.set_cloud(0, case.a)
        eng.set_cloud(1, case.b)
        eng.nn_pair("grid")
        g = _geometry(eng)
        if gp.same_geom(g, case.geom):
            return case
    pytest.fail(f"{case.name}: after 4 rounds the grid the library builds {g.dim.tolist()} {g.h.tolist()} is still not the one the probes were "
                f"placed on {case.geom.dim.tolist()} {case.geom.h.tolist()}")


def _counts(eng, case, d, kind, line, with_band=True):
    """Model against nn_stats() for the rows of this context's shard -> (flagged, lo, band) predicted and the stats measured.  On
    the brick path the queries of bricks that overflow their LDS budget count into lo: they go to the tail whatever the rule says."""
    b, e = eng.shard_range(d)
    p = gp.predict(case, d, kind if kind != "thread" and with_band else None)
    assert len(p.undecided) == 0, f"{case.name} direction {d}: queries {p.undecided[:8].tolist()} are undecided on the geometry read back"
    ring = p.ring[b:e]
    stats = eng.nn_stats(d)
    open1, over = ring != 1, 0
    if kind == "brick":
        q, s, _ = gp.pair_of(case, d)
        mask = gp.brick_overflow(case.geom, q[b:e], s, max(len(case.a), len(case.b)))
        over = int(np.sum(mask & ~open1))
        open1 = open1 | mask
    want_flagged, lo = int(np.sum(ring == gp.FLAGGED)), int(np.sum(open1))
    band = int(np.sum(p.band_mask[b:e] & ~open1)) if with_band else None
    line[str(d)] = {"rows": [b, e], "flagged": [want_flagged, stats["fallback_queries"]], "tail": [lo, band, stats["tail_queries"]],
                    "overflow": over, "settle_at": [int(np.sum(ring == r)) for r in (1, 2, 3)]}
    if d != 1 and case.sites:
        by = {}
        for s in case.sites:
            if b <= s.qrow < e:
                by.setdefault(s.spec[0], [0, 0, 0, 0])[p.by_site[s.name] - 1] += 1
        line[str(d)]["scenarios_by_ring"] = by
    return want_flagged, lo, band, stats


def _assert_counts(case, d, kind, want_flagged, lo, band, stats):
    assert stats["fallback_queries"] == want_flagged, (f"{case.name} direction {d}: {stats['fallback_queries']} queries went to the exact rescan, the "
                                                       f"model of the stop rule flags {want_flagged}")
    if kind != "thread":
        assert band <= lo / 20, (lo, band)
        assert lo <= stats["tail_queries"] <= lo + band, (f"{case.name} direction {d}: {stats['tail_queries']} tail queries, the model leaves {lo} "
                                                         f"open after ring 1 and cannot decide {band}")


@pytest.mark.parametrize("name", sorted(FRAME_CASES))
def test_planted_frame_is_exact_and_counts_what_the_model_counts(eng, name):
    frame, fmt, kind, rec = FRAME_CASES[name]
    case = _place(eng, lambda g: gp.cached("frame", frame, fmt) if g is None else gp.build(frame, fmt, g))
    eng.nn(2, "grid")
    line = {}
    for d in (0, 1, 2):
        _check_rows(eng, case, d)
        line.setdefault("path", {})[str(d)] = _check_path(eng, d, kind, rec)
        got = _counts(eng, case, d, kind, line)
        print(json.dumps({name: {str(d): line[str(d)]}}))
        _assert_counts(case, d, kind, *got)
    assert gp.same_geom(_geometry(eng), case.geom), "the last search ran on another grid than the one the probes were placed on"
    sound = [s for s in case.sites if s.spec[0] in ("F", "R") and hasattr(s, "decoy")]
    idx, _ = eng.fetch_nn(0)
    assert len(sound) == 18 + 4 and all(idx[s.qrow] == s.brows[s.want] for s in sound)


@pytest.mark.parametrize("fmt,rec", [((True, True), "Rec32"), ((False, False), "GridRec")], ids=["11", "00"])
def test_trimmed_box_is_exact_and_counts_what_the_model_counts(eng, fmt, rec):
    """X: stray points far outside on every side, so that the grid covers the quantile box and they clamp into boundary cells --
    outliers whose neighbour shares their boundary cell, outliers whose neighbour is inside the box, queries inside whose neighbour
    is a clamped outlier, outliers beyond two axes."""
    case = _place(eng, lambda g: gp.cached("trim", fmt) if g is None else gp.build_trim(fmt, g))
    both = np.vstack([case.a, case.b])
    assert np.all(case.geom.dim * case.geom.h < 0.1 * (both.max(axis=0) - both.min(axis=0))), "the grid is not smaller than the bounding box"
    eng.nn(2, "grid")
    line = {}
    for d in (0, 1, 2):
        _check_rows(eng, case, d)
        _check_path(eng, d, "thread", rec)
        got = _counts(eng, case, d, "thread", line)
        print(json.dumps({case.name: {str(d): line[str(d)]}}))
        _assert_counts(case, d, "thread", *got)
    assert gp.same_geom(_geometry(eng), case.geom), "the last search ran on another grid than the one the probes were placed on"


@pytest.mark.parametrize("name", ["long-00", "long-11", "flat-11"])
def test_shards_reassemble_and_their_counts_add_up(eng, name):
    """Three ranks' rows of direction 0: the pieces are the unsharded answer, the flagged counts sum to the model's and every rank's
    tail count lies inside its own bounds.  A shard of the fp32-exact frame takes the brick kernel's 4 x 4 bricks, whose LDS budget
    follows the MEAN density; the frame's dense zone holds 1.8 times that, so nearly all of those bricks overflow and hand their
    queries to the tail, as clumped data does by design: the port of the budget predicts that count too."""
    frame, fmt, kind, rec = FRAME_CASES[name]
    case = _place(eng, lambda g: gp.cached("frame", frame, fmt) if g is None else gp.build(frame, fmt, g))
    covered, flagged = 0, 0
    line = {}
    try:
        for rank in range(3):
            eng.set_shard_dir(0, rank, 3)
            eng.nn(0, "grid")
            b, e = _check_rows(eng, case, 0)
            assert (b, e) == bp.shard_of(len(case.a), rank, 3) and b == covered
            covered = e
            _check_path(eng, 0, kind, rec)
            want_flagged, lo, band, stats = _counts(eng, case, 0, kind, line)
            print(json.dumps({f"{name}/rank{rank}": line["0"]}))
            assert stats["fallback_queries"] == want_flagged
            if kind != "thread":
                assert lo <= stats["tail_queries"] <= lo + band, (rank, lo, band, stats["tail_queries"])
            flagged += stats["fallback_queries"]
            assert gp.same_geom(_geometry(eng), case.geom)
    finally:
        eng.set_shard_dir(0, 0, 1)
    assert covered == len(case.a) and flagged == gp.predict(case, 0).flagged


@pytest.mark.parametrize("name", sorted(gp.SMALL))
def test_flat_and_tiny_grids_settle_what_the_model_settles(eng, name):
    """dim = 1 on one or two axes, two cells on an axis, grids a ring-3 cube covers, on the kernel the case names (fp64 inputs:
    GridRec): rows, the flagged count and -- for the line along x, ONE x-row, which takes the cooperative kernel -- the tail count
    inside [lo, lo + band], all on the geometry the library reports."""
    kind = gp.SMALL[name][3]
    case = gp.small_case(name)
    eng.set_cloud(0, case.a)
    eng.set_cloud(1, case.b)
    eng.nn_pair("grid")
    eng.nn(2, "grid")
    case.geom = _geometry(eng)
    line = {"dim": case.geom.dim.tolist()}
    for d in (0, 1, 2):
        _check_rows(eng, case, d)
        _check_path(eng, d, kind, "GridRec")
        got = _counts(eng, case, d, kind, line)
        _assert_counts(case, d, kind, *got)
    print(json.dumps({name: line}))


def test_long_tail_takes_the_thread_per_query_half_of_k_grid_tail(eng):
    """More than 2^18 entries on both directions' tail lists (kTailWaveMax): k_grid_tail runs thread_search(from_tail = 1) for both
    jobs, counts what it retires for the rescan half that waits on it, and a handful of queries still go to the rescan.  The tail
    also holds the queries of bricks that overflow their LDS budget (a slab holds twice the mean density: 14 789 and 827 queries
    that ring 1 would settle, brick_overflow()), so the lower bound counts them; no upper bound is asserted here."""
    case = _place(eng, lambda g: gp.cached("long_tail") if g is None else gp.long_tail_case(g))
    line = {}
    for d in (0, 1):
        _check_rows(eng, case, d)
        line.setdefault("path", {})[str(d)] = _check_path(eng, d, "brick", "Rec32")
        want_flagged, lo, band, stats = _counts(eng, case, d, "brick", line, with_band=False)
        print(json.dumps({"long_tail": {str(d): line[str(d)]}}))
        assert lo > gp.TAIL_WAVE_MAX
        assert stats["tail_queries"] > gp.TAIL_WAVE_MAX, f"direction {d}: {stats['tail_queries']} tail queries do not reach the thread-per-query branch"
        assert stats["tail_queries"] >= lo
        assert stats["fallback_queries"] == want_flagged >= gp.LONG_TAIL_ISOLATED
    assert gp.same_geom(_geometry(eng), case.geom)
