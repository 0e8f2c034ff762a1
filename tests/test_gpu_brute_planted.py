"""The brute-force engine (k1_scan<8, SELF> -> k2_refine<SELF> -> k2b_fallback<SELF>, open_pcc_metric_amd/csrc/pccm_brute.hip, and
rescan_body, pccm_rescan.h) on the planted families of tests/brute_planted.py: rows and d2 against the kd-tree oracle bit for bit,
and nn_stats()["fallback_queries"] against the count the host model of the scan and the certificate predicts, 0 included.

  R  fp32 order reversed against fp64 (exact inputs at 0 and 1e3; fp64 inputs at 0 .. 9e14; one cloud exact, the other not): all
     256 queries must go to the rescan -- a certificate that is too narrow certifies the wrong granule and returns a wrong row;
  C  winner and runner-up 2^-12 apart at rows 0, 63|64, 1023|1024, 2047|2048, 65535|65536 and n - 1, n = 1 .. 66 565 (33 splits):
     no query may go to the rescan -- a certificate that is too wide computes the same answers ~80 times slower, and only the
     count shows it;
  T  exact ties across granules, tiles, splits, rescan slices and rescan threads, 0 / 1 / 32 / 33 / 600 of them (no rescan / the
     split regime up to kSplitMax / the list regime past one list's 512 workgroups), in-granule ties settled by k2_refine;
     k32_wide: the split regime on 512 workgroups with tied partials 256 slices apart, which one thread of the fold reads;
  S  a cloud against itself: neighbours in other granules and across the scan workgroup's own rows, duplicates, 130 equal points;
  rev  R (both mixed-precision ways and exact), C 3077 and T k600 the other way round through nn(1): the second cloud on the
     query side of all three kernels, 3077 queries against 8 .. 700 rows;
  L  a uniform pair scaled down until fp32 distances are subnormal and 0, through brute, grid and auto: results only.

The split regime's ticket is not visible from outside; the sequence test reads it off the results instead: were it left non-zero,
the next split-regime launch would never see its last ticket, emit nothing, and leave the previous case's rows in place -- so the
cases that follow each other there have different answers in the same slots.  tests/test_brute_planted_host.py proves the cases."""
import json

import numpy as np
import pytest

import brute_planted as bp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from open_pcc_metric_amd import _native as nat
    e = nat.Engine(0)
    e.nn_want_idx(True)
    yield e
    e.close()


def _load(eng, c):
    """Cloud 0 searches cloud 1 in direction 0 and itself in direction 2; in direction 1 cloud 1 searches cloud 0."""
    eng.set_cloud(1 if c.direction == 1 else 0, c.queries)
    eng.set_cloud(0 if c.direction == 1 else 1, c.searched)


def _search(eng, c, engine="brute", count=True):
    """One search of the case's direction on this context's shard -> flagged count; asserts rows, d2, kernels, splits."""
    d = c.direction
    eng.nn(d, engine)
    b, e = eng.shard_range(d)
    rows, d2 = bp.truth(c)
    idx, got = eng.fetch_nn(d)
    bad = np.flatnonzero((idx != rows[b:e]) | (got != d2[b:e]))
    assert len(bad) == 0, (f"{c.name} [{b}, {e}) {engine}: {len(bad)} of {e - b} differ, first at query {b + bad[0]}: row {idx[bad[0]]} d2 {got[bad[0]]!r}, "
                           f"oracle row {rows[b + bad[0]]} d2 {d2[b + bad[0]]!r}")
    if not count or e == b:
        return 0
    self_ = "true" if c.self_search else "false"
    path = eng.last_path(d)
    assert path == [f"k1_scan<8, {self_}>", f"k2_refine<{self_}>", f"k2b_fallback<{self_}>"], path
    stats = eng.nn_stats(d)
    want = int(bp.model(c).flag[b:e].sum())
    print(json.dumps({c.name: {"rows": [b, e], "flagged": [want, stats["fallback_queries"]], "splits": stats["splits"]}}))
    assert stats["splits"] == bp.splits_for(e - b, len(c.searched))[0]
    assert stats["fallback_queries"] == want, f"{c.name}: {stats['fallback_queries']} queries went to the exact rescan, the model of the certificate flags {want}"
    return stats["fallback_queries"]


@pytest.mark.parametrize("name", bp.COUNTED)
def test_planted_case_is_exact_and_flags_what_the_model_flags(eng, name):
    c = bp.case(name)
    want = bp.predicted_flagged(c)
    _load(eng, c)
    assert _search(eng, c) == want
    if name == f"C_{bp.C_BIG}":
        assert eng.nn_stats(0)["splits"] == 33
    if name in bp.R_CASES:
        assert want == 256
    if name in bp.C_NAMES:
        assert want == 0


def test_split_and_list_regimes_follow_each_other_on_one_context(eng):
    """k = 32 (split regime), k = 33 (list regime), another k = 32, and after drop_caches() the first again: every run exact, which
    the third and fourth can only be if the split regime's ticket was back at zero after the run before (module docstring)."""
    a, l, b = bp.case("T_k32"), bp.case("T_k33"), bp.case("T_k32_b")
    assert not set(a.want_rows[:32]) & set(b.want_rows[:32]) and np.array_equal(a.searched, b.searched)
    _load(eng, a)
    assert _search(eng, a) == 32
    for c in (l, b, a):
        eng.set_cloud(0, c.queries)
        assert _search(eng, c) == c.tie_queries
    eng.drop_caches()
    assert _search(eng, a) == 32
    eng.set_cloud(0, b.queries)
    assert _search(eng, b) == 32


@pytest.mark.parametrize("name", ["R_fp64_4e6", "S_4100"])
def test_shards_reassemble_and_their_counts_add_up(eng, name):
    """Three ranks' rows of one direction: the first query row is not 0 (q_begin in the scan's SELF mask, in k2_refine and in the
    rescan), the pieces are the unsharded answer and the flagged counts sum to the model's."""
    c = bp.case(name)
    _load(eng, c)
    total, covered = 0, 0
    try:
        for rank in range(3):
            eng.set_shard_dir(c.direction, rank, 3)
            b, e = eng.shard_range(c.direction)
            assert (b, e) == bp.shard_of(len(c.queries), rank, 3) and b == covered
            covered = e
            total += _search(eng, c)
    finally:
        eng.set_shard_dir(c.direction, 0, 1)
    assert covered == len(c.queries) and total == bp.predicted_flagged(c)


@pytest.mark.parametrize("rounded", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("scale", bp.L_SCALES)
def test_scale_ladder_results(eng, scale, rounded):
    c = bp.family_l(scale, rounded)
    _load(eng, c)
    for engine in ("brute", "grid", "auto"):
        _search(eng, c, engine, count=False)
