"""The planted cases of tests/brute_planted.py on the host: the fp32 helper of the model is the scan's arithmetic, every case has
the property its family claims, no case whose flagged count the GPU test asserts lies in the band where the device's own rounding
of thr could decide, and the shipped certificate formula certifies no wrong answer on any of them."""
import numpy as np
import pytest

import brute_planted as bp


# ---- the model's arithmetic ---------------------------------------------------------------------------------------------------
def _random_triples(count):
    """fp32 differences whose squares meet at every relative scale, a third of them placed beside a rounding boundary of the sum."""
    rng = np.random.default_rng(81)
    t = (rng.uniform(1.0, 2.0, (count, 3)) * 2.0 ** rng.integers(-40, 40, (count, 1)) * 2.0 ** rng.integers(-26, 3, (count, 3))).astype(np.float32)
    # dy tiny beside dx*dx: the sum sits a hair off an fp32 number or off a midpoint, where a second rounding goes wrong
    k = count // 3
    t[:k, 1] = (t[:k, 0].astype(np.float64) * 2.0 ** rng.integers(-30, -10, k)).astype(np.float32)
    t[:k // 2, 2] = 0
    # dy = Y * 2^j with Y odd in [2^12, 2^12.5): dy*dy is EXACTLY midway between two fp32 numbers, and a dx*dx some 80 binades
    # below it, which fp64 cannot hold beside it, is what decides the direction
    j = np.arange(k, k + 2000)
    t[j, 1] = ((2 * rng.integers(2048, 2896, 2000) + 1) * 2.0 ** rng.integers(-20, 20, 2000)).astype(np.float32)
    t[j, 0] = (t[j, 1].astype(np.float64) * 2.0 ** -40).astype(np.float32)
    t[j, 2] = 0
    t[0], t[1], t[2] = (0, 0, 0), (1e-30, 1e-30, 1e-30), (1e18, 1e18, 1e18)         # zero, underflow to subnormal, the padding's size
    return t


def test_the_fp32_helper_is_the_scan_arithmetic_rounded_once():
    t = _random_triples(100_000)
    got = bp.sq_sum32(t[:, 0], t[:, 1], t[:, 2])
    want = np.array([bp.sq_sum32_fraction(*row) for row in t])
    bad = np.flatnonzero(got.astype(np.float64) != want)
    assert len(bad) == 0, (len(bad), t[bad[:3]], got[bad[:3]], want[bad[:3]])
    # the sample has teeth: the fma emulated by rounding through fp64 differs from the exact one on it
    x = t.astype(np.float64)
    naive = (x[:, 1] * x[:, 1] + (t[:, 0] * t[:, 0]).astype(np.float64)).astype(np.float32)
    naive = (x[:, 2] * x[:, 2] + naive.astype(np.float64)).astype(np.float32)
    assert np.count_nonzero(naive.astype(np.float64) != want) >= 10
    assert np.count_nonzero((want > 0) & (want < bp.TINY32)) >= 1                    # subnormal results are part of the pin


def test_fp32_subtraction_is_the_correctly_rounded_difference():
    from fractions import Fraction
    rng = np.random.default_rng(83)
    a = (rng.uniform(-2, 2, 2000) * 2.0 ** rng.integers(-20, 50, 2000)).astype(np.float32)
    b = (a.astype(np.float64) * rng.uniform(0.5, 1.5, 2000) + rng.uniform(-1, 1, 2000)).astype(np.float32)
    for x, y, d in zip(a.tolist(), b.tolist(), (a - b).tolist()):
        want = Fraction(x) - Fraction(y)
        assert abs(d) == float(bp.round32_fraction(abs(want))) and (d < 0) == (want < 0) or want == 0 == d


def test_the_split_rule_and_the_rescan_plan():
    assert bp.splits_for(8, bp.C_BIG) == (33, 2)                    # 66 tiles, at most 64 splits -> 2 tiles a split, 33 splits
    assert bp.splits_for(2048, bp.C_BIG) == (33, 2) and bp.splits_for(2049, bp.C_BIG) == (33, 2)
    assert bp.splits_for(256, bp.N0) == (4, 1)                      # three full tiles and the ragged one beside the padding
    assert bp.splits_for(1, 1) == (1, 1) and bp.splits_for(700, 1025) == (2, 1)
    assert bp.splits_for(4_000_000, 1_000_000)[0] == 4              # many query workgroups: few splits
    assert bp.rescan_plan(100, bp.N0, 32) == ("split", 100, 31) and bp.rescan_plan(100, bp.N0, 33)[0] == "list"
    assert bp.rescan_plan(600, 66, 32) == ("split", 512, 1) and bp.rescan_plan(1, bp.N0, 1) == ("split", 1, bp.N0)
    assert bp.rescan_plan(700, bp.N0, 600) == ("list", 512, 7) and bp.rescan_plan(50, bp.N0, 0)[0] == "none"
    assert bp.shard_of(256, 0, 3) == (0, 0) and bp.shard_of(256, 2, 3) == (128, 256) and bp.shard_of(4100, 1, 3) == (1408, 2816)


# ---- proofs common to every counted case ------------------------------------------------------------------------------------------
def _common(c, small=True):
    m = bp.model(c)
    rows, d2 = bp.truth(c)
    assert len(bp.band_violations(m)) == 0
    assert len(bp.unsound(m, rows)) == 0                                             # the reference certificate certifies no wrong answer
    if small:
        brows, bd2 = bp.brute64(c.queries, c.searched, c.self_search)
        assert np.array_equal(rows, brows) and np.array_equal(d2, bd2)               # kd-tree == definition, ties to the smallest row
    return m, rows, d2


@pytest.mark.parametrize("name", list(bp.R_CASES))
def test_reversal_triples_reverse_and_are_flagged(name):
    c = bp.case(name)
    m, rows, d2 = _common(c)
    k = np.arange(bp.R_TRIPLES)
    near, far = bp.R_NEAR_ROW(k), bp.R_FAR_ROW(k)
    assert c.queries.shape == (256, 3) and c.searched.shape == (bp.N0, 3) and np.abs(c.searched).max() < 1e15
    assert m.exact == (c.kind == "exact")
    assert bp.is_exact32(c.queries) == (c.kind in ("exact", "q_exact")) and bp.is_exact32(c.searched) == (c.kind in ("exact", "r_exact"))
    assert np.array_equal(rows, near)                                                # fp64: the near point, strictly
    assert np.all(bp.brute_d64(c.queries, c.searched[near]) < bp.brute_d64(c.queries, c.searched[far]))
    d_near = bp.dist32(c.queries.astype(np.float32), c.searched[near].astype(np.float32))
    d_far = bp.dist32(c.queries.astype(np.float32), c.searched[far].astype(np.float32))
    assert np.all(d_far <= d_near) and np.count_nonzero(d_far < d_near) >= 200       # fp32: the far point, or a tie
    assert np.count_nonzero(d_far == d_near) == c.fp32_ties
    assert np.array_equal(m.g1, far // bp.G) and np.all(m.g1 < near // bp.G)         # the scan's winner granule is the wrong one
    assert np.array_equal(m.b1, d_far) and np.array_equal(m.b2, d_near)
    # isolation: every other searched point is at least 4 radii away
    others = np.ones(bp.N0, bool)
    others[near], others[far] = False, False
    gap = np.sqrt(np.min(bp.brute_d64(c.queries[:, None, :], c.searched[None, others, :]), axis=1))
    assert np.all(gap >= 4.0 * np.sqrt(bp.brute_d64(c.queries, c.searched[far])))
    assert m.flag.all() and bp.predicted_flagged(c) == 256
    print(name, "fp32 ties", c.fp32_ties, "largest reversal b2/b1 - 1 =", float(np.max(m.b2.astype(np.float64) / np.maximum(m.b1, 1e-300) - 1)))


def test_the_reversals_separate_the_mutant_certificates():
    """What each family is there for: a certificate that is too narrow certifies a wrong answer on it (the model with that formula)."""
    def wrong(name, slack_of, factor=1.0 + 2.0 ** -20):
        c = bp.case(name)
        m = bp.model(c)
        rb1 = np.sqrt(m.b1.astype(np.float64))
        tq = rb1 * factor + slack_of(c, m, rb1)
        certified = m.b2.astype(np.float64) > tq * tq * (1.0 + 2.0 ** -30) + 1.0e-36
        return int(np.count_nonzero(certified))                 # every query of R is a reversal: certified means wrong
    zero = lambda c, m, rb1: 0.0                                # noqa: E731
    for name in ("R_exact_0", "R_exact_1e3"):                   # thr = b1
        assert wrong(name, zero, factor=1.0) >= 100
    for name in ("R_fp64_1e3", "R_fp64_4e6", "R_fp64_1e9", "R_fp64_9e14", "R_q_exact_1e6", "R_r_exact_1e6"):
        assert wrong(name, zero) >= 100                         # slack = 0, or `exact` read from one cloud only
    for name in ("R_fp64_1e9", "R_fp64_9e14"):                  # slack on sqrt(b1) only
        assert wrong(name, lambda c, m, rb1: 2.0 ** -20 * rb1) >= 100


@pytest.mark.parametrize("name", bp.C_NAMES)
def test_certified_pairs_are_certified(name):
    c = bp.case(name)
    n = len(c.searched)
    m, rows, d2 = _common(c, small=n <= bp.N0)
    assert bp.model(c).exact and np.array_equal(rows, c.want_rows)
    assert bp.predicted_flagged(c) == 0
    seams = {r for p in c.pairs for r in p}
    assert n < 2 or {0, n - 1} <= seams
    for k in (bp.G, bp.T, bp.W, 64 * bp.T):
        assert k >= n or {k - 1, k} <= seams
    if c.pairs:
        assert sorted(c.want_rows.tolist()) == sorted(seams)                         # every planted row wins once and loses once
        ratio = np.sqrt(m.b2.astype(np.float64) / m.b1)
        cross = np.array([p[0] // bp.G != p[1] // bp.G for p in c.pairs]).repeat(2)
        assert np.all(np.abs(ratio[cross] - (1 + 2.0 ** -12)) < 2.0 ** -20)          # runner-up in another granule: 2^-12 farther out
        assert np.all(m.b2[cross] <= 4.0 * m.thr[cross])                             # a certificate four times too wide flags them all
    if n == bp.C_BIG:
        assert bp.splits_for(len(c.queries), n) == (33, 2) and len(c.queries) <= 2048
        assert (2047, 2048) in c.pairs and (65535, 65536) in c.pairs and (0, n - 1) in c.pairs
        assert 65536 == 32 * 2 * bp.T                                                # the first row of the last split


@pytest.mark.parametrize("name", bp.T_NAMES)
def test_tie_queries_are_the_flagged_queries(name):
    c = bp.case(name)
    m, rows, d2 = _common(c)
    k = c.tie_queries
    assert bp.is_exact32(c.queries) and bp.is_exact32(c.searched)
    assert np.array_equal(rows, c.want_rows) and np.array_equal(d2, c.want_d2)
    assert np.array_equal(np.flatnonzero(m.flag), np.arange(k)) and bp.predicted_flagged(c) == k
    assert np.all(m.b2[k:] >= 1.0)
    dq = bp.brute_d64(c.queries[:, None, :], c.searched[None, :, :])
    for i, tied in enumerate(c.tied_rows):                                           # exactly the planted rows tie, in >= 2 granules
        assert np.flatnonzero(dq[i] == d2[i]).tolist() == tied and len({r // bp.G for r in tied}) >= 2
    regime, nb, per = bp.rescan_plan(len(c.queries), len(c.searched), k)
    assert regime == {0: "none"}.get(k, "split" if k <= bp.SPLIT_MAX else "list")
    if name in bp.T_CASES and k >= 32:
        spans = [sorted({(r[j + 1] - r[j]) for j in range(len(r) - 1)}) for r in c.tied_rows]
        assert {1, 64, 256, 1024} <= {s for sp in spans for s in sp}                  # duplicates and ties at every planted distance
        assert len({r[0] // bp.T for r in c.tied_rows}) >= 1 and len({r[-1] // bp.T for r in c.tied_rows}) == 3
        if regime == "split":                                                        # tied rows in different slices of ceil(n / nb) rows
            assert sum(len({r // per for r in tied}) >= 2 for tied in c.tied_rows) >= k * 3 // 4
        else:                                                                        # in different threads' strides, and in one stride
            assert sum(len({r % 256 for r in tied}) >= 2 for tied in c.tied_rows) >= k // 2
            assert sum(len({r % 256 for r in tied}) < len(tied) for tied in c.tied_rows) >= k // 8
    if name == "T_k32_wide":                                                         # two tied partials met by one thread of the fold
        assert (regime, nb, per) == ("split", 512, 7)
        assert sum(tied[-1] // per - tied[0] // per == 256 for tied in c.tied_rows) >= 3
    if name == "T_k1_alone":
        assert (regime, nb, per) == ("split", 1, bp.N0)
    if name == "T_n66":
        assert (regime, nb, per) == ("split", 512, 1)
    if name in bp.T_CASES and len(c.queries) > k:                                    # the in-granule ties are certified
        inside = np.arange(k, k + bp.T_INSIDE_N)
        assert np.all(np.sum(dq[inside] == d2[inside, None], axis=1) == 2) and not m.flag[inside].any()


@pytest.mark.parametrize("name", bp.S_NAMES)
def test_self_search_cases(name):
    c = bp.case(name)
    m, rows, d2 = _common(c)
    n = len(c.queries)
    assert c.self_search and np.array_equal(rows, c.want_rows) and np.array_equal(d2, c.want_d2)
    assert not np.any(rows == np.arange(n))
    bp.predicted_flagged(c)
    if name.startswith("S_identical"):
        assert m.flag.all() and n == 130
        return
    other = rows // bp.G != np.arange(n) // bp.G
    if n >= 65:
        assert rows[0] // bp.G >= 1                                                  # the neighbour sits in another granule
    if n >= 1025:
        assert other.sum() >= n // 2
    if n > bp.W:
        assert rows[bp.W - 1] == bp.W and rows[bp.W] == bp.W - 1                     # across the first scan workgroup's last own row
    if n > bp.W + 16:
        assert rows[bp.W - 48] == bp.W + 16 and rows[bp.W + 16] == bp.W - 48
    if n >= 1025:
        dup = d2 == 0
        assert np.count_nonzero(dup & (rows < np.arange(n))) >= 50 and np.count_nonzero(dup & (rows > np.arange(n))) >= 25


@pytest.mark.parametrize("rounded", [False, True])
@pytest.mark.parametrize("scale", bp.L_SCALES)
def test_the_certificate_stays_sound_down_the_scale_ladder(scale, rounded):
    c = bp.family_l(scale, rounded)
    m = bp.model(c)
    rows, d2 = bp.truth(c)
    brows, bd2 = bp.brute64(c.queries, c.searched)
    assert np.array_equal(rows, brows) and np.array_equal(d2, bd2)
    assert np.all(np.abs(c.queries.astype(np.float32)) >= bp.TINY32)                 # the coordinates stay normal fp32 numbers
    assert len(bp.unsound(m, rows)) == 0
    if scale <= 1e-18:
        assert m.flag.all()
    if scale <= 1e-23:
        assert np.all(m.b1 == 0)                                                     # the fp32 distances are gone altogether
    print(c.name, "flagged", int(m.flag.sum()), "of", len(m.flag), "subnormal", int(m.subnormal.sum()))


@pytest.mark.parametrize("name", bp.REV_NAMES)
def test_converse_searches(name):
    """Direction 1: the second cloud on the query side, the exactness of the two clouds in swapped roles."""
    c = bp.case(name)
    m, rows, d2 = _common(c)
    fwd = bp.case(name[:-4])
    assert c.direction == 1 and c.queries is fwd.searched and c.searched is fwd.queries
    assert m.exact == bp.model(fwd).exact
    print(name, "flagged", bp.predicted_flagged(c), "of", len(c.queries))
