"""Planted columns for the left-to-right column sum (k_colsum_approx / k_colsum_units / k_colsum_chain, pccm_color.hip), each with a
proof -- on the host, about the DATA -- that the column has the property its name claims.  No GPU, no library: NumPy and math only.

The kernels promise np.add.reduce(a, axis=0) bit for bit by guessing the binade of the running sum from an any-order sum and
checking the guess against the true running sum.  Random columns leave most of that check idle: the any-order and the true sum
agree to ~1e-13, so they name different binades only where a crossing is flagged anyway.  The columns here pull the two sums
apart on purpose, land the sum on a binade's end (and one unit past it) at every level of the walk, plant exact ties against
odd and even sums, cross more binades than the kernels list or stage, and climb across the 2^-900 limit below which the walk
takes no records at all.

The proofs speak about the true left-to-right sum (np.cumsum, which is that sum: tests/test_colsum_planted_host.py pins it
against a Python loop) and about exact prefix sums (math.fsum).  They never model the order in which the kernels form their
approximate sums; the one thing taken from the code is a bound on that sum's error:

    MARGIN = 256 units of 2^-53.  In the drift columns and the rounded landings one element is ~1 and all others are < 2^-49, so a
    partial sum of small elements alone stays below 41 000 * 2^-49 < 2^-33 and every addition among them rounds by < 2^-86: all of
    those together move an any-order sum by < 2^-70.  The additions that matter are the ones on the path of the large element through
    the kernels' fixed reduction tree.  Counted in pccm_color.hip: k_colsum_approx 8 per-thread adds + 6 shuffle steps + 16 wave
    partials = 30; k_colsum_units `before` 1 + 6, the sixteen s_red 16, up to 15 s_pre (whose own depth, 8 + 6, is parallel to
    that of `before`, not in series with it), then `end = start + mine` or the eight `front += sg[j]` of the groups: 8.
    30 + 7 + 16 + 15 + 8 = 76 < 100 additions of partial sums below 2, each rounding by at most 2^-53.  So where the EXACT prefix
    is more than 256 units away from 1.0, every guess the kernels can form lies on the exact prefix's side of 1.0.
"""
import math

import numpy as np

CHUNK, SUB, GROUP = 8192, 512, 64          # kSumChunk, kSumSub, one wave's group (pccm_color.hip)
U53, U52 = 2.0 ** -53, 2.0 ** -52          # the unit in the last place of binade -1 ([0.5, 1)) and of binade 0 ([1, 2))
MARGIN = 256


def cumsum(x):
    """The true left-to-right sum after every row (np.cumsum adds one after the other)."""
    return np.cumsum(np.asarray(x, dtype=np.float64))


def axis0_sum(x):
    """np.add.reduce(axis=0) of the column as one of three: the reference of the GPU tests.  (Of a 1-D array np.add.reduce is a
    PAIRWISE sum; down the rows of a C-contiguous (N, 3) array it adds one row after the other.)"""
    return float(np.add.reduce(np.c_[x, x, x], axis=0)[0])


def ilogb(v):
    return math.frexp(v)[1] - 1


def units_total(x, e):
    """SUM rint(x / u) * u for u = the unit of binade e: what a run of elements adds to a sum that stays in binade e (no ties)."""
    u = 2.0 ** (e - 52)
    return float(np.sum(np.rint(np.asarray(x) / u))) * u


def units_count(x, e):
    """SUM rint(x / u), the same total as a bare count of units."""
    return float(np.sum(np.rint(np.asarray(x) / 2.0 ** (e - 52))))


def _filler(count, u, seed):
    """k*u + 0.3*u, k in 1..5: each add rounds 0.3 u away, so the rounding decides the sum."""
    k = np.random.default_rng(seed).integers(1, 6, count).astype(np.float64)
    return (k + 0.3) * u


# ---- 1. the true sum ahead of / behind every any-order sum ----------------------------------------------------------------------
def drift_up(n=5 * CHUNK):
    """x[0] = 1 - 20000 * 2^-53, then 0.51 * 2^-53: in binade -1 every add rounds UP to a whole unit, the true sum is exactly 1.0
    at row 20000 and stays there (0.255 of binade 0's unit rounds to nothing); the exact prefix reaches 1.0 only near row 39216."""
    x = np.full(n, 0.51 * U53)
    x[0] = 1.0 - 20000 * U53
    return x


def check_drift(x=None):
    x = drift_up() if x is None else x
    cs = cumsum(x)
    assert axis0_sum(x) == 1.0 and cs[-1] == 1.0
    assert cs[19999] < 1.0 and cs[20000] == 1.0                                  # the crossing row
    assert round((math.fsum(x[:38400]) - 1.0) / U53) == -417 and round((math.fsum(x[:39424]) - 1.0) / U53) == 106
    starts = [s for s in range(SUB, len(x), SUB) if cs[s - 1] == 1.0 and math.fsum(x[:s]) < 1.0 - MARGIN * U53]
    assert len(starts) >= 30, len(starts)
    # the sub-chunk that holds the true crossing is not the one the exact prefix crosses in: no any-order sum flags it for that
    s0 = 20000 // SUB * SUB
    assert not (math.fsum(x[:s0]) < 1.0 <= math.fsum(x[:s0 + SUB]))
    assert math.fsum(x[:s0 + SUB]) < 1.0 - MARGIN * U53
    # accepting the guess (binade -1) where the true sum is 1.0: the sub-chunk's total in the wrong unit is not nothing
    for s in starts:
        assert cs[s + SUB - 1] == 1.0
        assert cs[s - 1] + units_total(x[s:s + SUB], -1) != cs[s + SUB - 1]          # ... in the guess's unit
        assert cs[s - 1] + units_count(x[s:s + SUB], -1) * U52 != cs[s + SUB - 1]      # ... nor counted in the true sum's
    return starts


def drift_stall(n=3 * CHUNK):
    """x[0] = 1 - 2^-53, then 2^-55 (a quarter unit of binade -1): the true sum never moves, the exact sum is above 1 after five
    elements.  Every later guess says binade 0, the walk's sum is in binade -1.  (A quarter unit of binade -1 is an eighth of
    binade 0's: the wrong-unit totals are zero here, so this column pins the PATH -- sub-chunks nobody flagged, redone from their
    elements -- while drift_up() and drift_behind() pin the comparison of the guess itself.)"""
    x = np.full(n, 2.0 ** -55)
    x[0] = 1.0 - U53
    return x


def check_stall(x=None):
    x = drift_stall() if x is None else x
    cs = cumsum(x)
    assert axis0_sum(x) == x[0] and np.all(cs == x[0]) and ilogb(cs[-1]) == -1
    assert math.fsum(list(x[:6]) + [-1.0]) > 0.0                # (exactly: 1 + 2^-55 itself is no double)
    starts = [s for s in range(SUB, len(x), SUB) if ilogb(cs[s - 1]) == -1 and math.fsum(x[:s]) > 1.0 + MARGIN * U53]
    assert len(starts) >= 40, len(starts)
    return starts


def drift_behind(n=4 * CHUNK):
    """drift_stall() with teeth: x[0] = 1 - 3200 * 2^-53; rows 32, 64, 96, ... hold 2.6 * 2^-53 (three units of binade -1, but 1.3 ->
    ONE unit of binade 0), all others 2^-55.  The true sum gains three units per 32 rows and stays below 1; the exact sum is above
    1 + 256 units from row 10700 on.  Taking a guess of binade 0 for good counts one where three are due."""
    x = np.full(n, 2.0 ** -55)
    x[32::32] = 2.6 * U53
    x[0] = 1.0 - 3200 * U53
    return x


def check_behind(x=None):
    x = drift_behind() if x is None else x
    cs = cumsum(x)
    assert cs[-1] < 1.0 and cs[-1] == x[0] + 3 * ((len(x) - 1) // 32) * U53
    starts = [s for s in range(SUB, len(x), SUB) if ilogb(cs[s - 1]) == -1 and math.fsum(x[:s]) > 1.0 + MARGIN * U53]
    assert len(starts) >= 40, len(starts)
    for s in starts:
        assert cs[s - 1] + units_total(x[s:s + SUB], 0) != cs[s + SUB - 1]
        assert cs[s - 1] + units_count(x[s:s + SUB], 0) * U53 != cs[s + SUB - 1]
    return starts


# ---- 2. landings on a binade's end, and one unit past it -------------------------------------------------------------------------
LANDING_ROWS = {
    "chunk": 2 * CHUNK - 1,                                  # the last row of a chunk
    "sub": CHUNK + 5 * SUB - 1,                              # the last row of a sub-chunk inside a chunk
    "group": CHUNK + 3 * SUB + 2 * GROUP - 1,                # the last row of a group inside a sub-chunk
    "mid": CHUNK + 3 * SUB + 2 * GROUP + 29,                 # a row in the middle of a group
}
LANDING_TAIL = 700                                           # rows of filler behind the landing (>= 600)


def landing(level, kind, over):
    """The running sum climbs through binade -1 and arrives at 1.0 on row L = LANDING_ROWS[level].
    kind "dyadic":  x[0] = 1 - 3 L * 2^-53, rows 1..L hold 3 * 2^-53: every partial sum is exact, any-order sums included, so the
                    kernels see the landing coming (the record that holds it is flagged, the landing is met one level down).
    kind "rounded": x[0] = 1 - L * 2^-53, rows 1..L hold 0.51 * 2^-53, each rounding up to a whole unit: the true sum lands on
                    1.0, every any-order sum stays ~0.49 L units short -- nothing is flagged, and the landing is met by the
                    largest record that ends on row L.
    over = 1:       row L holds 1.3 units more than the room that is left, so the sum passes the end by exactly one old unit and a bit: 1 + 2^-52.  (Taking
                    the run for `room + 1` units instead gives (2^53 + 1) * 2^-53 = 1.0, a tie to even.)
    Behind row L: LANDING_TAIL rows of k*u + 0.3 u in binade 0's unit."""
    L = LANDING_ROWS[level]
    x = np.empty(L + 1 + LANDING_TAIL)
    if kind == "dyadic":
        x[:L + 1] = 3 * U53
        x[0] = 1.0 - 3 * L * U53
    else:
        x[:L + 1] = 0.51 * U53
        x[0] = 1.0 - L * U53
    if over:
        x[L] = ((3 if kind == "dyadic" else 1) + 1.3) * U53
    x[L + 1:] = _filler(LANDING_TAIL, U52, L + over)
    return x


def landings():
    return {f"landing_{level}_{kind}{'_over' if over else ''}": landing(level, kind, over)
            for level in LANDING_ROWS for kind in ("dyadic", "rounded") for over in (0, 1)}


def check_landing(level, kind, over, x=None):
    x = landing(level, kind, over) if x is None else x
    L = LANDING_ROWS[level]
    cs = cumsum(x)
    assert {"chunk": (L + 1) % CHUNK == 0,
            "sub": (L + 1) % SUB == 0 and (L + 1) % CHUNK != 0,
            "group": (L + 1) % GROUP == 0 and (L + 1) % SUB != 0,
            "mid": 8 < (L + 1) % GROUP < 56}[level]
    step = 3 if kind == "dyadic" else 1
    assert cs[L - 1] == 1.0 - step * U53                     # binade -1 up to the row before, `step` units of room left
    if kind == "dyadic":
        assert all(cs[i] == math.fsum(x[:i + 1]) for i in range(0, L, 997))        # exact partial sums
    else:
        assert math.fsum(x[:L + 1]) < 1.0 - MARGIN * U53     # the exact prefix is far short of the landing
    if over:
        assert cs[L] == 1.0 + U52
        assert cs[L - 1] + (step + 1) * U53 == 1.0           # ... which `room + 1` units would not reach
    else:
        assert cs[L] == 1.0
    tail = x[L + 1:]
    assert len(tail) >= 600 and np.all(np.rint(tail / U52) * U52 != tail)
    assert cs[-1] == cs[L] + units_total(tail, 0)            # every filler rounds 0.3 u away ...
    assert cs[-1] != cs[L] + math.fsum(tail)                 # ... and that decides the result
    return L


# ---- 3. exact ties ------------------------------------------------------------------------------------------------------------------
def tie_odd(n=4096 + 1):
    """x[0] = 1 + 2^-52 (odd in units of 2^-52), then 2^-53, 2^-52, 2^-53, 2^-52, ...: every 2^-53 is an exact tie against an odd
    sum and rounds up."""
    x = np.empty(n)
    x[0] = 1.0 + U52
    x[1::2] = U53
    x[2::2] = U52
    return x


def tie_even(n=4096 + 1):
    """x[0] = 1 (even), then 2^-53, 2^-51, ...: every tie meets an even sum and stays."""
    x = np.empty(n)
    x[0] = 1.0
    x[1::2] = U53
    x[2::2] = 2 * U52
    return x


TIE_EDGE_ROWS = (GROUP, 2 * GROUP - 1, SUB, 2 * SUB - 1, CHUNK - 1, CHUNK)


def tie_edges(n=CHUNK + SUB + 1):
    """Ties on the first and the last row of a group, of a sub-chunk and of a chunk.  Filler 2.3 units (parity kept), x[0] odd;
    a row of 1.3 units behind each tie makes the sum odd again -- except behind row CHUNK - 1, so that the tie on row CHUNK
    meets an even sum and stays."""
    x = np.full(n, 2.3 * U52)
    x[0] = 1.0 + U52
    for r in TIE_EDGE_ROWS:
        x[r] = U53
        if r + 1 not in TIE_EDGE_ROWS:
            x[r + 1] = 1.3 * U52
    return x


def check_ties():
    units = lambda v: round((v - 1.0) / U52)
    x = tie_odd()
    cs = cumsum(x)
    assert units(cs[-1]) - units(x[0]) == 4096                                   # 2048 ties rounded up + 2048 whole units
    assert float(np.sum(np.rint(x[1:] / U52))) == 2048                           # a model without ties gains half of that
    assert all(units(cs[i - 1]) % 2 == 1 and cs[i] == cs[i - 1] + U52 for i in range(1, len(x), 2))
    x = tie_even()
    cs = cumsum(x)
    assert units(cs[-1]) == 4096
    assert all(units(cs[i - 1]) % 2 == 0 and cs[i] == cs[i - 1] for i in range(1, len(x), 2))
    assert float(np.sum(np.ceil(x[1:] / U52))) == 4096 + 2048                    # "ties go up" would gain this
    x = tie_edges()
    cs = cumsum(x)
    for r in TIE_EDGE_ROWS:
        assert x[r] == U53
        odd = units(cs[r - 1]) % 2 == 1
        assert odd == (r != CHUNK)
        assert cs[r] == (cs[r - 1] + U52 if odd else cs[r - 1])
    assert [r % GROUP for r in TIE_EDGE_ROWS[:2]] == [0, GROUP - 1] and [r % SUB for r in TIE_EDGE_ROWS[2:4]] == [0, SUB - 1]
    assert [r % CHUNK for r in TIE_EDGE_ROWS[4:]] == [CHUNK - 1, 0]


# ---- 4. more crossings than are staged (14) or listed (64) -----------------------------------------------------------------------
def crossings(nsub=112):
    """Seven chunks.  Every sub-chunk but the first opens with an element equal to the running sum so far -- the sum doubles, into the
    next binade -- followed by 511 rows of k*u + 0.3 u in the new binade's unit.  Starts at 2^-60, ends near 2^51."""
    x = np.empty(nsub * SUB)
    s = 0.0
    for k in range(nsub):
        first = 2.0 ** -60 if k == 0 else s
        e = ilogb(s + first)
        part = np.concatenate(([first], _filler(SUB - 1, 2.0 ** (e - 52), 1000 + k)))
        x[k * SUB:(k + 1) * SUB] = part
        s = float(cumsum(np.concatenate(([s], part)))[-1])
    return x


def check_crossings(x=None):
    x = crossings() if x is None else x
    cs = cumsum(x)
    assert np.all(np.isfinite(x)) and np.all(x > 0) and np.isfinite(cs[-1]) and cs[-1] < 2.0 ** 60
    nsub = len(x) // SUB
    crossed = [k for k in range(1, nsub) if ilogb(cs[k * SUB - 1]) != ilogb(cs[(k + 1) * SUB - 1])]
    assert len(crossed) > 64 and len(crossed) >= 100, len(crossed)
    decided = [k for k in crossed[64:] if cs[(k + 1) * SUB - 1] != cs[k * SUB] + math.fsum(x[k * SUB + 1:(k + 1) * SUB])]
    assert decided, "no late sub-chunk whose rounding decides the sum"
    for k in crossed:                                        # the crossing is the opening element, the rest stays in the binade
        assert x[k * SUB] == cs[k * SUB - 1] and cs[k * SUB] == 2 * cs[k * SUB - 1]
        assert ilogb(cs[k * SUB]) == ilogb(cs[(k + 1) * SUB - 1])
    return crossed


# ---- 5. across the 2^-900 limit --------------------------------------------------------------------------------------------------
def threshold(n=2 * CHUNK + SUB):
    """The running sum starts among subnormals, climbs through 2^-900 -- below which units_of() calls a sum unusable -- inside the
    second chunk and goes on for ten more binades; subnormal elements are sprinkled over the whole column."""
    rng = np.random.default_rng(900)
    x = rng.integers(1, 1 << 20, n).astype(np.float64) * 2.0 ** -1074          # subnormals: chunk 0 sums to ~2^-1042
    up = np.arange(CHUNK + 700, n)
    x[up] = (rng.integers(1, 6, len(up)) + 0.3) * np.exp2(-913.0 + (up - up[0]) / 350.0)
    x[up[5::7]] = rng.integers(1, 1 << 20, len(up[5::7])) * 2.0 ** -1074
    return x


def check_threshold(x=None):
    x = threshold() if x is None else x
    cs = cumsum(x)
    lim = 2.0 ** -900
    assert np.all(x > 0) and cs[CHUNK - 1] < 2.0 ** -1022 and cs[-1] > lim * 2.0 ** 10
    row = int(np.searchsorted(cs, lim))                      # the first row at or above the limit
    assert CHUNK + SUB < row < 2 * CHUNK - SUB and row % GROUP not in (0, GROUP - 1)
    sub = x < 2.0 ** -1022
    assert sub[:row].sum() > CHUNK and sub[row:].sum() > 100
    assert cs[-1] != math.fsum(x)                            # rounding decides
    return row


# ---- everything, and the ragged ends ---------------------------------------------------------------------------------------------
def columns():
    """name -> column, every planted column at its full length."""
    c = {"drift_up": drift_up(), "drift_stall": drift_stall(), "drift_behind": drift_behind()}
    c.update(landings())
    c.update({"tie_odd": tie_odd(), "tie_even": tie_even(), "tie_edges": tie_edges(), "crossings": crossings(), "threshold": threshold()})
    return c


def ragged_lengths(n):
    """n itself, and the lengths that end one row after the last chunk, sub-chunk and group boundary below n."""
    out = [n]
    for unit, coarser in ((CHUNK, None), (SUB, CHUNK), (GROUP, SUB)):
        b = (n - 2) // unit * unit
        while b > 0 and coarser and b % coarser == 0:
            b -= unit
        if b > 0 and b + 1 not in out:
            out.append(b + 1)
    return out


def lengths(name, x):
    """The lengths a planted column is summed at: ragged_lengths(), and for a landing the length that ends one row behind it."""
    out = ragged_lengths(len(x))
    if name.startswith("landing_"):
        cut = LANDING_ROWS[name.split("_")[1]] + 2
        if cut not in out:
            out.append(cut)
    return out


def check_all():
    check_drift()
    check_stall()
    check_behind()
    for level in LANDING_ROWS:
        for kind in ("dyadic", "rounded"):
            for over in (0, 1):
                check_landing(level, kind, over)
    check_ties()
    check_crossings()
    check_threshold()
    for name, x in columns().items():
        assert x.dtype == np.float64 and x.ndim == 1 and np.all(x >= 0) and np.all(np.isfinite(x)), name
        assert len(x) <= 7 * CHUNK, name
