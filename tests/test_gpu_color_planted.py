"""The colour kernels (pccm_color.hip) where random data leaves them idle:
A. the column sum on the planted columns of tests/colsum_planted.py -- guesses that are wrong without having been flagged, landings on
   a binade's end and one unit past it at every level of the walk, ties against odd and even sums, more crossings than are listed or
   staged, the 2^-900 limit -- against np.add.reduce(axis=0), bit for bit;
B. both directions of a pair in one launch with unequal chunk counts, the column maxima in the last partial chunk and in row 0;
C. k_rgb8_pack's decision that a float colour table is bytes / 255, and what depends on it;
D. NaN and infinite colours through pccm_color_reduce.
tests/test_colsum_planted_host.py proves on the host what the columns of A are; the mutants this file was checked against are
listed in DESIGN.md ("Colour: planted tests")."""
import functools

import numpy as np
import pytest

import colsum_planted as cp
from conftest import same_bits
from open_pcc_metric_amd import _native as nat
from oracle import oracle as orc
from test_gpu_color import _coloured

pytestmark = pytest.mark.gpu

SCHEMES = ("rgb", "ycc", "yuv")
LEFT, RIGHT = nat.DIR_LEFT, nat.DIR_RIGHT


@pytest.fixture(scope="module")
def engine():
    e = nat.Engine(0)
    yield e
    e.close()


def _hex(v):
    return [float(x).hex() for x in np.atleast_1d(v)]


# ---- A. the sum alone -------------------------------------------------------------------------------------------------------------
COLUMNS = cp.columns()
NAMES = list(COLUMNS)


def _fit(x, n):
    """The first n rows of a column; a shorter one is filled up with +0, which leaves every partial sum as it is."""
    return x[:n] if len(x) >= n else np.concatenate((x, np.zeros(n - len(x))))


@pytest.mark.parametrize("name", NAMES)
def test_planted_columns_sum_like_numpy(engine, name):
    """Every planted column at its own length and at its ragged cuts, beside two columns of other families (one column's flag list and
    staging must never serve another's), and once more with the three columns in another order."""
    i = NAMES.index(name)
    partners = [NAMES[(i + 7) % len(NAMES)], NAMES[(i + 13) % len(NAMES)]]
    assert len({name, *partners}) == 3
    for n in cp.lengths(name, COLUMNS[name]):
        assert n <= 7 * cp.CHUNK
        a = np.ascontiguousarray(np.c_[COLUMNS[name][:n], _fit(COLUMNS[partners[0]], n), _fit(COLUMNS[partners[1]], n)])
        want = np.add.reduce(a, axis=0)
        assert want[0] == cp.cumsum(a[:, 0])[-1]
        for order in ([0, 1, 2], [2, 0, 1]):
            got = engine.seq_colsum(a[:, order])
            assert same_bits(got, want[order]), (name, partners, n, order, _hex(got), _hex(want[order]))


# ---- pairs of coloured clouds and their references --------------------------------------------------------------------------------
def _scales(scheme):
    return (1.0, 255.0) if scheme == "rgb" else (1.0,)          # (ColorMSE's scale, and ColorHausdorffDistance's where it differs)


def _want(own, other, idx, scheme, scale):
    """-> (squared rows, np.add.reduce of them, np.max of them): the oracle's rows, NumPy's reductions."""
    with np.errstate(all="ignore"):
        sq, sums, maxs = orc.color_columns(own, other, idx, scheme, scale)
        want_sum, want_max = np.add.reduce(sq, axis=0), np.max(sq, axis=0)
        if scheme == "rgb":                                         # plain NumPy on the doubles says the same as the oracle
            mine = (scale * (own - np.take(other, idx, axis=0))) ** 2
            assert np.array_equal(mine, sq, equal_nan=True)
    assert same_bits(sums, want_sum) and same_bits(maxs, want_max)
    return sq, want_sum, want_max


class Pair:
    """Two clouds, the oracle's nearest rows both ways, and their colours (replaceable)."""

    def __init__(self, a, b, ca, cb):
        self.a, self.b, self.ca, self.cb = a, b, ca, cb
        self.idx = {LEFT: orc.nn(a, b)[0], RIGHT: orc.nn(b, a)[0]}

    def want(self, direction, scheme, scale, ca=None, cb=None):
        ca, cb = self.ca if ca is None else ca, self.cb if cb is None else cb
        own, other = (ca, cb) if direction == LEFT else (cb, ca)
        return _want(own, other, self.idx[direction], scheme, scale)

    def load(self, eng, colours=True):
        eng.set_cloud(0, self.a)
        eng.set_cloud(1, self.b)
        if colours:
            eng.set_colors(0, self.ca)
            eng.set_colors(1, self.cb)


def _check_reduce(eng, pair, what, ca=None, cb=None, directions=(LEFT, RIGHT)):
    """color_reduce of every scheme and scale against NumPy on the reference's rows: the first direction computes both, the second
    is answered from what the first left behind."""
    for scheme in SCHEMES:
        for scale in _scales(scheme):
            for d in directions:
                got_sum, got_max = eng.color_reduce(d, scheme, scale)
                _, want_sum, want_max = pair.want(d, scheme, scale, ca, cb)
                assert same_bits(got_sum, want_sum), (what, scheme, scale, d, _hex(got_sum), _hex(want_sum))
                assert same_bits(got_max, want_max), (what, scheme, scale, d, _hex(got_max), _hex(want_max))


# ---- B. both directions in one launch, unequal chunk counts -----------------------------------------------------------------------
WHITE, BLACK = (255, 255, 255), (0, 0, 0)
# own colour / neighbour's colour: the largest difference there is in R, G, B and Y | Cb, U | Cr, U | V
PLANTED = ((WHITE, BLACK), ((0, 0, 255), (255, 255, 0)), ((255, 0, 0), (0, 255, 255)), ((0, 255, 0), (255, 0, 255)))


@functools.lru_cache(maxsize=None)
def _unequal_pair(n, m):
    """Clouds of n and m points with byte colours in 10..245 -- except: four rows of the LONGER cloud's last (partial) chunk and
    their neighbours hold the pairs of PLANTED, and row 0 of the SHORTER cloud is white, its neighbour black."""
    a, _, ca, _ = _coloured(n, 1)
    _, b, _, cb = _coloured(m, 2)
    pair = Pair(a, b, None, None)
    col = [np.clip(np.rint(ca * 255), 10, 245), np.clip(np.rint(cb * 255), 10, 245)]
    long_ = 0 if n > m else 1
    d_long, d_short = (LEFT, RIGHT) if long_ == 0 else (RIGHT, LEFT)
    size = (n, m)[long_]
    first = (size - 1) // cp.CHUNK * cp.CHUNK                     # where the longer cloud's last chunk begins
    rows = np.arange(first, first + 4)
    partners = pair.idx[d_long][rows]
    back = int(pair.idx[d_short][0])
    assert rows[-1] < size and len(set(partners.tolist())) == 4 and 0 not in partners and back not in rows
    for r, j, (own, other) in zip(rows, partners, PLANTED):
        col[long_][r] = own
        col[1 - long_][j] = other
    col[1 - long_][0] = WHITE
    col[long_][back] = BLACK
    pair.ca, pair.cb = col[0] / 255.0, col[1] / 255.0
    return pair, d_long, d_short, first


@pytest.mark.parametrize("n,m", [(3 * 8192 + 5, 8192 - 3), (8192 - 3, 3 * 8192 + 5), (2 * 8192, 8192 + 1)])
def test_both_directions_of_unequal_chunk_counts_in_one_launch(engine, n, m):
    pair, d_long, d_short, first = _unequal_pair(n, m)
    # the maxima are where they were planted: by the reference's rows
    for scheme in SCHEMES:
        sq = pair.want(d_long, scheme, 1.0)[0]
        assert np.all(sq[first:].max(axis=0) == sq.max(axis=0)), scheme
        if scheme != "rgb":
            assert np.all(sq[first:, 1:].max(axis=0) > sq[:first, 1:].max(axis=0)), scheme      # the chroma maxima are nowhere else
        sq = pair.want(d_short, scheme, 1.0)[0]
        cols = slice(0, 3) if scheme == "rgb" else slice(0, 1)
        assert np.all(sq[0, cols] == sq[:, cols].max(axis=0)) and np.all(sq[0, cols] > 0.99), scheme
    pair.load(engine)
    engine.nn_pair()
    assert np.array_equal(engine.fetch_nn(LEFT, want_d2=False)[0], pair.idx[LEFT])
    assert np.array_equal(engine.fetch_nn(RIGHT, want_d2=False)[0], pair.idx[RIGHT])
    _check_reduce(engine, pair, "left first")                     # LEFT computes both, RIGHT comes from the memo
    _check_reduce(engine, pair, "right first", directions=(RIGHT, LEFT))
    # one direction alone, on an engine that has no result for the other: bit for bit the same
    fresh = nat.Engine(0)
    try:
        for d in (LEFT, RIGHT):
            pair.load(fresh)
            fresh.nn(d)
            for scheme in SCHEMES:
                for scale in _scales(scheme):
                    alone = fresh.color_reduce(d, scheme, scale)
                    engine.color_reduce(LEFT if d == RIGHT else RIGHT, scheme, scale)
                    both = engine.color_reduce(d, scheme, scale)          # from the memo of the call above
                    assert same_bits(alone[0], both[0]) and same_bits(alone[1], both[1]), (scheme, scale, d)
    finally:
        fresh.close()


# ---- C. the byte decision ---------------------------------------------------------------------------------------------------------
N_BYTES = 20011
BYTE_ROWS = (0, 255, 256, N_BYTES - 1)


@functools.lru_cache(maxsize=None)
def _byte_pair():
    a, b, ca, cb = _coloured(N_BYTES, 31)
    ca[list(BYTE_ROWS)] = np.array([17, 100, 254]) / 255.0        # (no 255 here: np.nextafter(1.0, 1) would change nothing)
    return Pair(a, b, ca, cb)


@pytest.fixture(scope="module")
def byte_engine():
    """An engine that holds _byte_pair()'s clouds, both searches and cloud 1's colours; the tests give cloud 0 its colours."""
    e = nat.Engine(0)
    pair = _byte_pair()
    pair.load(e, colours=False)
    e.nn_pair()
    e.set_colors(1, pair.cb)
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_byte_table_comes_back_as_it_went_in(byte_engine):
    pair = _byte_pair()
    byte_engine.set_colors(0, pair.ca)
    assert np.array_equal(_bits(byte_engine.color_rows(LEFT, "rgb", nat.COLOR_OWN)), _bits(pair.ca))
    assert np.array_equal(_bits(byte_engine.color_rows(RIGHT, "rgb", nat.COLOR_OWN)), _bits(pair.cb))
    assert np.array_equal(_bits(byte_engine.color_rows(LEFT, "rgb", nat.COLOR_NEIGHBOUR)), _bits(np.take(pair.cb, pair.idx[LEFT], axis=0)))
    _check_reduce(byte_engine, pair, "bytes")


OFF_BYTE = {
    "one ulp up": lambda v: np.nextafter(v, 1),
    "minus zero": lambda v: -0.0,
    "256/255": lambda v: 256 / 255.0,
    "-1/255": lambda v: -1 / 255.0,
    "nan": lambda v: np.nan,
}


@pytest.mark.parametrize("row", BYTE_ROWS)
@pytest.mark.parametrize("kind", list(OFF_BYTE))
def test_one_value_that_is_no_byte_quotient(byte_engine, kind, row):
    """One channel of one row is not k / 255.0: the cloud must be read as the doubles it holds -- the table comes back bit for bit
    (sign of zero included) and every sum and maximum is NumPy's on those doubles."""
    pair = _byte_pair()
    channel = BYTE_ROWS.index(row) % 3
    ca = pair.ca.copy()
    ca[row, channel] = OFF_BYTE[kind](ca[row, channel])
    assert _bits(ca)[row, channel] != _bits(pair.ca)[row, channel] and (_bits(ca) != _bits(pair.ca)).sum() == 1
    byte_engine.set_colors(0, ca)
    assert np.array_equal(_bits(byte_engine.color_rows(LEFT, "rgb", nat.COLOR_OWN)), _bits(ca)), (kind, row)
    back = byte_engine.color_rows(RIGHT, "rgb", nat.COLOR_NEIGHBOUR)
    assert np.array_equal(_bits(back), _bits(np.take(ca, pair.idx[RIGHT], axis=0))), (kind, row)
    _check_reduce(byte_engine, pair, (kind, row), ca=ca)
    byte_engine.set_colors(0, pair.ca)                            # ... and bytes again
    assert np.array_equal(_bits(byte_engine.color_rows(LEFT, "rgb", nat.COLOR_OWN)), _bits(pair.ca))
    _check_reduce(byte_engine, pair, (kind, row, "bytes again"), directions=(LEFT,))


@pytest.mark.parametrize("bytes_in", [0, 1])
def test_one_byte_cloud_beside_one_that_is_not(byte_engine, bytes_in):
    pair = _byte_pair()
    rng = np.random.default_rng(41 + bytes_in)
    n = (len(pair.a), len(pair.b))
    u8 = rng.integers(0, 256, (n[bytes_in], 3)).astype(np.uint8)
    other = rng.random((n[1 - bytes_in], 3))
    col = [None, None]
    col[bytes_in], col[1 - bytes_in] = u8 / 255.0, other
    try:
        byte_engine.set_colors_u8(bytes_in, u8)
        byte_engine.set_colors(1 - bytes_in, other)
        for d, which in ((LEFT, 0), (RIGHT, 1)):
            assert np.array_equal(_bits(byte_engine.color_rows(d, "rgb", nat.COLOR_OWN)), _bits(col[which]))
        _check_reduce(byte_engine, pair, ("mixed", bytes_in), ca=col[0], cb=col[1])
        _check_reduce(byte_engine, pair, ("mixed, right first", bytes_in), ca=col[0], cb=col[1], directions=(RIGHT, LEFT))
    finally:
        byte_engine.set_colors(1, pair.cb)


def test_a_cloud_that_changes_kind_between_calls():
    """bytes -> arbitrary doubles -> bytes on one engine, then a shorter and a longer cloud 0 of either kind: after every step the
    engine answers what a fresh engine answers (and what the reference says)."""
    rng = np.random.default_rng(51)
    base = _byte_pair()
    short = _coloured(9001, 52)[0]
    long_ = _coloured(26003, 53)[0]
    kept = nat.Engine(0)

    def step(what, a, ca, u8):
        pair = Pair(a, base.b, ca, base.cb)
        fresh = nat.Engine(0)
        try:
            pair.load(fresh, colours=False)
            fresh.set_colors(1, base.cb)
            fresh.nn_pair()
            if what == "start":
                pair.load(kept, colours=False)
                kept.set_colors(1, base.cb)
                kept.nn_pair()
            elif len(a) != kept.n_iter(LEFT):                     # a new cloud 0: its colours go with the old one, cloud 1 keeps its own
                kept.set_cloud(0, a)
                kept.nn_pair()
            for eng in (kept, fresh):
                if u8:
                    eng.set_colors_u8(0, np.rint(ca * 255).astype(np.uint8))
                else:
                    eng.set_colors(0, ca)
            _check_reduce(kept, pair, what)
            for scheme in SCHEMES:
                for d in (LEFT, RIGHT):
                    got, want = kept.color_reduce(d, scheme), fresh.color_reduce(d, scheme)
                    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (what, scheme, d)
            assert np.array_equal(_bits(kept.color_rows(LEFT, "ycc", nat.COLOR_DIFF)), _bits(fresh.color_rows(LEFT, "ycc", nat.COLOR_DIFF))), what
            assert np.array_equal(_bits(kept.color_rows(LEFT, "rgb", nat.COLOR_OWN)), _bits(ca)), what
            assert np.array_equal(_bits(kept.color_rows(RIGHT, "rgb", nat.COLOR_OWN)), _bits(base.cb)), what
        finally:
            fresh.close()

    def bytes_(n):
        return rng.integers(0, 256, (n, 3)) / 255.0

    try:
        step("start", base.a, base.ca, False)
        step("arbitrary", base.a, rng.random((N_BYTES, 3)), False)
        step("bytes again", base.a, bytes_(N_BYTES), False)
        step("shorter, arbitrary", short, rng.random((len(short), 3)), False)
        step("longer, bytes", long_, bytes_(len(long_)), False)
        step("shorter, uchar", short, bytes_(len(short)), True)
        step("longer, arbitrary", long_, rng.random((len(long_), 3)), False)
    finally:
        kept.close()


# ---- D. non-finite colours through the reduce -------------------------------------------------------------------------------------
def _non_finite(kind, pair):
    """-> (ca, cb, the rgb columns NumPy's LEFT sums must be NaN in)."""
    ca, cb = pair.ca.copy(), pair.cb.copy()
    if kind == "nan in the iterating cloud":
        ca[4321, 1] = np.nan
        return ca, cb, [1]
    if kind == "nan in a neighbour":
        j = int(pair.idx[LEFT][1234])                             # a searched row that IS somebody's neighbour
        cb[j, 2] = np.nan
        return ca, cb, [2]
    if kind == "inf on both sides":
        i = 777
        ca[i, 0] = np.inf
        cb[int(pair.idx[LEFT][i]), 0] = np.inf                    # inf - inf
        return ca, cb, [0]
    if kind == "inf on one side":
        ca[N_BYTES - 2, 2] = np.inf
        return ca, cb, []
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["nan in the iterating cloud", "nan in a neighbour", "inf on both sides", "inf on one side"])
def test_non_finite_colours_propagate_like_numpy(byte_engine, kind):
    pair = _byte_pair()
    ca, cb, nan_cols = _non_finite(kind, pair)
    # what the reference says, per scheme: in "rgb" the NaN stays in its column, the matrices of "ycc" and "yuv" spread it
    _, s_rgb, m_rgb = pair.want(LEFT, "rgb", 1.0, ca, cb)
    assert np.flatnonzero(np.isnan(s_rgb)).tolist() == nan_cols and np.flatnonzero(np.isnan(m_rgb)).tolist() == nan_cols
    if kind == "inf on one side":
        assert s_rgb[2] == np.inf and m_rgb[2] == np.inf and np.all(np.isfinite(s_rgb[:2]))
    for scheme in ("ycc", "yuv"):
        _, s, m = pair.want(LEFT, scheme, 1.0, ca, cb)
        assert not np.any(np.isfinite(s)) and not np.any(np.isfinite(m))
        assert np.all(np.isnan(s)) or kind == "inf on one side"
    try:
        byte_engine.set_colors(0, ca)
        byte_engine.set_colors(1, cb)
        _check_reduce(byte_engine, pair, kind, ca=ca, cb=cb)
        _check_reduce(byte_engine, pair, (kind, "right first"), ca=ca, cb=cb, directions=(RIGHT, LEFT))
    finally:
        byte_engine.set_colors(1, pair.cb)
