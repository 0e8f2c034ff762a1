"""Planted cases for the brute-force engine (k1_scan / k2_refine / k2b_fallback, open_pcc_metric_amd/csrc/pccm_brute.hip, and rescan_body,
pccm_rescan.h), each with a host model of what the engine's certificate must decide and a proof -- on the host, about the DATA --
that the case has the property its family claims.  NumPy only; the truth comes from oracle/ (kd-tree) and, for the small cases,
from an fp64 brute force in the reference's expression ((dx*dx)+(dy*dy))+(dz*dz), smallest row on ties.

The model, written from the kernel source:

  dist32    dx = qx - rx (one fp32 rounding each), d = dx*dx, d = fma(dy, dy, d), d = fma(dz, dz, d).  The square of an fp32 number
            is exact in fp64 (48 bits), and TwoSum gives p + d = s + e EXACTLY as an unevaluated pair of fp64 numbers; that exact
            sum is rounded ONCE to fp32 (s is moved to the odd neighbour on e's side first, which is what makes the last
            conversion a single rounding of s + e: Boldo & Melquiond, 53 >= 2 * 24 + 2).  tests/test_brute_planted_host.py pins it
            on 1e5 random triples against fractions.Fraction, and shows that the naive float32(float64(dy) * dy + d) is NOT it.
  padding   rows n .. n_pad - 1 (n_pad: the next multiple of 1024) sit at kPadCoord = 1e18f in every coordinate.
  granules  per query the minimum of dist32 over each 64 rows (SELF: the query's own row counts as kBig32); b1 is the smallest
            granule minimum, b2 the second smallest of that multiset, g1 the earliest granule that holds b1 (k1_scan and the merge
            in k2_refine improve on `<` only).  Min and second-min of a multiset do not depend on how the tiles are split over
            workgroups, so one model serves every launch shape.
  thr       slack = (both clouds survive fp64 -> fp32 -> fp64 ? 0 : 2^-20) * (|q|_inf + sqrt(b1)),
            thr = (sqrt(b1) * (1 + 2^-20) + slack)^2 * (1 + 2^-30) + 1e-36, all in fp64; a query is FLAGGED (goes to the exact
            rescan) when not (b2 > thr), else its answer is taken from granule g1.

The device evaluates thr with its own sqrt and multiplies, so a case whose flagged COUNT is asserted must keep every b2 / thr
outside [1 - 2^-40, 1 + 2^-40] and every granule minimum out of the fp32 subnormal range (band_violations()): the host test
rejects a case that breaks either rule, it does not skip the query.

Families (G = 64 rows a granule, T = 1024 a tile, W = 2048 queries a scan workgroup; n = 3T + 5 = 3077 unless stated):
  R  reversal: 256 isolated triples (q, r_near, r_far) per magnitude whose modelled fp32 order is the reverse of the fp64 order
     (every eighth: an fp32 tie), r_far in an earlier granule -- the certificate MUST flag all of them;
  C  certified: winner and runner-up 2^-12 apart in radius at the rows where granule, tile, split and padding meet -- count 0;
  T  exact ties on an integer lattice, across granules, tiles, splits, rescan slices and rescan threads -- count = tie queries;
  S  a cloud against itself: neighbours in another granule, duplicates at smaller and larger rows, 130 identical points;
  L  a 300 x 500 uniform pair scaled down until the fp32 distances go subnormal and to 0 -- results only.
"""
import functools
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

G, T, W = 64, 1024, 2048                       # kGranule, kScanTile, kScanThreads * QT (QT = 8)
PAD = np.float32(1.0e18)                       # kPadCoord
BIG = np.float32(3.0e38)                       # kBig32
SPLIT_MAX, RESCAN_CAP = 32, 512                # kSplitMax, kRescanCap
N0 = 3 * T + 5
TINY32 = float(np.finfo(np.float32).tiny)      # 2^-126
BAND = 2.0 ** -40


# ---- fp32 arithmetic of the scan -------------------------------------------------------------------------------------------------
def fma_sq_add32(y, d):
    """fma(y, y, d) of fp32 arrays y and d >= 0, rounded once."""
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    d = np.asarray(d, dtype=np.float32).astype(np.float64)
    p = y * y                                           # exact: 24 x 24 bits, exponents far inside fp64's
    s = p + d
    bb = s - p
    e = (p - (s - bb)) + (d - bb)                       # TwoSum: p + d == s + e exactly
    bits = np.ascontiguousarray(s).view(np.int64)
    step = np.where(e > 0, 1, -1).astype(np.int64)      # s >= 0: the next fp64 number up / down
    bits = np.where((e != 0) & ((bits & 1) == 0), bits + step, bits)
    return bits.view(np.float64).astype(np.float32)


def sq_sum32(dx, dy, dz):
    """The scan's accumulation of three fp32 differences: dx*dx, then fma(dy, dy, .), then fma(dz, dz, .)."""
    dx = np.asarray(dx, dtype=np.float32)
    return fma_sq_add32(dz, fma_sq_add32(dy, dx * dx))


def dist32(q, r):
    """dist32() of pccm_rescan.h for fp32 arrays q[..., 3] and r[..., 3] (broadcast)."""
    q, r = np.asarray(q, dtype=np.float32), np.asarray(r, dtype=np.float32)
    return sq_sum32(q[..., 0] - r[..., 0], q[..., 1] - r[..., 1], q[..., 2] - r[..., 2])


def round32_fraction(v):
    """The fp32 number nearest to the Fraction v >= 0, ties to even, subnormals included (as a Fraction)."""
    if v == 0:
        return Fraction(0)
    num, den = v.numerator, v.denominator
    e = num.bit_length() - den.bit_length()
    if (num < den << e) if e >= 0 else (num << -e < den):
        e -= 1                                          # 2^e <= v < 2^(e+1)
    ue = max(e - 23, -149)                              # the unit in the last place
    n, rem = divmod(num << -ue, den) if ue < 0 else divmod(num, den << ue)
    half = den if ue < 0 else den << ue
    if 2 * rem > half or (2 * rem == half and n % 2 == 1):
        n += 1
    return Fraction(n, 1 << -ue) if ue < 0 else Fraction(n << ue)


def sq_sum32_fraction(dx, dy, dz):
    """sq_sum32 of three fp32 numbers in exact rational arithmetic, one rounding per operation."""
    x, y, z = Fraction(float(dx)), Fraction(float(dy)), Fraction(float(dz))
    d = round32_fraction(x * x)
    d = round32_fraction(y * y + d)
    return float(round32_fraction(z * z + d))


# ---- the model -------------------------------------------------------------------------------------------------------------------
def is_exact32(a):
    a = np.asarray(a, dtype=np.float64)
    return bool(np.all(a.astype(np.float32).astype(np.float64) == a))


def padded32(r):
    r = np.asarray(r, dtype=np.float64)
    n_pad = -(-len(r) // T) * T
    out = np.full((n_pad, 3), PAD, dtype=np.float32)
    out[:len(r)] = r.astype(np.float32)
    return out


def scan_model(queries, searched, self_search=False):
    """What k1_scan leaves and k2_refine decides for every query -> b1, b2 (fp32), g1, thr (fp64), flag, subnormal (any granule
    minimum of that query in the fp32 subnormal range)."""
    q64 = np.asarray(queries, dtype=np.float64)
    exact = is_exact32(q64) and is_exact32(searched)
    q32, r32 = q64.astype(np.float32), padded32(searched)
    nq, ng = len(q64), len(r32) // G
    b1, b2 = np.empty(nq, np.float32), np.empty(nq, np.float32)
    g1, sub = np.empty(nq, np.int64), np.zeros(nq, bool)
    step = max(1, (1 << 21) // len(r32))
    for lo in range(0, nq, step):
        hi = min(nq, lo + step)
        d = dist32(q32[lo:hi, None, :], r32[None, :, :])
        if self_search:
            d[np.arange(hi - lo), np.arange(lo, hi)] = BIG
        gm = d.reshape(hi - lo, ng, G).min(axis=2)
        sub[lo:hi] = np.any((gm > 0) & (gm < TINY32), axis=1)
        g1[lo:hi] = gm.argmin(axis=1)                   # the first of equal minima
        two = np.partition(gm, 1, axis=1)
        b1[lo:hi], b2[lo:hi] = two[:, 0], two[:, 1]
    rb1 = np.sqrt(b1.astype(np.float64))
    slack = (0.0 if exact else 2.0 ** -20) * (np.abs(q64).max(axis=1) + rb1)
    tq = rb1 * (1.0 + 2.0 ** -20) + slack
    thr = tq * tq * (1.0 + 2.0 ** -30) + 1.0e-36
    flag = ~(b2.astype(np.float64) > thr)
    return SimpleNamespace(b1=b1, b2=b2, g1=g1, thr=thr, flag=flag, subnormal=sub, exact=exact)


def band_violations(m):
    """Queries whose flag the device's own rounding of thr could turn, or whose granule minima depend on how it treats subnormals."""
    ratio = m.b2.astype(np.float64) / m.thr
    return np.flatnonzero((np.abs(ratio - 1.0) <= BAND) | m.subnormal)


def unsound(m, truth_rows):
    """Queries the model certifies although the truth lies outside the winner granule (must be empty for the shipped formula)."""
    return np.flatnonzero(~m.flag & (m.g1 != np.asarray(truth_rows) // G))


def splits_for(nq, n):
    """nn_brute's launch rule -> (splits, tiles per split)."""
    qblocks, ntiles = -(-nq // W), -(-n // T)
    s = max(1, min(-(-6144 // qblocks), ntiles, 64))
    tps = -(-ntiles // s)
    return -(-ntiles // tps), tps


def rescan_plan(nq, n, flagged):
    """launch_fallback / rescan_body -> (regime, workgroups, rows per slice in the split regime)."""
    nb = min(max(nq, 1), RESCAN_CAP)
    regime = "none" if flagged == 0 else ("split" if flagged <= SPLIT_MAX else "list")
    return regime, nb, -(-n // nb)


def shard_of(n, rank, world):
    """pccm_api.hip's shard_of for world > 0."""
    unit = 8192 if n >= world * 8192 else 128
    units = -(-n // unit)
    return min(units * rank // world * unit, n), min(units * (rank + 1) // world * unit, n)


# ---- truth -----------------------------------------------------------------------------------------------------------------------
def brute64(queries, searched, self_search=False):
    """fp64 brute force in the reference's expression, smallest row on ties -> (rows, d2)."""
    q, r = np.asarray(queries, dtype=np.float64), np.asarray(searched, dtype=np.float64)
    rows, d2 = np.empty(len(q), np.int64), np.empty(len(q))
    step = max(1, (1 << 21) // len(r))
    for lo in range(0, len(q), step):
        hi = min(len(q), lo + step)
        dx, dy, dz = (q[lo:hi, None, a] - r[None, :, a] for a in range(3))
        d = ((dx * dx) + (dy * dy)) + (dz * dz)
        if self_search:
            d[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
        rows[lo:hi] = d.argmin(axis=1)
        d2[lo:hi] = d[np.arange(hi - lo), rows[lo:hi]]
    return rows, d2


def truth(case):
    """oracle.nn(method="kdtree") of a case, computed once per case object."""
    if case.truth is None:
        from oracle import oracle as orc
        rows, d2 = orc.nn(case.queries, case.searched, skip_same_index=case.self_search, method="kdtree")
        case.truth = (rows.astype(np.int64), d2)
    return case.truth


def model(case):
    if case.model is None:
        case.model = scan_model(case.queries, case.searched, case.self_search)
    return case.model


def converse(c):
    """The search the other way round (direction 1): the searched cloud's rows look for their neighbours among the queries."""
    r = make_case(c.name + "_rev", c.searched, c.queries)
    r.direction = 1
    return r


def make_case(name, queries, searched, self_search=False, **meta):
    q = np.ascontiguousarray(queries, dtype=np.float64)
    r = q if self_search else np.ascontiguousarray(searched, dtype=np.float64)
    return SimpleNamespace(name=name, queries=q, searched=r, self_search=self_search, direction=2 if self_search else 0,
                           truth=None, model=None, **meta)


def _sites(dims, spacing, origin):
    """Centres of a coarse lattice, as an (prod(dims), 3) array in C order."""
    ax = [origin + spacing * (np.arange(d) - d // 2) for d in dims]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)


# ---- R: reversals ----------------------------------------------------------------------------------------------------------------
# kind: which cloud is fp32-exact ("exact": both, slack 0; "fp64": neither; "q_exact" / "r_exact": the queries / the searched cloud only)
R_CASES = {
    "R_exact_0": ("exact", 0.0), "R_exact_1e3": ("exact", 1.0e3),
    "R_fp64_0": ("fp64", 0.0), "R_fp64_1e3": ("fp64", 1.0e3), "R_fp64_4e6": ("fp64", 4.0e6), "R_fp64_1e9": ("fp64", 1.0e9),
    "R_fp64_9e14": ("fp64", 9.0e14),
    "R_q_exact_1e6": ("q_exact", 1.0e6), "R_r_exact_1e6": ("r_exact", 1.0e6),
}
R_TRIPLES = 256


def R_NEAR_ROW(k):
    return 300 + 10 * k                        # rows 300 .. 2850: granules 4 .. 44 of tiles 0, 1 and 2


def R_FAR_ROW(k):
    return k                                   # rows 0 .. 255: granules 0 .. 3


def _r32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def family_r(name):
    """256 queries on a lattice of spacing 16 rho, each with a near and a far point at radius ~rho whose modelled fp32 distances are
    in the wrong order (every eighth triple: equal, where the search finds such a pair); every other searched point sits on another
    lattice site, more than 4 rho away.  rho = max(1, offset * 2^-18), so that the fp32 rounding of inexact coordinates
    (<= offset * 2^-24) is a visible fraction of the radius at every magnitude."""
    kind, off = R_CASES[name]
    rng = np.random.default_rng([82, sorted(R_CASES).index(name)])
    rho = 1.0 if kind == "exact" else max(1.0, off * 2.0 ** -18)
    sites = _sites((16, 16, 16), 16.0 * rho, off)
    order = rng.permutation(len(sites))
    width = 2.0 ** -20 if kind == "exact" else min(2.0 ** -8, max(2.0 ** -20, 2.0 ** -22 * off / rho))
    q_round = kind in ("exact", "q_exact")
    r_round = kind in ("exact", "r_exact")
    queries = np.empty((R_TRIPLES, 3))
    searched = np.empty((N0, 3))
    fill_rows = sorted(set(range(N0)) - {R_NEAR_ROW(k) for k in range(R_TRIPLES)} - {R_FAR_ROW(k) for k in range(R_TRIPLES)})
    fill = sites[order[R_TRIPLES:R_TRIPLES + len(fill_rows)]] + rng.uniform(-0.5, 0.5, (len(fill_rows), 3)) * rho
    searched[fill_rows] = _r32(fill) if r_round else fill
    ties = 0
    for k in range(R_TRIPLES):
        for attempt in range(64):
            q = sites[order[k]] + rng.uniform(-0.5, 0.5, 3) * rho
            q = _r32(q) if q_round else q
            u = rng.normal(size=(4096, 3))
            u /= np.linalg.norm(u, axis=1)[:, None]
            cand = q + rho * (1.0 + rng.uniform(0.0, width, (4096, 1))) * u
            cand = _r32(cand) if r_round else cand
            d64 = brute_d64(q, cand)
            d32 = dist32(q.astype(np.float32), cand.astype(np.float32)).astype(np.float64)
            o = np.argsort(d64, kind="stable")
            d64, d32, cand = d64[o], d32[o], cand[o]
            # for every i the candidate j with d64[j] > d64[i] and the smallest fp32 distance
            later = np.searchsorted(d64, d64, side="right")
            sufmin = np.minimum.accumulate(d32[::-1])[::-1]
            rev = d32[::-1]                                      # sufarg[j]: the smallest index >= j that holds sufmin[j]
            hit = np.where(rev <= np.minimum.accumulate(rev), np.arange(len(rev)), 0)
            sufarg = (len(rev) - 1 - np.maximum.accumulate(hit))[::-1]
            ok = later < len(d32)
            lm = np.where(ok, sufmin[np.minimum(later, len(d32) - 1)], np.inf)
            if k % 8 == 7 and np.any(ok & (lm == d32)):
                i = int(np.flatnonzero(ok & (lm == d32))[0])
            else:
                gain = np.where(ok & (lm < d32), d32 / np.where(lm > 0, lm, 1.0), 0.0)
                if not gain.max() > 1.0:
                    continue
                i = int(gain.argmax())
            j = int(sufarg[later[i]])
            ties += int(d32[i] == d32[j])
            queries[k], searched[R_NEAR_ROW(k)], searched[R_FAR_ROW(k)] = q, cand[i], cand[j]
            break
        else:
            raise AssertionError(f"{name}: no reversal found for triple {k}")
    return make_case(name, queries, searched, kind=kind, offset=off, rho=rho, fp32_ties=ties)


def brute_d64(q, pts):
    d = np.asarray(q, dtype=np.float64) - np.asarray(pts, dtype=np.float64)
    return ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])


# ---- C: certified pairs at the seams ----------------------------------------------------------------------------------------------
C_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, N0)
C_BIG = 65 * T + 5
C_A, C_H, C_DELTA = 0.75, 0.75, 3.0 * 2.0 ** -14      # the two radii differ by ~2^-12: 4 a delta / (a^2 + h^2) = 2^-11 * 1.0001


def c_pairs(n):
    """Row pairs (low, high) planted in a cloud of n rows: across every granule / tile / workgroup seam below n, across the first row
    of the last split of the 66 565-row cloud, and row 0 with the last row that is still free (n - 1 unless a seam pair holds it)."""
    pairs = [(k - 1, k) for k in (G, T, W, 64 * T) if k < n]
    used = {r for p in pairs for r in p}
    if n >= 2:
        if n - 1 not in used:
            hi = n - 1
        else:
            hi = max(r for r in range(n) if r not in used and r != 0)
        pairs.append((0, hi))
    return pairs


def family_c(n):
    """Per planted pair two mirror-image queries: for one the low row wins and the high row is the runner-up 2^-12 farther out, for
    the other the reverse.  All inputs are fp32-exact dyadic numbers (slack 0); every other point is a lattice site >= 14 away."""
    pairs = c_pairs(n)
    side = 2
    while side ** 3 < n + len(pairs):
        side += 1
    sites = _sites((side, side, side), 16.0, 8.0 * side)
    searched = np.empty((n, 3))
    queries, want = [], []
    planted = {}
    for k, (lo, hi) in enumerate(pairs):
        c = sites[k]
        planted[lo], planted[hi] = c + (-C_A, 0, 0), c + (C_A, 0, 0)
        queries += [c + (-C_DELTA, C_H, 0), c + (C_DELTA, C_H, 0)]
        want += [lo, hi]
    free = iter(sites[len(pairs):])
    for row in range(n):
        searched[row] = planted[row] if row in planted else next(free)
    if not pairs:                                       # n = 1: one point, one query
        queries, want = [searched[0] + (C_DELTA, C_H, 0)], [0]
    return make_case(f"C_{n}", np.array(queries), searched, pairs=pairs, want_rows=np.array(want))


# ---- T: exact ties ---------------------------------------------------------------------------------------------------------------
# (points of the cluster as offsets from its site, row offsets from the cluster's first row, the query's offset)
_A, _B, _C = (0, 0, 0), (1, 0, 0), (0, 1, 0)
T_PATTERNS = (
    ((_A, _B), (0, 64), (0.5, 0, 0)),                  # next granule
    ((_A, _B), (0, 1024), (0.5, 0, 0)),                # next tile = next split
    ((_A, _A, _B), (0, 1, 2048), (0.5, 0, 0)),         # duplicates at r, r + 1: neighbouring rescan threads
    ((_A, _A, _B), (0, 64, 300), (0.5, 0, 0)),         # duplicates at r, r + 64: the next wave of the rescan workgroup
    ((_A, _A), (0, 256), (0.5, 0, 0)),                 # duplicates at r, r + 256: the SAME rescan thread, one stride on
    ((_A, _A, _B), (0, 1024, 2), (0.5, 0, 0)),         # duplicates a tile apart
    ((_A, _B, _C), (0, 1100, 2200), (0.5, 0.5, 0)),    # three distinct points in three tiles
    ((_B, _A), (0, 256), (0.5, 0, 0)),                 # two distinct points in one thread's stride
    ((_A, _B), (0, 256 * 7), (0.5, 0, 0)),             # 512 rescan workgroups, slices of 7 rows: 256 slices apart, ONE thread of the fold
)
T_INSIDE = (((_A, _A), (0, 1)), ((_A, _B), (0, 3)))   # ties inside ONE granule: certified, settled by k2_refine's lowest lane
T_TIES, T_INSIDE_N = 600, 8
T_CASES = {                                            # name -> (tie queries, other queries, first tie cluster taken)
    "T_k0": (0, 50, 0), "T_k1_alone": (1, 0, 0), "T_k32": (32, 68, 0), "T_k33": (33, 67, 0), "T_k600": (600, 100, 0),
    "T_k32_b": (32, 68, 304),                          # other clusters: no answer of T_k32 or T_k33 is an answer here
    "T_k32_wide": (32, 568, 0),                        # 600 queries: the split regime on 512 workgroups, every slice holds rows
}


@functools.lru_cache(maxsize=None)
def _t_cloud():
    rng = np.random.default_rng(84)
    sites = _sites((16, 16, 12), 4.0, 32.0)
    site = iter(sites[rng.permutation(len(sites))])
    free = np.ones(N0, bool)
    searched = np.full((N0, 3), np.nan)
    ties = []                                           # (query, tied rows ascending, d2)

    def place(points, offs, query, start, same_granule=False):
        for r in range(start, N0):
            rows = [r + o for o in offs]
            if max(rows) < N0 and all(free[x] for x in rows) and (not same_granule or len({x // G for x in rows}) == 1):
                c = next(site)
                for x, p in zip(rows, points):
                    searched[x], free[x] = c + p, False
                qq = c + query
                d2 = float(brute_d64(qq, searched[rows[0]]))
                ties.append((qq, sorted(rows), d2))
                return
        raise AssertionError("no room for a tie cluster")

    for k in range(T_TIES):
        pts, offs, query = T_PATTERNS[k % len(T_PATTERNS)]
        place(pts, offs, query, start=(37 * k) % (N0 - max(offs) - 200))
    inside = []
    for k in range(T_INSIDE_N):
        pts, offs = T_INSIDE[k % 2]
        place(pts, offs, (0.5, 0, 0), start=2100 + 70 * k, same_granule=True)
        inside.append(ties.pop())
    rest = np.flatnonzero(free)
    for x in rest:
        searched[x] = next(site)
    return searched, ties, inside, rest


def family_t(name):
    """Tie queries at half-integer midpoints first (each equidistant from the 2 or 3 points of its cluster, in different granules),
    then the in-granule ties, then queries that sit on an isolated searched point (d2 = 0, b2 >= 9)."""
    k, others, first = T_CASES[name]
    searched, ties, inside, rest = _t_cloud()
    tq = ties[first:first + k]
    ins = inside if others else []
    on = rest[np.arange(max(0, others - len(ins))) * 7 % len(rest)] if others else np.zeros(0, np.int64)
    queries = np.array([t[0] for t in tq] + [t[0] for t in ins] + [searched[x] for x in on]).reshape(-1, 3)
    want_rows = np.array([t[1][0] for t in tq] + [t[1][0] for t in ins] + list(on), dtype=np.int64)
    want_d2 = np.array([t[2] for t in tq] + [t[2] for t in ins] + [0.0] * len(on))
    return make_case(name, queries, searched, want_rows=want_rows, want_d2=want_d2, tie_queries=k,
                     tied_rows=[t[1] for t in tq])


def family_t_small(n):
    """600 queries against a cloud of n rows with 512 rescan workgroups.  n = 66: rows 0, 64 and 65 are (0,0,0), (1,0,0), (1,0,0),
    rows 1 .. 63 far away; 32 queries at (0.5, y, 0) tie across the two granules and the 512 slices hold one row or none.
    n = 3: the same three points -- one granule, so b2 is the padding's distance and NO query can be flagged (count 0)."""
    far = np.array([[40.0 + 4 * i, 40.0, 40.0] for i in range(63)])
    trio = np.array([[0.0, 0, 0], [1, 0, 0], [1, 0, 0]])
    searched = trio if n == 3 else np.vstack([trio[:1], far, trio[1:]])
    second = 1 if n == 3 else 64
    tq = np.array([[0.5, y / 8.0, 0.0] for y in range(32)])
    on_rows = np.array([(0, second, 5 % n, n - 1)[i % 4] for i in range(568)])
    queries = np.vstack([tq, searched[on_rows]])
    on_want = np.where(on_rows == n - 1, second, on_rows)          # the duplicate of the last row answers with the smaller row
    want_rows = np.concatenate([np.zeros(32, np.int64), on_want])
    want_d2 = np.concatenate([0.25 + (np.arange(32) / 8.0) ** 2, np.zeros(568)])
    return make_case(f"T_n{n}", queries, searched, want_rows=want_rows, want_d2=want_d2, tie_queries=32 if n > G else 0,
                     tied_rows=[[0, 64, 65]] * (32 if n > G else 0))


# ---- S: a cloud against itself ----------------------------------------------------------------------------------------------------
S_SIZES = (2, 3, 65, 1025, 2049, 4100)
S_STEPS = (64, 128, 1024, 2048, 192, 1)               # a pair sits at rows i and i + step: other granule, tile, scan workgroup


def family_s(n):
    """Clusters on a lattice of spacing 8, integer coordinates.  Pairs P, P + (1,0,0) at rows i and i + 64k (each the other's
    neighbour, d2 = 1); every fifth cluster a triple of identical points (d2 = 0: rows b and c answer a, row a answers b); rows
    2047 | 2048 and W - 48 | W + 16 pair across the edge of the first scan workgroup's own rows.  n = 3: two identical points and
    P + (1,0,0), whose two neighbours tie inside one granule."""
    side = 2
    while side ** 3 < n:
        side += 1
    site = iter(_sites((side, side, side), 8.0, 4.0 * side))
    pts = np.full((n, 3), np.nan)
    free = np.ones(n, bool)
    want = np.full(n, -1, np.int64)
    want_d2 = np.zeros(n)

    def put(rows, kind):
        c = next(site)
        for x in rows:
            free[x] = False
        if kind == "pair":
            a, b = rows
            pts[a], pts[b] = c, c + _B
            want[a], want[b], want_d2[a], want_d2[b] = b, a, 1.0, 1.0
        else:                                           # identical points: the smallest OTHER row
            for x in rows:
                pts[x] = c
                want[x] = rows[0] if x != rows[0] else rows[1]

    if n == 3:
        c = next(site)
        pts[:] = [c, c, c + _B]
        return make_case("S_3", pts, None, True, want_rows=np.array([1, 0, 0]), want_d2=np.array([0.0, 0.0, 1.0]))
    for a, b in ((W - 1, W), (W - 48, W + 16)):
        if b < n:
            put((a, b), "pair")
    k = 0
    for i in range(n):
        if not free[i]:
            continue
        k += 1
        placed = False
        for step in (S_STEPS[k % len(S_STEPS)],) + S_STEPS:
            rows = (i, i + step, i + 2 * step) if k % 5 == 0 else (i, i + step)
            if rows[-1] < n and all(free[x] for x in rows):
                put(rows, "same" if len(rows) == 3 else "pair")
                placed = True
                break
        if not placed:                                  # the last free rows: pair with the next free one, or join row 0's cluster
            later = np.flatnonzero(free[i + 1:])
            if len(later):
                put((i, i + 1 + int(later[0])), "pair")
            else:
                free[i] = False
                pts[i] = pts[0] + _C                    # a third point beside the pair at row 0: P + (0,1,0), d2 = 1 to P
                want[i], want_d2[i] = 0, 1.0
                want[0] = min(want[0], i)               # row 0's own neighbours now tie at d2 = 1: smallest row
    return make_case(f"S_{n}", pts, None, True, want_rows=want, want_d2=want_d2)


def family_s_identical(n=130):
    pts = np.tile(np.array([[3.0, -2.0, 7.0]]), (n, 1))
    want = np.zeros(n, np.int64)
    want[0] = 1
    return make_case(f"S_identical_{n}", pts, None, True, want_rows=want, want_d2=np.zeros(n))


# ---- L: the scale ladder ----------------------------------------------------------------------------------------------------------
L_SCALES = (1e-12, 1e-15, 1e-17, 1e-18, 1e-19, 1e-20, 1e-21, 1e-23, 1e-30)


def family_l(scale, rounded):
    rng = np.random.default_rng(76)
    q, r = rng.uniform(0.1, 1.0, (300, 3)) * scale, rng.uniform(0.1, 1.0, (500, 3)) * scale
    if rounded:
        q, r = _r32(q), _r32(r)
    return make_case(f"L_{scale:g}_{'fp32' if rounded else 'fp64'}", q, r, scale=scale, rounded=rounded)


# ---- every case whose flagged count is asserted -----------------------------------------------------------------------------------
_CACHE = {}


def case(name):
    """Cases by name, built once per process (the GPU tests and the host proofs share them)."""
    if name not in _CACHE:
        if name.endswith("_rev"):
            c = converse(case(name[:-4]))
        elif name in R_CASES:
            c = family_r(name)
        elif name in T_CASES:
            c = family_t(name)
        elif name.startswith("T_n"):
            c = family_t_small(int(name[3:]))
        elif name.startswith("C_"):
            c = family_c(int(name[2:]))
        elif name.startswith("S_identical"):
            c = family_s_identical()
        elif name.startswith("S_"):
            c = family_s(int(name[2:]))
        else:
            raise KeyError(name)
        _CACHE[name] = c
    return _CACHE[name]


C_NAMES = tuple(f"C_{n}" for n in C_SIZES + (C_BIG,))
T_NAMES = tuple(T_CASES) + ("T_n66", "T_n3")
S_NAMES = tuple(f"S_{n}" for n in S_SIZES) + ("S_identical_130",)
REV_NAMES = ("R_q_exact_1e6_rev", "R_r_exact_1e6_rev", "R_exact_1e3_rev", "T_k600_rev", f"C_{N0}_rev")
COUNTED = tuple(R_CASES) + C_NAMES + T_NAMES + S_NAMES + REV_NAMES


def predicted_flagged(c):
    """The modelled flagged count of a case; refuses a case inside the band."""
    m = model(c)
    bad = band_violations(m)
    assert len(bad) == 0, f"{c.name}: queries {bad[:8].tolist()} lie in the band where the device's rounding of thr decides"
    return int(m.flag.sum())
