"""What leaves a reduction slot, on the real kernels (open_pcc_metric_amd/csrc/pccm_slot.h; tests/test_slot_host.py is the same
without a GPU): the per-chunk and per-leaf exchange vectors of shards emulated one after the other on one context, summed over
the ranks and finished on the host, and the totals and selections of a captured graph replayed onto slots it finds pending and
idle.  28673 rows = 3 chunks of 8192 + a partial chunk longer than half a chunk: two ranks get whole chunks, four get leaves.
Sums are held to np.sum of the oracle's column bit for bit."""
import numpy as np
import pytest

import chamfer_reference
from open_pcc_metric_amd import _native as nat
from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu

N = 28673
L, R, D1, D2 = nat.DIR_LEFT, nat.DIR_RIGHT, nat.METRIC_D1, nat.METRIC_D2
REQ = [(L, D1), (R, D1), (L, D2), (R, D2)]


def _bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


@pytest.fixture(scope="module")
def pair():
    """the clouds, their normals, and the oracle's four columns (computed once, never written to)"""
    rng = np.random.default_rng(28673)
    pts = [rng.random((N, 3), dtype=np.float32).astype(np.float64) for _ in range(2)]
    nrm = [rng.standard_normal((N, 3), dtype=np.float32).astype(np.float64) for _ in range(2)]
    ref = OracleEngine(method="kdtree")
    for k in range(2):
        ref.set_cloud(k, pts[k])
        ref.set_normals(k, nrm[k])
    ref.nn(L)
    ref.nn(R)
    cols = {req: ref.point_metric(*req) for req in REQ}
    for c in cols.values():
        c.setflags(write=False)
    return pts, nrm, cols


def _engine(pts, nrm):
    eng = nat.Engine(0)
    for k in range(2):
        eng.set_cloud(k, pts[k])
        eng.set_normals(k, nrm[k])
    return eng


@pytest.mark.parametrize("world", [2, 4])
def test_emulated_shards_add_up_to_numpy(pair, world):
    pts, nrm, cols = pair
    eng = _engine(pts, nrm)
    try:
        xsum = {req: np.zeros(nat.xvec_len(N)) for req in REQ}
        csum = {req: np.zeros(nat.cvec_len(N)) for req in REQ}
        mins = {req: [] for req in REQ}
        cmins = {req: [] for req in REQ}
        covered = {L: 0, R: 0}
        aligned = []
        for rank in range(world):
            eng.set_shard(rank, world)
            eng.nn_pair()
            for d in (L, R):
                b, e = eng.shard_range(d)
                assert b == covered[d] and e > b
                covered[d] = e
            b, e = eng.shard_range(L)
            aligned.append(b % 8192 == 0 and (e % 8192 == 0 or e == N))
            if aligned[-1]:
                buf, lens, mms = eng.reduce_chunks_many(REQ)
                assert lens == [nat.cvec_len(N)] * 4
                for i, req in enumerate(REQ):
                    csum[req] += buf[sum(lens[:i]):sum(lens[:i + 1])]
                    cmins[req].append(mms[i])
            else:
                with pytest.raises(nat.PccmStateError):
                    eng.reduce_chunks_many(REQ)
            eng.reduce_prefetch_many(REQ)
            for req in REQ:
                xvec, mn, mx = eng.reduce(*req)
                xsum[req] += xvec
                mins[req].append((mn, mx))
        assert covered == {L: N, R: N}
        assert aligned == [world == 2] * world       # whole chunks for two ranks, leaves for four
        for req in REQ:
            col = cols[req]
            assert _bits(eng.finish_sum(xsum[req], N)) == _bits(np.sum(col)), (req, "leaves")
            assert _bits(min(m[0] for m in mins[req])) == _bits(np.min(col))
            assert _bits(max(m[1] for m in mins[req])) == _bits(np.max(col))
            if all(aligned):
                assert _bits(eng.finish_chunks(csum[req], N)) == _bits(np.sum(col)), (req, "chunks")
                assert _bits(min(m[0] for m in cmins[req])) == _bits(np.min(col))
                assert _bits(max(m[1] for m in cmins[req])) == _bits(np.max(col))
    finally:
        eng.close()


def _between(col, at):
    """a number strictly between two neighbouring values of the column, near its at-th smallest"""
    s = np.sort(col)
    while True:
        x = np.float64(0.5) * (s[at] + s[at + 1])
        if s[at] < x < s[at + 1]:
            return float(x)
        at += 1


def test_replays_restore_pending_and_idle_slots(pair):
    pts, nrm, cols = pair
    k = (N + 1) // 2
    sel = [(L, D1, k), (R, D1, k)]
    cnt = [(d, D1, _between(cols[(d, D1)], N // 3)) for d in (L, R)]
    maps = [(d, D1, nat.MAP_CLAMP | nat.MAP_ROOT, _between(cols[(d, D1)], (2 * N) // 3)) for d in (L, R)]
    for d, m, _, cap in maps:
        assert np.min(cols[(d, m)]) < cap < np.max(cols[(d, m)])
    eng = _engine(pts, nrm)

    def enqueue():
        eng.drop_caches()
        eng.nn_pair()
        eng.reduce_prefetch_many(REQ)
        eng.select_prefetch_many(sel)
        eng.count_prefetch_many(cnt)
        eng.reduce_map_prefetch_many(maps)

    try:
        for _ in range(2):                            # (a capture allocates nothing: run the sequence first)
            enqueue()
            totals = [_bits(t) for t in eng.reduce_total_many(REQ)]
            picks = [_bits(v) for v in eng.select_many(sel)]
            counts = eng.count_many(cnt)
            mapped = [_bits(t) for t in eng.reduce_map_total_many(maps)]
        for req, t in zip(REQ, totals):
            col = cols[req]
            assert t == _bits([np.sum(col), np.min(col), np.max(col)]), req
        for (d, m, _), v in zip(sel, picks):
            assert v == _bits(np.partition(cols[(d, m)], k - 1)[k - 1])
        for (d, m, x), c in zip(cnt, counts):
            assert c == np.count_nonzero(cols[(d, m)] <= x) and 0 < c < N
        for (d, m, which, cap), t in zip(maps, mapped):
            assert t == _bits(chamfer_reference.totals(cols[(d, m)], which, cap)), (d, m)
        eng.graph_begin()
        enqueue()
        gid = eng.graph_end()                          # (runs the graph once)
        assert [_bits(t) for t in eng.reduce_total_many(REQ)] == totals
        assert [_bits(v) for v in eng.select_many(sel)] == picks
        assert eng.count_many(cnt) == counts
        assert [_bits(t) for t in eng.reduce_map_total_many(maps)] == mapped
        # each replay consumes another part of what it enqueued: the next one meets those slots idle and the others pending
        parts = [([0, 2], [0], [1], [0]), ([1, 3], [1], [0], [1]), ([0, 1, 2, 3], [0, 1], [0, 1], [0, 1])]
        for reqs, sels, cnts, mps in parts:
            eng.graph_launch(gid)
            got = eng.reduce_total_many([REQ[i] for i in reqs])
            assert [_bits(t) for t in got] == [totals[i] for i in reqs], reqs
            got = eng.select_many([sel[i] for i in sels])
            assert [_bits(v) for v in got] == [picks[i] for i in sels], sels
            assert eng.count_many([cnt[i] for i in cnts]) == [counts[i] for i in cnts], cnts
            got = eng.reduce_map_total_many([maps[i] for i in mps])
            assert [_bits(t) for t in got] == [mapped[i] for i in mps], mps
        eng.graph_destroy(gid)
    finally:
        eng.close()


def _select_family(cols):
    ranks = [1, N, (N + 1) // 2] + [2 + 773 * i for i in range(37)]
    reqs = [REQ[i % 4] + (r,) for i, r in enumerate(ranks)]
    return reqs, "select_prefetch_many", "select_many", lambda col, r: _bits(np.partition(col, r - 1)[r - 1]), _bits


def _count_family(cols):
    # every other threshold is a value of the column it is counted in (<= includes it), the others lie between two values
    reqs = []
    for i in range(40):
        col = cols[REQ[i % 4]]
        at = (i + 1) * N // 42
        reqs.append(REQ[i % 4] + (float(np.sort(col)[at]) if i % 8 < 4 else _between(col, at),))
    return reqs, "count_prefetch_many", "count_many", lambda col, x: int(np.count_nonzero(col <= x)), int


def _map_family(cols):
    # clamp and clamp + root in turn, every cap inside its column's range
    reqs = []
    for i in range(40):
        which = nat.MAP_CLAMP | (nat.MAP_ROOT if i % 8 < 4 else 0)
        reqs.append(REQ[i % 4] + (which, _between(cols[REQ[i % 4]], (i + 1) * N // 42)))
    return (reqs, "reduce_map_prefetch_many", "reduce_map_total_many",
            lambda col, which, cap: _bits(chamfer_reference.totals(col, which, cap)), _bits)


@pytest.mark.parametrize("family", [_select_family, _count_family, _map_family])
def test_given_up_slots_are_answered_again(pair, family):
    """Five batches of eight distinct requests on a table of 32 slots, none consumed in between: the fifth batch finds every slot
    pending and current and takes the first batch's (pick_free's third tier).  Consumed in enqueue order, the first batch is
    computed again -- on the slots of the fifth, which is computed again in its turn -- and every answer is the oracle's."""
    pts, nrm, cols = pair
    reqs, prefetch, consume, want, as_bits = family(cols)
    assert len(reqs) == 40 and len({r[2:] for r in reqs}) == 40
    eng = _engine(pts, nrm)
    try:
        eng.nn_pair()
        plain = [_bits(t) for t in eng.reduce_total_many(REQ)]
        for b in range(5):
            getattr(eng, prefetch)(reqs[8 * b:8 * b + 8])
        for b in range(5):
            batch = reqs[8 * b:8 * b + 8]
            got = getattr(eng, consume)(batch)
            assert [as_bits(v) for v in got] == [want(cols[r[:2]], *r[2:]) for r in batch], (b, batch)
        assert [_bits(t) for t in eng.reduce_total_many(REQ)] == plain
        for req, t in zip(REQ, plain):
            col = cols[req]
            assert t == _bits([np.sum(col), np.min(col), np.max(col)]), req
    finally:
        eng.close()
