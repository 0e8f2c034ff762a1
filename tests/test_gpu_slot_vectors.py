"""What leaves a reduction slot, on the real kernels (open_pcc_metric_amd/csrc/pccm_slot.h; tests/test_slot_host.py is the same
without a GPU): the per-chunk and per-leaf exchange vectors of shards emulated one after the other on one context, summed over
the ranks and finished on the host, and the totals and selections of a captured graph replayed onto slots it finds pending and
idle.  28673 rows = 3 chunks of 8192 + a partial chunk longer than half a chunk: two ranks get whole chunks, four get leaves.
Sums are held to np.sum of the oracle's column bit for bit."""
import numpy as np
import pytest

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


def test_replays_restore_pending_and_idle_slots(pair):
    pts, nrm, cols = pair
    k = (N + 1) // 2
    sel = [(L, D1, k), (R, D1, k)]
    eng = _engine(pts, nrm)
    try:
        for _ in range(2):                            # (a capture allocates nothing: run the sequence first)
            eng.drop_caches()
            eng.nn_pair()
            eng.reduce_prefetch_many(REQ)
            eng.select_prefetch_many(sel)
            totals = [_bits(t) for t in eng.reduce_total_many(REQ)]
            picks = [_bits(v) for v in eng.select_many(sel)]
        for req, t in zip(REQ, totals):
            col = cols[req]
            assert t == _bits([np.sum(col), np.min(col), np.max(col)]), req
        for (d, m, _), v in zip(sel, picks):
            assert v == _bits(np.partition(cols[(d, m)], k - 1)[k - 1])
        eng.graph_begin()
        eng.drop_caches()
        eng.nn_pair()
        eng.reduce_prefetch_many(REQ)
        eng.select_prefetch_many(sel)
        gid = eng.graph_end()                          # (runs the graph once)
        assert [_bits(t) for t in eng.reduce_total_many(REQ)] == totals
        assert [_bits(v) for v in eng.select_many(sel)] == picks
        # each replay consumes another part of what it enqueued: the next one meets those slots idle and the others pending
        parts = [([0, 2], [0]), ([1, 3], [1]), ([0, 1, 2, 3], [0, 1])]
        for reqs, sels in parts:
            eng.graph_launch(gid)
            got = eng.reduce_total_many([REQ[i] for i in reqs])
            assert [_bits(t) for t in got] == [totals[i] for i in reqs], reqs
            got = eng.select_many([sel[i] for i in sels])
            assert [_bits(v) for v in got] == [picks[i] for i in sels], sels
        eng.graph_destroy(gid)
    finally:
        eng.close()
