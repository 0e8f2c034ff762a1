"""NumPy restatement of ``ties="mean"`` (include/pccm.h, PCCM_TIES_MEAN) -- the yardstick of the tie tests.

TEST INFRASTRUCTURE.  ``tie_sets`` enumerates every equidistant nearest neighbour with a dense fp64 distance matrix in chunks
(``((dx*dx)+(dy*dy))+(dz*dz)``, no contraction: NumPy rounds every operation); ``tie_mean`` adds the rows of each set in
ascending row order and divides once by ``k``.  ``MeanOracleEngine`` is the CPU test double of tests/oracle_engine.py with that
neighbour policy, so that the product's host logic (metric DAG, sharded exchange) can be run against it without a GPU, and the
GPU's reports can be compared with it row by row."""
import numpy as np

from open_pcc_metric_amd import _native as nat
from oracle import oracle as orc
from oracle_engine import OracleEngine


def tie_sets(q, r, chunk=1024):
    """-> (d2 [n], sets: list of ascending int64 row arrays) of every row of q in r."""
    q64, r64 = np.asarray(q, dtype=np.float64), np.asarray(r, dtype=np.float64)
    d2s, sets = np.empty(len(q64)), []
    for s in range(0, len(q64), chunk):
        blk = q64[s:s + chunk]
        dx = blk[:, None, 0] - r64[None, :, 0]
        dy = blk[:, None, 1] - r64[None, :, 1]
        dz = blk[:, None, 2] - r64[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        best = d.min(axis=1)
        d2s[s:s + len(blk)] = best
        hit = d == best[:, None]
        sets.extend(np.flatnonzero(h) for h in hit)
    return d2s, sets


def tie_mean(values, sets):
    """Per set: (((v[j1] + v[j2]) + v[j3]) + ...) / k in fp64."""
    v = np.asarray(values, dtype=np.float64)
    out = np.empty((len(sets), v.shape[1]))
    for i, rows in enumerate(sets):
        acc = v[rows[0]].copy()
        for j in rows[1:]:
            acc = acc + v[j]
        out[i] = acc / np.float64(len(rows))
    return out


class MeanOracleEngine(OracleEngine):
    """OracleEngine with pccm_set_ties: under "mean" the neighbour of directions 0 and 1 is the virtual one of tie_mean."""

    def __init__(self, method="auto"):
        super().__init__(method)
        self.ties = "pick"
        self._sets = {}

    def set_ties(self, policy):
        if policy not in nat.TIES:
            raise ValueError(policy)
        self.ties = policy

    def set_cloud(self, which, points):
        super().set_cloud(which, points)
        self._sets.clear()

    def _full_sets(self, d):
        if d not in self._sets:
            it, se = self._clouds(d)
            self._sets[d] = tie_sets(self.pts[it], self.pts[se])[1]
        return self._sets[d]

    def _mean(self, d):
        return self.ties == "mean" and d in (nat.DIR_LEFT, nat.DIR_RIGHT)

    def tie_counts(self, d):
        b, e = self.shard_range(d)
        return np.array([len(s) for s in self._full_sets(d)[b:e]], dtype=np.int32)

    def error_vectors(self, d):
        if not self._mean(d):
            return super().error_vectors(d)
        it, se = self._clouds(d)
        b, e = self.shard_range(d)
        return self.pts[it][b:e] - tie_mean(self.pts[se], self._full_sets(d)[b:e])

    def point_metric(self, d, metric, normal_mode="row"):
        if not self._mean(d) or metric == nat.METRIC_D1:
            return super().point_metric(d, metric, normal_mode)
        it, se = self._clouds(d)
        b, e = self.shard_range(d)
        nrm = self.nrm[se]
        if nrm is None:
            raise RuntimeError("no normals")
        sets = self._full_sets(d)[b:e]
        c = tie_mean(self.pts[se], sets) if e > b else np.zeros((0, 3))
        rows = np.arange(e - b, dtype=np.int64)
        if normal_mode == "row":
            if (self.n_iter(d) if self.world > 1 else e) > nrm.shape[0]:
                raise IndexError(f"index {nrm.shape[0]} is out of bounds for axis 0 with size {nrm.shape[0]}")
            proj = orc.point_to_plane(self.pts[it][b:e], c, rows, np.ascontiguousarray(nrm[b:e]))
        else:
            navg = tie_mean(nrm, sets) if e > b else np.zeros((0, 3))
            proj = orc.point_to_plane(self.pts[it][b:e], c, rows, navg, normal_index="neighbour")
        return proj if metric == nat.METRIC_PROJ else np.square(proj)

    def _colour_operands(self, d, rows):
        if not self._mean(d):
            return super()._colour_operands(d, rows)
        it, se = self._clouds(d)
        avg = tie_mean(self.rgb[se], self._full_sets(d))
        return self.rgb[it], avg, np.arange(len(avg), dtype=np.int64)
