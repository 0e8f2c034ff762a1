"""``AlignOracleEngine``: the CPU test double (oracle_engine.OracleEngine) with what alignment asks of an engine -- a move of a
resident cloud, inlier counts and the alignment moments, all in NumPy through align_reference.  TEST INFRASTRUCTURE."""
import numpy as np

import align_reference as ar
from oracle_engine import OracleEngine
from open_pcc_metric_amd import _native as nat


class AlignOracleEngine(OracleEngine):
    def set_cloud(self, which, points):
        super().set_cloud(which, points)
        self.nrm[which] = None

    def transform_cloud(self, which, matrix):
        m = np.asarray(matrix, dtype=np.float64)[:3, :4]
        self.calls.append(("transform_cloud", which))
        if np.array_equal(m, np.eye(4)[:3]):
            return
        self.pts[which] = ar.move_points(self.pts[which], m)
        if self.nrm[which] is not None:
            self.nrm[which] = ar.move_normals(self.nrm[which], m)
        for d in list(self.res):
            if d != nat.DIR_SELF or which == 0:
                del self.res[d]

    def get_points(self, which):
        return self.pts[which].copy()

    def get_normals(self, which):
        return self.nrm[which].copy()

    def count_many(self, requests, normal_mode="row"):
        self.calls.append(("count_many", tuple(requests)))
        return [int(np.count_nonzero(self.point_metric(d, metric, normal_mode) <= x)) for d, metric, x in requests]

    def reduce_moment_total_many(self, requests, pivot):
        self.calls.append(("reduce_moment_total_many", tuple(r[1] for r in requests)))
        out = []
        for d, kind, cap in requests:
            it, se = self._clouds(d)
            idx, d2 = self.res[d]
            out.append(ar.moment_totals(kind, self.pts[it], self.pts[se], idx, d2, cap, pivot))
        return out
