"""NumPy restatement of carried normals (include/pccm.h, pccm_carry_normals) -- the yardstick of the carry tests.

TEST INFRASTRUCTURE.  ``carried_normals`` groups the source rows by the target row they matched with a stable argsort (so every
group keeps ascending row order), then takes one vectorised step per list position: the first row of every list is assigned,
each later one is added -- one separately rounded fp64 add per component -- and the sums are divided once by the list length;
target rows that nobody matched copy the normal of their own matched row.  ``CarryOracleEngine`` is the CPU test double of
tests/oracle_engine.py with that operation (and a stand-in normal estimator), so that ``CloudPair``'s wiring can be run without a
GPU."""
import numpy as np

from open_pcc_metric_amd import _native as nat
from oracle_engine import OracleEngine


def carried_normals(n_from, rows_f, rows_g, n_to):
    """n_from [nf][3]; rows_f [nf]: the target row every source row matched; rows_g [n_to]: the source row every target row
    matched -> [n_to][3] fp64."""
    src = np.ascontiguousarray(np.asarray(n_from, dtype=np.float64))
    rows_f = np.asarray(rows_f, dtype=np.int64)
    rows_g = np.asarray(rows_g, dtype=np.int64)
    assert src.shape == (len(rows_f), 3) and len(rows_g) == n_to
    order = np.argsort(rows_f, kind="stable")              # grouped by target, ascending source row inside a group
    count = np.bincount(rows_f, minlength=n_to).astype(np.int64)
    start = np.concatenate(([0], np.cumsum(count)[:-1]))
    out = np.empty((n_to, 3), dtype=np.float64)
    acc = np.zeros((n_to, 3), dtype=np.float64)
    for pos in range(int(count.max()) if len(count) else 0):
        live = np.flatnonzero(count > pos)
        rows = order[start[live] + pos]
        if pos == 0:
            acc[live] = src[rows]
        else:
            acc[live] = acc[live] + src[rows]
    has = count > 0
    out[has] = acc[has] / count[has].astype(np.float64)[:, None]
    out[~has] = src[rows_g[~has]]
    return out


def carried_normals_reversed(n_from, rows_f, rows_g, n_to):
    """The same lists summed in DESCENDING row order: what a kernel that ignores the order could return."""
    src = np.asarray(n_from, dtype=np.float64)
    nf = len(src)
    return carried_normals(src[::-1], np.asarray(rows_f)[::-1], nf - 1 - np.asarray(rows_g, dtype=np.int64), n_to)


class CarryOracleEngine(OracleEngine):
    """OracleEngine with pccm_carry_normals, pccm_estimate_normals (a stand-in: unit vectors from the coordinates' hash, enough
    to tell estimated from carried) and pccm_get_normals."""

    def set_cloud(self, which, points):
        super().set_cloud(which, points)
        self.nrm[which] = None                              # (pccm_set_cloud drops the cloud's normals ...)
        if getattr(self, "carried_to", None) is not None:   # (... and normals carried to or from it)
            self.nrm[self.carried_to] = None
        self.carried_to = None

    def set_normals(self, which, normals):
        super().set_normals(which, normals)
        if getattr(self, "carried_to", None) == 1 - which:
            self.nrm[1 - which] = None
        self.carried_to = None

    def estimate_normals(self, which, knn=30):
        p = self.pts[which]
        v = np.stack([np.sin(p[:, 0] * 3.0 + 1.0), np.cos(p[:, 1] * 5.0), np.sin(p[:, 2] * 7.0) + 1.5], axis=1)
        self.set_normals(which, v / np.linalg.norm(v, axis=1)[:, None])
        self.calls.append(("estimate", which))

    def get_normals(self, which):
        return self.nrm[which].copy()

    def carry_normals(self, from_which):
        to = 1 - from_which
        if self.world != 1:
            raise nat.PccmStateError("sharded")
        d_f, d_g = (nat.DIR_LEFT, nat.DIR_RIGHT) if from_which == 0 else (nat.DIR_RIGHT, nat.DIR_LEFT)
        if self.nrm[from_which] is None or d_f not in self.res or d_g not in self.res:
            raise nat.PccmStateError("nothing to carry")
        self.nrm[to] = carried_normals(self.nrm[from_which], self.res[d_f][0], self.res[d_g][0], len(self.pts[to]))
        self.carried_to = to
        self.calls.append(("carry", from_which))
        return True
