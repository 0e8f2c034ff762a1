"""Cost of alignment (CloudPair(align="icp")) on a resident pair ("Alignment").

    python scripts/align_cost.py [--points 1000000] [--steps 10] [--warmup 3] [--degrees 1.0]

bench.py's uniform cloud against itself moved by a small rigid motion (``--degrees`` about (1, 2, 3) and a shift of 1e-3) and
permuted.  Two figures:

* one ICP iteration on resident clouds, as align.icp runs it: the search of direction RIGHT, the inlier count, the sixteen moment
  sums (two calls) and the move of cloud 1 -- each timed to its own synchronisation, median over ``--steps``;
* a full default alignment: ``CloudPair(..., align="icp")`` minus the same pair built without it, which also pays the upload and
  the report's two searches; with its iterations, fitness and inlier RMSE.

One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import synth  # noqa: E402
from open_pcc_metric_amd import _native as nat  # noqa: E402
from open_pcc_metric_amd import align as al  # noqa: E402
from open_pcc_metric_amd.cloud_pair import CloudPair  # noqa: E402
from open_pcc_metric_amd.point_cloud import PointCloud  # noqa: E402


def rigid(degrees, shift):
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    th = np.radians(degrees)
    k = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(th) * k + (1.0 - np.cos(th)) * (k @ k)
    m[:3, 3] = shift
    return m


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--degrees", type=float, default=1.0)
    args = ap.parse_args()
    a = np.asarray(synth(args.points)[0], dtype=np.float64)
    planted = rigid(args.degrees, (1e-3, -1e-3, 5e-4))
    perm = np.random.default_rng(1).permutation(len(a))
    b = np.ascontiguousarray((a @ planted[:3, :3].T + planted[:3, 3])[perm])
    out = {"points": [len(a), len(b)], "steps": args.steps, "degrees": args.degrees}

    # ---- one iteration, piece by piece
    eng = nat.Engine(0)
    try:
        eng.set_cloud(0, a); eng.set_cloud(1, b)
        eng.nn_want_idx(True)
        c = al.centre_of(*eng.get_bounds(0))
        step, back = rigid(0.01, (1e-5, 0.0, 0.0)), None
        back = np.linalg.inv(step)
        parts = {k: [] for k in ("search", "count", "moments", "move", "iteration")}
        req = [(nat.DIR_RIGHT, kind, float("inf")) for kind in range(nat.MOMENT_KINDS)]
        for s in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            dt_s, _ = timed(lambda: (eng.nn(nat.DIR_RIGHT, "auto"), eng.sync()))
            dt_c, m = timed(lambda: eng.count_many([(nat.DIR_RIGHT, nat.METRIC_D1, float("inf"))]))
            dt_m, sums = timed(lambda: eng.reduce_moment_total_many(req[:8], c) + eng.reduce_moment_total_many(req[8:], c))
            dt_t, _ = timed(lambda: eng.transform_cloud(1, step if s % 2 == 0 else back))
            if s >= args.warmup:
                for k, v in zip(parts, (dt_s, dt_c, dt_m, dt_t, time.perf_counter() - t0)):
                    parts[k].append(v)
        out["iteration_ms"] = {k: round(1e3 * float(np.median(v)), 4) for k, v in parts.items()}
        out["moment_path"] = eng.last_path(nat.PATH_REDUCE)
    finally:
        eng.close()

    # ---- a full default alignment, against the same pair without it
    full, plain = [], []
    result = None
    for s in range(2 + 3):
        for align, sink in (("icp", full), (None, plain)):
            dt, pair = timed(lambda: CloudPair(PointCloud(a), PointCloud(b), align=align))
            if align:
                result = pair.alignment
            pair.close()
            if s >= 2:
                sink.append(dt)
    out["pair_ms_with_align"] = round(1e3 * float(np.median(full)), 3)
    out["pair_ms_without"] = round(1e3 * float(np.median(plain)), 3)
    out["alignment_ms"] = round(out["pair_ms_with_align"] - out["pair_ms_without"], 3)
    out["iterations"], out["converged"] = result.iterations, bool(result.converged)
    out["fitness"], out["inlier_rmse"] = result.fitness, result.inlier_rmse
    out["max_abs_error_vs_planted_inverse"] = float(np.max(np.abs(result.transformation - np.linalg.inv(planted))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
