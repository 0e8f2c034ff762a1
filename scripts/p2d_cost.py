"""Cost of the point-to-distribution rows (CalculateOptions(point_to_distribution=True)) on a resident pair (DESIGN.md,
"Point-to-distribution").

    python scripts/p2d_cost.py [--steps 20] [--warmup 5] [--k 30] [--pair uniform|content|both] [--only without|p2d|build]

bench.py's 1M vs 1M uniform pair (unit normals; D1 + D2 + Hausdorff rows) and its 0.8M voxelised surrogate (no normals; D1 +
Hausdorff rows).  Two figures per pair:

* the build: pccm_p2d_build (both directions: two searches across the clouds and two solves), timed on the host clock around a
  pccm_sync, median of `steps` builds (each timed build follows an untimed one at another k, so that nothing is reused);
* the report: one resident pair without the rows and one with them, stepped alternately: recompute() + the report, with the
  hipGraph replay bench.py measures.  The columns are built once, by the first report.  The figure is the median per report and
  the difference.

One JSON line per pair.  For the kernels' own times run the build alone under
``rocprofv3 --kernel-trace --stats -- python scripts/p2d_cost.py --only build --pair uniform`` (k_knn_cov_wave, k_knn_normals,
k_knn_normals_full, k_p2d_geometry and the grid build)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import synth, synth_content  # noqa: E402
from open_pcc_metric_amd.calculator import MetricCalculator  # noqa: E402
from open_pcc_metric_amd.cloud_pair import CloudPair  # noqa: E402
from open_pcc_metric_amd.options import CalculateOptions, transform_options  # noqa: E402
from open_pcc_metric_amd.point_cloud import PointCloud  # noqa: E402


def step(pair, metrics, first):
    t0 = time.perf_counter()
    if not first:
        pair.recompute()
    with np.errstate(divide="ignore"):
        rows = MetricCalculator(pair).calculate(metrics).as_dict()      # (a fresh calculator: no memoised rows)
    return time.perf_counter() - t0, rows


def build_ms(pair, k, reps):
    eng = pair._engine
    ts = []
    for _ in range(reps):
        eng.p2d_build(k + 1 if k < 64 else k - 1)                      # (another k: the timed build below starts from nothing)
        eng.sync()
        t0 = time.perf_counter()
        assert eng.p2d_build(k)
        eng.sync()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(ts)), 4)


def measure(name, clouds, base, extent, args):
    make = lambda **kw: CloudPair(clouds[0](), clouds[1](), extent=extent, **kw)       # noqa: E731
    out = {"pair": name, "points": [len(clouds[0]().points), len(clouds[1]().points)], "steps": args.steps, "k": args.k}
    if args.only in (None, "build"):
        with make() as pair:
            out["build_ms_both_directions"] = build_ms(pair, args.k, args.steps)
    if args.only == "build":
        return out
    runs = {"without": CalculateOptions(**base), "p2d": CalculateOptions(**base, point_to_distribution=True, p2d_neighbours=args.k)}
    if args.only:
        runs = {args.only: runs[args.only]}
    pairs = {k: make(use_graph=True) for k in runs}
    metrics = {k: transform_options(o) for k, o in runs.items()}
    ts = {k: [] for k in runs}
    rows = {}
    try:
        for s in range(args.warmup + args.steps):
            for k in runs:                                               # alternated: both see the same machine state
                dt, rows[k] = step(pairs[k], metrics[k], s == 0)
                if s >= args.warmup:
                    ts[k].append(dt)
    finally:
        for p in pairs.values():
            p.close()
    for k in runs:
        out["report_ms_" + k] = round(1e3 * float(np.median(ts[k])), 4)
        out["rows_" + k] = len(rows[k])
    if len(runs) == 2:
        out["added_ms_p2d"] = round(out["report_ms_p2d"] - out["report_ms_without"], 4)
        out["other_rows_identical"] = bool(all(np.asarray(rows["p2d"][key]).tobytes() == np.asarray(v).tobytes()
                                               for key, v in rows["without"].items()))
    if "p2d" in runs:
        for cls in ("MahalanobisDistance", "MaxMahalanobisDistance"):
            out[cls] = [float(rows["p2d"][(cls, True, args.k)]), float(rows["p2d"][(cls, False, args.k)])]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--pair", choices=("uniform", "content", "both"), default="both")
    ap.add_argument("--only", choices=("without", "p2d", "build"), default=None)
    args = ap.parse_args()
    if args.pair in ("uniform", "both"):
        a, b, na, nb = synth(1_000_000)
        clouds = (lambda: PointCloud(a, na), lambda: PointCloud(b, nb))
        print(json.dumps(measure("uniform 1M + 1M", clouds, dict(color=None, hausdorff=True, point_to_plane=True), [1.0, 1.0, 1.0], args)),
              flush=True)
    if args.pair in ("content", "both"):
        ca, cb = synth_content()
        clouds = (lambda: PointCloud(ca), lambda: PointCloud(cb))
        print(json.dumps(measure("voxelised surrogate 0.8M", clouds, dict(color=None, hausdorff=True), [1024.0, 1024.0, 1024.0], args)),
              flush=True)


if __name__ == "__main__":
    main()
