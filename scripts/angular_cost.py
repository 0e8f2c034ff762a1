"""Cost of the plane-to-plane rows (CalculateOptions(plane_to_plane=True)) on a resident pair ("Plane-to-plane").

    python scripts/angular_cost.py [--steps 30] [--warmup 5] [--only with|without]

bench.py's 1M vs 1M uniform pair (unit normals; D1 + D2 + Hausdorff rows).  Two resident pairs in one process, one reporting
without and one with the angular rows, are stepped alternately: recompute() + the report, timed on the host clock (the
report's numbers are on the host when it returns), with the hipGraph replay bench.py measures.  The figure is the median per
report and the difference.  One JSON line.  For the kernels' own times run it under
``rocprofv3 --kernel-trace --stats -- python scripts/angular_cost.py --only with`` (k_point_jobs)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import synth  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["with", "without"], default=None)
    args = ap.parse_args()
    a, b, na, nb = synth(1_000_000)
    runs = {"without": CalculateOptions(None, True, True), "with": CalculateOptions(None, True, True, plane_to_plane=True)}
    if args.only:
        runs = {args.only: runs[args.only]}
    pairs = {k: CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0], use_graph=True) for k in runs}
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
    out = {"points": [len(a), len(b)], "steps": args.steps}
    for k in runs:
        out[k + "_ms"] = round(1e3 * float(np.median(ts[k])), 4)
        out[k + "_rows"] = len(rows[k])
    if len(runs) == 2:
        out["added_ms"] = round(out["with_ms"] - out["without_ms"], 4)
        out["angular_L"] = float(rows["with"][("AngularSimilarity", True)])
        out["angular_R"] = float(rows["with"][("AngularSimilarity", False)])
        same = all(np.asarray(rows["with"][k]).tobytes() == np.asarray(v).tobytes() for k, v in rows["without"].items())
        out["other_rows_identical"] = bool(same)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
