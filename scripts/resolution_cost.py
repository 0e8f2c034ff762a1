"""Cost of the resolution-adaptive PSNR rows (CalculateOptions(resolution_psnr=True)) on a resident pair (DESIGN.md,
"Resolution-adaptive PSNR").

    python scripts/resolution_cost.py [--steps 20] [--warmup 5] [--only without|with] [--k 10]

bench.py's 1M vs 1M uniform pair (unit normals; D1 + D2 + Hausdorff rows).  Two figures:

* the build: pccm_resolution_build of each cloud at K neighbours, timed on the host clock around a pccm_sync, median of 5 builds
  (each timed build follows an untimed one at another K, so that nothing is reused);
* the report: one resident pair per configuration -- without the option and with it --, stepped alternately: recompute() + the
  report, with the hipGraph replay bench.py measures.  The columns are built once, by the first report.  The figure is the median
  per report and the difference to "without".

``--ssim-geometry``: also the build of the PointSSIM geometry features of cloud 0 at k = 12 (the other branch of k_ssim_features),
the same way.

One JSON line.  For the kernels' own times run it under
``rocprofv3 --kernel-trace --stats -- python scripts/resolution_cost.py --only with`` (k_knn_cov_wave, k_knn_normals,
k_ssim_features and k_unit_jobs)."""
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


def timed_builds(eng, build, other, reps=5):
    ts = []
    for _ in range(reps):
        other()                                                        # (another size: the timed build below starts from nothing)
        eng.sync()
        t0 = time.perf_counter()
        assert build()
        eng.sync()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(ts)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--only", choices=("without", "with"), default=None)
    ap.add_argument("--ssim-geometry", action="store_true")
    args = ap.parse_args()
    a, b, na, nb = synth(1_000_000)
    base = dict(color=None, hausdorff=True, point_to_plane=True)
    runs = {"without": CalculateOptions(**base),
            "with": CalculateOptions(**base, resolution_psnr=True, resolution_neighbours=args.k)}
    if args.only:
        runs = {args.only: runs[args.only]}
    out = {"points": [len(a), len(b)], "steps": args.steps, "k": args.k}
    if not args.only:
        with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0]) as pair:
            eng = pair._engine
            other = args.k + 1 if args.k < 63 else args.k - 1
            for which in (0, 1):
                out[f"build_ms_cloud{which}"] = timed_builds(eng, lambda: eng.resolution_build(which, args.k),
                                                             lambda: eng.resolution_build(which, other))
            if args.ssim_geometry:
                out["build_ms_ssim_geometry_k12"] = timed_builds(eng, lambda: eng.ssim_features(0, 12, ["geometry"]),
                                                                 lambda: eng.ssim_features(0, 13, ["geometry"]))
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
    for k in runs:
        out["report_ms_" + k] = round(1e3 * float(np.median(ts[k])), 4)
        out["rows_" + k] = len(rows[k])
    if len(runs) == 2:
        out["added_ms"] = round(out["report_ms_with"] - out["report_ms_without"], 4)
        out["other_rows_identical"] = bool(all(np.asarray(rows["with"][key]).tobytes() == np.asarray(v).tobytes()
                                               for key, v in rows["without"].items()))
    if "with" in runs:
        out["IntrinsicResolution"] = [float(rows["with"][("IntrinsicResolution", side, args.k)]) for side in (True, False)]
        out["GeoResolutionPSNR"] = [float(rows["with"][("GeoResolutionPSNR", side, False, args.k)]) for side in (True, False)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
