"""Cost of the PointSSIM rows (CalculateOptions(point_ssim=...)) on a resident pair ("PointSSIM").

    python scripts/pointssim_cost.py [--steps 20] [--warmup 5] [--only without|geometry|normal|curvature|color|all] [--k 12]

bench.py's 1M vs 1M uniform pair (unit normals, byte colours; D1 + D2 + Hausdorff rows).  Two figures:

* the feature build: pccm_ssim_features of one cloud for one attribute (and all four at once), timed on the host clock around a
  pccm_sync, median of 5 builds (each timed build follows an untimed one at another k, so that nothing is reused);
* the report: one resident pair per configuration -- without PointSSIM, with each attribute alone, with all four --, stepped
  alternately: recompute() + the report, with the hipGraph replay bench.py measures.  The features are built once, by the first
  report.  The figure is the median per report and the difference to "without".

One JSON line.  For the kernels' own times run it under
``rocprofv3 --kernel-trace --stats -- python scripts/pointssim_cost.py --only all`` (k_knn_cov_wave, k_ssim_curvature, k_ssim_features and
k_point_jobs)."""
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

ATTRS = ("geometry", "normal", "curvature", "color")


def step(pair, metrics, first):
    t0 = time.perf_counter()
    if not first:
        pair.recompute()
    with np.errstate(divide="ignore"):
        rows = MetricCalculator(pair).calculate(metrics).as_dict()      # (a fresh calculator: no memoised rows)
    return time.perf_counter() - t0, rows


def build_ms(pair, attrs, k, reps=5):
    eng = pair._engine
    pair._ensure_ssim(attrs, k)                                        # normals / colours on the device first
    ts = []
    for _ in range(reps):
        eng.ssim_features(0, k + 1, attrs)                             # (another k: the timed build below starts from nothing)
        eng.sync()
        t0 = time.perf_counter()
        assert eng.ssim_features(0, k, attrs)
        eng.sync()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(ts)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--only", choices=("without",) + ATTRS + ("all",), default=None)
    args = ap.parse_args()
    a, b, na, nb = synth(1_000_000)
    rng = np.random.default_rng(99)
    ca, cb = rng.integers(0, 256, (len(a), 3)) / 255.0, rng.integers(0, 256, (len(b), 3)) / 255.0
    base = dict(color=None, hausdorff=True, point_to_plane=True)
    runs = {"without": CalculateOptions(**base)}
    for attr in ATTRS:
        runs[attr] = CalculateOptions(**base, point_ssim=[attr], ssim_neighbours=args.k)
    runs["all"] = CalculateOptions(**base, point_ssim=ATTRS, ssim_neighbours=args.k)
    if args.only:
        runs = {args.only: runs[args.only]}
    out = {"points": [len(a), len(b)], "steps": args.steps, "k": args.k}
    if not args.only:
        with CloudPair(PointCloud(a, na, ca), PointCloud(b, nb, cb), extent=[1.0, 1.0, 1.0]) as pair:
            for attr in ATTRS:
                out["build_ms_" + attr] = build_ms(pair, [attr], args.k)
            out["build_ms_all"] = build_ms(pair, list(ATTRS), args.k)
    pairs = {k: CloudPair(PointCloud(a, na, ca), PointCloud(b, nb, cb), extent=[1.0, 1.0, 1.0], use_graph=True) for k in runs}
    metrics = {k: transform_options(o) for k, o in runs.items()}
    ts = {k: [] for k in runs}
    rows = {}
    try:
        for s in range(args.warmup + args.steps):
            for k in runs:                                               # alternated: all see the same machine state
                dt, rows[k] = step(pairs[k], metrics[k], s == 0)
                if s >= args.warmup:
                    ts[k].append(dt)
    finally:
        for p in pairs.values():
            p.close()
    for k in runs:
        out["report_ms_" + k] = round(1e3 * float(np.median(ts[k])), 4)
        out["rows_" + k] = len(rows[k])
    if "without" in runs:
        for k in runs:
            if k != "without":
                out["added_ms_" + k] = round(out["report_ms_" + k] - out["report_ms_without"], 4)
                same = all(np.asarray(rows[k][key]).tobytes() == np.asarray(v).tobytes() for key, v in rows["without"].items())
                out["other_rows_identical_" + k] = bool(same)
    if "all" in runs:
        for attr, cls in zip(ATTRS, ("GeometrySSIM", "NormalSSIM", "CurvatureSSIM", "ColorSSIM")):
            out[cls] = [float(rows["all"][(cls, True, args.k)]), float(rows["all"][(cls, False, args.k)])]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
