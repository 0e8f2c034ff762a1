"""Cost of ties="mean" over ties="pick" on resident pairs ("Exact ties: the mean policy").

    python scripts/ties_cost.py [--steps 30] [--only mean]

Two workloads: bench.py's 1M vs 1M uniform pair (unit normals; D1 + D2 + Hausdorff rows) and its 0.8M voxelised surrogate
(unit normals, byte colours; the full 32-row --color ycc --hausdorff --point-to-plane --normal-index neighbour report).  Per
policy a resident pair runs recompute() + the report; the figure is the median over the steps on the host clock (the
report's numbers are on the host when it returns).  "pick" is timed with its hipGraph replay (what bench.py measures) and
eagerly; "mean" is always eager.  One JSON line.  For the new kernels' own times run it under
``rocprofv3 --kernel-trace --stats -- python scripts/ties_cost.py --only mean``."""
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


def time_pair(a, b, opts, steps, warmup, **kw):
    metrics = transform_options(opts)
    ts, rows = [], None
    with CloudPair(a, b, **kw) as pair:
        for s in range(warmup + steps):
            t0 = time.perf_counter()
            if s:
                pair.recompute()
            with np.errstate(divide="ignore"):
                res = MetricCalculator(pair).calculate(metrics).as_dict()      # (a fresh calculator: no memoised rows)
            ts.append(time.perf_counter() - t0)
            rows = res
    return 1e3 * float(np.median(ts[warmup:])), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["pick", "mean"], default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(7)
    a, b, na, nb = synth(1_000_000)
    ca, cb = synth_content()
    unit = lambda n: (lambda g: g / np.linalg.norm(g, axis=1, keepdims=True))(rng.standard_normal((n, 3)))
    work = {
        "uniform_1M": (PointCloud(a, na), PointCloud(b, nb), CalculateOptions(None, True, True), dict(extent=[1, 1, 1])),
        "voxel_0.8M": (PointCloud(ca, unit(len(ca)), rng.integers(0, 256, (len(ca), 3)) / 255.0),
                       PointCloud(cb, unit(len(cb)), rng.integers(0, 256, (len(cb), 3)) / 255.0),
                       CalculateOptions("ycc", True, True), dict(extent=[1024.0, 1024.0, 1024.0], normal_index="neighbour")),
    }
    out = {}
    for name, (pa, pb, opts, kw) in work.items():
        r = {"points": [len(pa.points), len(pb.points)]}
        runs = [("pick_graph", dict(ties="pick", use_graph=True)), ("pick_eager", dict(ties="pick")), ("mean", dict(ties="mean"))]
        for label, extra in runs:
            if args.only and not label.startswith(args.only):
                continue
            ms, rows = time_pair(pa, pb, opts, args.steps, args.warmup, **kw, **extra)
            r[label + "_ms"] = round(ms, 4)
            r["rows"] = len(rows)
        if "mean_ms" in r and "pick_graph_ms" in r:
            r["mean_extra_ms_vs_graph"] = round(r["mean_ms"] - r["pick_graph_ms"], 4)
            r["mean_extra_ms_vs_eager"] = round(r["mean_ms"] - r["pick_eager_ms"], 4)
        out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
