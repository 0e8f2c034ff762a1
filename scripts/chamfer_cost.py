"""Cost of the Chamfer and truncated-distance rows (CalculateOptions(chamfer=True, truncate=...)) on a resident pair
("Chamfer and truncated distances").

    python scripts/chamfer_cost.py [--steps 20] [--warmup 5] [--only without|with] [--truncate TAU ...]

bench.py's 1M vs 1M uniform pair (unit normals; D1 + D2 + Hausdorff rows).  One resident pair per configuration -- without the
options and with them --, stepped alternately: recompute() + the report, with the hipGraph replay bench.py measures.  The figures
are the median per report, the difference to "without", and -- from a few more steps under pccm_profile_enable, run eagerly -- the
launches and the GPU time per report of every kernel class (the mapped batches count under "reduce": the difference of that class
between the two configurations is their GPU time).

``--only without`` needs nothing of the feature: the same file run from an older checkout gives that checkout's figure for the
same report.

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


def profiled(pair, metrics, steps=3):
    """-> {kernel class: [launches per report, GPU ms per report]} over eager steps (a replayed graph records no spans)."""
    eng = pair._engine
    pair._use_graph, pair._graph_id = False, None
    step(pair, metrics, False)
    eng.profile(True)
    eng.profile_reset()
    for _ in range(steps):
        step(pair, metrics, False)
    out = {}
    for name in nat.KERNEL_CLASSES:
        ms, launches = eng.profile_get(name)
        if launches:
            out[name] = [round(launches / steps, 2), round(ms / steps, 4)]
    eng.profile(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("without", "with"), default=None)
    ap.add_argument("--truncate", type=float, action="append", default=None, help="thresholds of the 'with' report (default: 0.005 0.01)")
    args = ap.parse_args()
    taus = tuple(args.truncate or (0.005, 0.01))
    a, b, na, nb = synth(1_000_000)
    base = dict(color=None, hausdorff=True, point_to_plane=True)
    runs = {"without": lambda: CalculateOptions(**base), "with": lambda: CalculateOptions(**base, chamfer=True, truncate=taus)}
    if args.only:
        runs = {args.only: runs[args.only]}
    out = {"points": [len(a), len(b)], "steps": args.steps, "truncate": list(taus)}
    pairs = {k: CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0], use_graph=True) for k in runs}
    metrics = {k: transform_options(o()) for k, o in runs.items()}
    ts = {k: [] for k in runs}
    rows = {}
    try:
        for s in range(args.warmup + args.steps):
            for k in runs:                                               # alternated: both see the same machine state
                dt, rows[k] = step(pairs[k], metrics[k], s == 0)
                if s >= args.warmup:
                    ts[k].append(dt)
        for k in runs:
            out["profile_" + k] = profiled(pairs[k], metrics[k])
        if "with" in runs:
            out["reduce_path_with"] = pairs["with"]._engine.last_path(nat.PATH_REDUCE)
            out["mapped_reductions"] = len(pairs["with"]._results["mapped"][1])
    finally:
        for p in pairs.values():
            p.close()
    for k in runs:
        out["report_ms_" + k] = round(1e3 * float(np.median(ts[k])), 4)
        out["report_ms_min_" + k] = round(1e3 * float(np.min(ts[k])), 4)
        out["rows_" + k] = len(rows[k])
    if len(runs) == 2:
        out["added_ms"] = round(out["report_ms_with"] - out["report_ms_without"], 4)
        out["other_rows_identical"] = bool(all(np.asarray(rows["with"][key]).tobytes() == np.asarray(v).tobytes()
                                               for key, v in rows["without"].items()))
        r0, r1 = out["profile_without"].get("reduce", [0, 0.0]), out["profile_with"].get("reduce", [0, 0.0])
        out["mapped_gpu_ms"] = round(r1[1] - r0[1], 4)
        out["mapped_launches"] = round(r1[0] - r0[0], 2)
    if "with" in runs:
        out["GeoChamferL1"] = float(rows["with"][("GeoChamferL1",)])
        out["GeoChamferL2"] = float(rows["with"][("GeoChamferL2",)])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
