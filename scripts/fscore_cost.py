"""Cost of the F-score rows (CalculateOptions(fscore=...)) on a resident pair ("F-score").

    python scripts/fscore_cost.py [--steps 20] [--warmup 5] [--only without|with] [--root CHECKOUT]

bench.py's 1M vs 1M uniform pair (unit normals; D1 + D2 + Hausdorff rows).  One resident pair per configuration -- without the
option and with four thresholds --, stepped alternately in one process: recompute() + the report, with the hipGraph replay
bench.py measures.  The figures are the median per report, the difference to "without", and -- from a few more steps under
pccm_profile_enable, run eagerly -- the launches and the GPU time per report of every kernel class.

``--only without`` needs nothing of the feature; with ``--root CHECKOUT`` the package and bench.py are imported from that tree
(an older checkout, built): the same file then gives that checkout's figure for the same report, in a process of its own.

One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

TAUS = (0.0, 0.002, 0.005, 0.01)       # the nearest-neighbour distances of the pair are around 0.005: the counts are not trivial


def step(pair, calculator, metrics, first):
    t0 = time.perf_counter()
    if not first:
        pair.recompute()
    with np.errstate(divide="ignore"):
        rows = calculator(pair).calculate(metrics).as_dict()            # (a fresh calculator: no memoised rows)
    return time.perf_counter() - t0, rows


def profiled(nat, pair, calculator, metrics, steps=3):
    """-> {kernel class: [launches per report, GPU ms per report]} over eager steps (a replayed graph records no spans)."""
    eng = pair._engine
    pair._use_graph, pair._graph_id = False, None
    step(pair, calculator, metrics, False)
    eng.profile(True)
    eng.profile_reset()
    for _ in range(steps):
        step(pair, calculator, metrics, False)
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
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from bench import synth
    from open_pcc_metric_amd import _native as nat
    from open_pcc_metric_amd.calculator import MetricCalculator
    from open_pcc_metric_amd.cloud_pair import CloudPair
    from open_pcc_metric_amd.options import CalculateOptions, transform_options
    from open_pcc_metric_amd.point_cloud import PointCloud

    a, b, na, nb = synth(1_000_000)
    base = dict(color=None, hausdorff=True, point_to_plane=True)
    runs = {"without": lambda: CalculateOptions(**base), "with": lambda: CalculateOptions(**base, fscore=TAUS)}
    if args.only:
        runs = {args.only: runs[args.only]}
    out = {"points": [len(a), len(b)], "steps": args.steps, "root": os.path.abspath(args.root)}
    pairs = {k: CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0], use_graph=True) for k in runs}
    metrics = {k: transform_options(o()) for k, o in runs.items()}
    ts = {k: [] for k in runs}
    rows = {}
    try:
        for s in range(args.warmup + args.steps):
            for k in runs:                                               # alternated: both see the same machine state
                dt, rows[k] = step(pairs[k], MetricCalculator, metrics[k], s == 0)
                if s >= args.warmup:
                    ts[k].append(dt)
        for k in runs:
            out["profile_" + k] = profiled(nat, pairs[k], MetricCalculator, metrics[k])
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
    if "with" in runs:
        out["GeoFScore"] = {repr(t): float(rows["with"][("GeoFScore", t)]) for t in TAUS}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
