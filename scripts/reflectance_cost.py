"""Cost of the reflectance rows (CalculateOptions(reflectance=True)) on a resident pair ("Reflectance").

    python scripts/reflectance_cost.py [--steps 20] [--warmup 5] [--only without|with]

bench.py's 1M vs 1M uniform pair (unit normals; D1 + D2 + Hausdorff rows), each cloud with a random 16-bit reflectance.  One
resident pair per configuration -- without the option and with it --, stepped alternately: recompute() + the report, with the
hipGraph replay bench.py measures.  The reflectance goes up once, with the first report.  The figures are the median per report,
the difference to "without", and -- from a few more steps under pccm_profile_enable, run eagerly -- the launches and the GPU time
per report of every kernel class.

``--merge``: instead, the cost of pccm_merge_duplicates ("average") of one cloud of 1M rows over 750k positions, with colours,
without and with a reflectance column: host clock around a pccm_sync, median of 5 merges (each of a freshly set cloud).

``--only without`` needs nothing of the feature (the clouds then carry no reflectance): the same file run from an older checkout
gives that checkout's figure for the same report.

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


def merge_cost(reps=5):
    rng = np.random.default_rng(1)
    keys = rng.random((750_000, 3), dtype=np.float32)
    pts = np.concatenate([keys, keys[rng.integers(0, len(keys), 250_000)]])[rng.permutation(1_000_000)]
    col = rng.integers(0, 256, (len(pts), 3)).astype(np.uint8)
    refl = rng.integers(0, 65536, len(pts)).astype(np.uint16)
    out = {"merge_rows": len(pts)}
    eng = nat.Engine(0)
    try:
        for name in ("without", "with", "without", "with"):             # (the first two warm the allocations up)
            ts = []
            for _ in range(reps):
                eng.set_cloud(0, pts)
                eng.set_colors_u8(0, col)
                if name == "with":
                    eng.set_reflectance(0, refl)
                eng.sync()
                t0 = time.perf_counter()
                left = eng.merge_duplicates(0, "average")
                eng.sync()
                ts.append(time.perf_counter() - t0)
            out["merge_ms_" + name] = round(1e3 * float(np.median(ts)), 4)
            out["merge_rows_left"] = left
    finally:
        eng.close()
    out["merge_added_ms"] = round(out["merge_ms_with"] - out["merge_ms_without"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("without", "with"), default=None)
    args = ap.parse_args()
    if args.merge:
        print(json.dumps(merge_cost()))
        return
    a, b, na, nb = synth(1_000_000)
    base = dict(color=None, hausdorff=True, point_to_plane=True)
    runs = {"without": lambda: CalculateOptions(**base), "with": lambda: CalculateOptions(**base, reflectance=True)}
    if args.only:
        runs = {args.only: runs[args.only]}
    rng = np.random.default_rng(0)
    clouds = {"without": lambda: (PointCloud(a, na), PointCloud(b, nb)),
              "with": lambda: (PointCloud(a, na, reflectance=rng.integers(0, 65536, len(a)).astype(np.uint16)),
                               PointCloud(b, nb, reflectance=rng.integers(0, 65536, len(b)).astype(np.uint16)))}
    out = {"points": [len(a), len(b)], "steps": args.steps}
    pairs = {k: CloudPair(*clouds[k](), extent=[1.0, 1.0, 1.0], use_graph=True) for k in runs}
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
        out["ReflectanceMSE"] = [float(rows["with"][("ReflectanceMSE", side)]) for side in (True, False)]
        out["ReflectancePSNR"] = [float(rows["with"][("ReflectancePSNR", side, 65535.0)]) for side in (True, False)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
