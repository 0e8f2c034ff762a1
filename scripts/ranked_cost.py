"""Cost of the ranked Hausdorff rows (CalculateOptions(hausdorff_rank=...)) on a resident pair ("Ranked Hausdorff").

    python scripts/ranked_cost.py [--steps 20] [--warmup 5] [--only without|one|three] [--content] [--host]

bench.py's 1M vs 1M uniform pair (unit normals; D1 + D2 + Hausdorff rows), or with ``--content`` its 0.8M-point voxelised
surrogate (no normals; D1 + Hausdorff rows: every column is a few dozen integers, the all-ties case).  Resident pairs in one
process -- one reporting without the option, one with one rank (0.99), one with three (0.95, 0.99, 0.999) -- are stepped
alternately: recompute() + the report, timed on the host clock (the report's numbers are on the host when it returns), with the
hipGraph replay bench.py measures.  The figures are the median per report, the 10th and 90th percentile (the run-to-run spread)
and the differences.  ``--host``: also what the same rows cost without the option -- every column fetched with np.asarray and
ranked with np.partition on the host.  ``--only without`` uses nothing the option added (it also runs on a commit without it).
One JSON line.  For the kernels' own times run it under
``rocprofv3 --kernel-trace --stats -- python scripts/ranked_cost.py --only three`` (k_unit_jobs: seven launches per selection batch)."""
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

RANKS = {"without": None, "one": (0.99,), "three": (0.95, 0.99, 0.999)}


def step(pair, metrics, first):
    t0 = time.perf_counter()
    if not first:
        pair.recompute()
    with np.errstate(divide="ignore"):
        rows = MetricCalculator(pair).calculate(metrics).as_dict()      # (a fresh calculator: no memoised rows)
    return time.perf_counter() - t0, rows


def host_rows(pair, p2plane, ranks):
    """The same rows as a user gets them without the option: the columns over PCIe, np.partition on the host."""
    from open_pcc_metric_amd.metric import rank_index
    t0 = time.perf_counter()
    pair.recompute()
    cols = [np.asarray(pair.get_left_neighbour_distances()), np.asarray(pair.get_right_neighbour_distances())]
    if p2plane:
        cols += [np.asarray(np.square(pair.point_to_plane_column(True))), np.asarray(np.square(pair.point_to_plane_column(False)))]
    out = []
    for col in cols:
        ks = [rank_index(r, len(col)) - 1 for r in ranks]
        part = np.partition(col, ks)
        out += [part[k] for k in ks]
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=sorted(RANKS), default=None)
    ap.add_argument("--content", action="store_true", help="the 0.8M-point voxelised surrogate instead of the uniform pair")
    ap.add_argument("--host", action="store_true", help="also time the host route (np.asarray + np.partition) for three ranks")
    args = ap.parse_args()
    if args.content:
        a, b = synth_content()
        clouds, p2plane, extent = (PointCloud(a), PointCloud(b)), False, [1024.0, 1024.0, 1024.0]
    else:
        a, b, na, nb = synth(1_000_000)
        clouds, p2plane, extent = (PointCloud(a, na), PointCloud(b, nb)), True, [1.0, 1.0, 1.0]
    names = [args.only] if args.only else list(RANKS)
    options = {k: CalculateOptions(None, True, p2plane) if RANKS[k] is None else
               CalculateOptions(None, True, p2plane, hausdorff_rank=RANKS[k]) for k in names}
    pairs = {k: CloudPair(*clouds, extent=extent, use_graph=True) for k in names}
    metrics = {k: transform_options(o) for k, o in options.items()}
    ts = {k: [] for k in names}
    rows, host = {}, []
    try:
        for s in range(args.warmup + args.steps):
            for k in names:                                              # alternated: all see the same machine state
                dt, rows[k] = step(pairs[k], metrics[k], s == 0)
                if s >= args.warmup:
                    ts[k].append(dt)
        if args.host:
            any_pair = pairs[names[0]]
            for s in range(3 + 5):
                dt, _ = host_rows(any_pair, p2plane, RANKS["three"])
                if s >= 3:
                    host.append(dt)
    finally:
        for p in pairs.values():
            p.close()
    out = {"points": [len(a), len(b)], "steps": args.steps, "content": bool(args.content)}
    for k in names:
        t = 1e3 * np.asarray(ts[k])
        out[k + "_ms"] = round(float(np.median(t)), 4)
        out[k + "_p10_p90_ms"] = [round(float(np.percentile(t, 10)), 4), round(float(np.percentile(t, 90)), 4)]
        out[k + "_rows"] = len(rows[k])
    for k in names:
        if k != "without" and "without" in names:
            out[k + "_added_ms"] = round(out[k + "_ms"] - out["without_ms"], 4)
            same = all(np.asarray(rows[k][key]).tobytes() == np.asarray(v).tobytes() for key, v in rows["without"].items())
            out[k + "_other_rows_identical"] = bool(same)
    if host:
        out["host_three_ranks_ms"] = round(1e3 * float(np.median(host)), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
