"""Cost of pccm_merge_duplicates on one resident cloud, beside the host alternative it replaces ("Duplicate points").

    python scripts/merge_cost.py [--n 1000000] [--rounds 10] [--mode average]

Three inputs of ``n`` fp32 rows with colours: no duplicate, about 10 % of the rows duplicated, and all rows identical (one group of
n rows: the averaging walk's worst case).  Every timed merge follows an untimed upload of the same cloud and colours; it is timed
with HIP events on the context's stream around the call, with the host clock, and with the library's own profile of its point-kernel
launches (pccm_profile_get(PCCM_K_POINT)).  The host alternative is ``np.unique(points, axis=0)`` on the same array as fp64 plus
the upload of its result.  One JSON line per input: median, min and max in ms."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4), "calls": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--mode", default="average", choices=["drop", "average"])
    ap.add_argument("--no-host", action="store_true", help="skip the np.unique arm")
    args = ap.parse_args()
    import torch
    from open_pcc_metric_amd import _native as nat

    n = args.n
    rng = np.random.default_rng(0)
    base = rng.random((n, 3), dtype=np.float32)
    tenth = base.copy()
    dup = rng.permutation(n)[: n // 10]
    tenth[dup] = base[rng.integers(0, n, n // 10)]
    inputs = {"no_duplicates": base, "tenth_duplicated": tenth, "all_identical": np.repeat(base[:1], n, axis=0)}
    colours = rng.integers(0, 256, (n, 3)) / 255.0
    stream = torch.cuda.Stream()
    eng = nat.Engine(0, stream=stream.cuda_stream)
    try:
        for name, pts in inputs.items():
            rounds = max(3, args.rounds // 3) if name == "all_identical" else args.rounds
            ev_ms, wall_ms, kern_ms, left = [], [], [], None
            for r in range(rounds + 2):                                  # two warm-up rounds (allocations, code load)
                eng.set_cloud(0, pts)
                eng.set_colors(0, colours)
                eng.sync()
                eng.profile(True)
                eng.profile_reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                t0 = time.perf_counter()
                left = eng.merge_duplicates(0, args.mode)
                eng.sync()
                t1 = time.perf_counter()
                e1.record(stream)
                e1.synchronize()
                k_ms, launches = eng.profile_get("point")
                eng.profile(False)
                if r >= 2:
                    ev_ms.append(e0.elapsed_time(e1))
                    wall_ms.append(1e3 * (t1 - t0))
                    kern_ms.append(k_ms)
            line = {"input": name, "n": n, "rows_left": left, "mode": args.mode, "hip_events_ms": stats(ev_ms),
                    "host_clock_ms": stats(wall_ms), "point_kernels_ms": stats(kern_ms), "point_launch_groups": launches}
            if not args.no_host:
                uniq_ms, up_ms = [], []
                p64 = pts.astype(np.float64)
                for r in range(3):
                    t0 = time.perf_counter()
                    u = np.unique(p64, axis=0)
                    t1 = time.perf_counter()
                    eng.set_cloud(0, u)
                    eng.sync()
                    t2 = time.perf_counter()
                    uniq_ms.append(1e3 * (t1 - t0))
                    up_ms.append(1e3 * (t2 - t1))
                line["host_np_unique_ms"] = stats(uniq_ms)
                line["host_reupload_ms"] = stats(up_ms)
            print(json.dumps(line), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
