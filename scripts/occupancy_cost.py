"""Cost of the voxel-occupancy counts (pccm_voxel_occupancy; CalculateOptions(occupancy=...)) on resident pairs (INTEGRATION.md,
"Voxel occupancy"; DESIGN.md, "Voxel occupancy").

    python scripts/occupancy_cost.py [--steps 30] [--warmup 5] [--merge]

bench.py's 1M vs 1M uniform pair (voxels of 1/64 and of 1/256, 1/64, 1/16, 1/4 of the unit cube's edge) and its voxelised 0.8M
content surrogate (integer coordinates: voxels of 1 -- octree level 0 -- and of 1, 2, 4, 8), both resident, no search run.  A
timed call is Engine.voxel_occupancy: the memsets, two launches per size, the copy of the tallies and the one wait, from the
host's point of view; after the warm-up calls the figures are the median and the minimum over ``--steps`` calls.  The counts are
checked against NumPy once per pair and size.

``--merge``: instead, the time of pccm_merge_duplicates ("drop") on a cloud of 1M rows of which a tenth are duplicates, uploaded
afresh before every timed call (the upload is not timed) -- the existing path whose two probe kernels the occupancy mode shares.
The same file run with PCCM_LIB pointing at the parent's library gives the parent's figure.

One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import synth, synth_content  # noqa: E402
from open_pcc_metric_amd import _native as nat  # noqa: E402


def numpy_occupancy(a, b, v):
    """A copy of ``occupancy`` of tests/occupancy_reference.py -- the canonical statement -- so that this script runs on its own."""
    ka = np.unique(np.floor(np.asarray(a, np.float64) / v) + 0.0, axis=0)
    kb = np.unique(np.floor(np.asarray(b, np.float64) / v) + 0.0, axis=0)
    both = len(ka) + len(kb) - len(np.unique(np.vstack([ka, kb]), axis=0))
    return len(ka), len(kb), both


def timed(call, warmup, steps):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(ts)), 4), round(1e3 * float(np.min(ts)), 4)


def occupancy_cost(args):
    out = {"steps": args.steps, "warmup": args.warmup}
    pairs = {"uniform_1M": (synth(1_000_000)[:2], (1.0 / 64,), (1.0 / 256, 1.0 / 64, 1.0 / 16, 1.0 / 4)),
             "content_0.8M": (synth_content(), (1.0,), (1.0, 2.0, 4.0, 8.0))}
    for name, ((a, b), one, four) in pairs.items():
        eng = nat.Engine(0)
        try:
            eng.set_cloud(0, a)
            eng.set_cloud(1, b)
            eng.sync()
            got = eng.voxel_occupancy(list(four))
            want = [numpy_occupancy(a, b, v) for v in four]
            rec = {"points": [len(a), len(b)], "voxels": list(four), "counts": [list(t) for t in got], "equals_numpy": got == want}
            rec["one_size_ms"], rec["one_size_ms_min"] = timed(lambda: eng.voxel_occupancy(list(one)), args.warmup, args.steps)
            rec["four_sizes_ms"], rec["four_sizes_ms_min"] = timed(lambda: eng.voxel_occupancy(list(four)), args.warmup, args.steps)
            eng.profile(True)                                        # GPU time of the launches alone, from the library's events
            eng.profile_reset()
            for _ in range(args.steps):
                eng.voxel_occupancy(list(one))
            ms, launches = eng.profile_get("point")
            eng.profile(False)
            rec["one_size_gpu_ms"] = round(ms / args.steps, 4)
            out[name] = rec
        finally:
            eng.close()
    return out


def merge_cost(args):
    rng = np.random.default_rng(3)
    uniq = rng.random((900_000, 3), dtype=np.float32)
    pts = np.concatenate([uniq, uniq[rng.integers(0, len(uniq), 100_000)]])[rng.permutation(1_000_000)]
    eng = nat.Engine(0)
    ts = []
    try:
        for s in range(args.warmup + args.steps):
            eng.set_cloud(0, pts)
            eng.sync()
            t0 = time.perf_counter()
            n_new = eng.merge_duplicates(0, "drop")
            dt = time.perf_counter() - t0
            if s >= args.warmup:
                ts.append(dt)
        eng.profile(True)                                            # the merge's own launches, from the library's events
        gpu = []
        for _ in range(args.steps):
            eng.set_cloud(0, pts)
            eng.sync()
            eng.profile_reset()
            eng.merge_duplicates(0, "drop")
            gpu.append(eng.profile_get("point")[0])
        eng.profile(False)
    finally:
        eng.close()
    return {"library": os.environ.get("PCCM_LIB") or "in-tree", "rows": len(pts), "rows_after": int(n_new), "steps": args.steps,
            "merge_ms": round(1e3 * float(np.median(ts)), 4), "merge_ms_min": round(1e3 * float(np.min(ts)), 4),
            "merge_ms_max": round(1e3 * float(np.max(ts)), 4), "merge_launches_gpu_ms": round(float(np.median(gpu)), 4),
            "merge_launches_gpu_ms_min": round(float(np.min(gpu)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--merge", action="store_true", help="time pccm_merge_duplicates on a 1M-row cloud with 10 % duplicates instead")
    args = ap.parse_args()
    print(json.dumps(merge_cost(args) if args.merge else occupancy_cost(args)))


if __name__ == "__main__":
    main()
