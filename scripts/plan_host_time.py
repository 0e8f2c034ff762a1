"""Host time of one timed step's Python -- ``recompute()`` plus ``MetricCalculator(pair)._plan(...)`` -- on the recording stand-in
of tests/plan_trace.py with recording switched off, for the headline report and the report with every option: best of five runs
of ``--steps`` steps, after a warm-up and ``gc.freeze()``.  The figures include the stand-in's own overhead; compare two commits
in one session.   python scripts/plan_host_time.py [--steps 500]"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import plan_trace  # noqa: E402
from open_pcc_metric_amd.calculator import MetricCalculator  # noqa: E402


def ms_per_step(report, steps):
    pair = plan_trace.make_pair(plan_trace.RecordingEngine(record=False), use_graph=True)
    metrics = plan_trace.metrics_of(report)

    def step():
        pair.recompute()
        MetricCalculator(pair)._plan(metrics)
    for _ in range(50):
        step()
    gc.collect()
    gc.freeze()
    best = float("inf")
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        best = min(best, (time.perf_counter() - t0) / steps)
    gc.unfreeze()
    return best * 1e3


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--steps", type=int, default=500)
    args = parser.parse_args()
    print(json.dumps({report: round(ms_per_step(report, args.steps), 5) for report in ("headline", "every")}))
