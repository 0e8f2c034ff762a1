"""How the wait of a report (pccm_set_wait) shows in the headline step (GPU box): the replayed 1M + 1M step of bench.py, timed in
rounds that alternate the wait modes in one process, plus where the host's time goes around the report's one blocking call.

    python scripts/dev_wait_modes.py                      # spin (the completion counter) against event (hipEventSynchronize)
    PCCM_LIB=<make DIAG=1 BUILD=dir>/libpccm.so python scripts/dev_wait_modes.py
                                                          # ... and a hipEventQuery spin (mode 2, diagnostic builds only)"""
import gc
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from open_pcc_metric_amd import _native as nat, metric as m
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud

n = int(os.environ.get("N", 1000000))
K = int(os.environ.get("STEPS", 300))
a, b, na, nb = bench.synth(n)
pair = CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0], use_graph=True)
eng = pair._engine
options = CalculateOptions(color=None, hausdorff=False, point_to_plane=True)
modes = {"spin": 0, "event": 1}
if eng._lib.pccm_set_wait(eng._ctx, 2) == 0:
    modes["query"] = 2
stamps = {}
orig = type(eng).reduce_total_many


def wrapped(self, *a, **k):
    stamps["call"] = time.perf_counter()
    r = orig(self, *a, **k)
    stamps["ret"] = time.perf_counter()
    return r


type(eng).reduce_total_many = wrapped


def metrics():
    return transform_options(options)[2:] + [m.GeoHausdorffDistance(True, False), m.GeoHausdorffDistance(False, False)]


def step():
    pair.recompute()
    return MetricCalculator(pair).calculate(metrics()).as_dict()


for _ in range(6):
    ref = step()
gc.collect()
gc.freeze()
res = {k: [] for k in modes}
for rnd in range(3):
    for name, mode in modes.items():
        nat._check(eng._lib.pccm_set_wait(eng._ctx, mode))
        eng.sync()
        pre = wait = post = 0.0
        T0 = time.perf_counter()
        for _ in range(K):
            t0 = time.perf_counter()
            out = step()
            t1 = time.perf_counter()
            pre += stamps["call"] - t0
            wait += stamps["ret"] - stamps["call"]
            post += t1 - stamps["ret"]
        eng.sync()
        tot = (time.perf_counter() - T0) / K
        assert repr(out) == repr(ref), name
        res[name].append((tot * 1e6, pre / K * 1e6, wait / K * 1e6, post / K * 1e6))
for name, rows in res.items():
    med = [statistics.median(r[i] for r in rows) for i in range(4)]
    print(f"RESULT n {n} wait {name:5s}: step {med[0]:6.1f} us = before the blocking call {med[1]:5.1f} + inside it {med[2]:5.1f} + after it "
          f"{med[3]:5.1f}   (rounds: {', '.join(f'{r[0]:.1f}' for r in rows)})")
