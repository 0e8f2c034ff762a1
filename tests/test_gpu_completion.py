"""Reductions wait on the context's completion counter (pccm_set_wait, include/pccm.h): the last k_unit_lean of a batch bumps a
word in host-coherent memory once the batch's numbers are on the host, and the caller spins on it instead of sleeping in
hipEventSynchronize.  Both wait modes must give the reports the oracle gives, the counter must move exactly once per batch,
eager or replayed, contexts on different threads must not see each other's counters, and the device error word must still
surface in spin mode."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import same_bits
from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud
from oracle import oracle as orc
from test_gpu_device_errors import CHILD as ERROR_CHILD
from test_gpu_parity import clouds, unit_normals

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = CalculateOptions(None, True, True)


def report(p):
    return MetricCalculator(p).calculate(transform_options(OPTS)).as_dict()


def check(got, want):
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert same_bits(got[k], want[k]), (k, got[k], want[k])


@pytest.fixture(scope="module")
def pair_data():
    n = 100_000
    a, b = clouds("uniform32", n, n, seed=21)
    na, nb = unit_normals(n, 5), unit_normals(n, 6)
    want = orc.OraclePair(a, b, na, nb, method="kdtree").report(hausdorff=True, point_to_plane_=True, peak=1.0)
    return a, b, na, nb, want


@pytest.mark.parametrize("mode", ["spin", "event"])
def test_wait_modes_give_the_oracle_rows(pair_data, mode):
    a, b, na, nb, want = pair_data
    rows = []
    with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0], use_graph=True) as p:
        p._engine.set_wait(mode)
        for _ in range(53):                                 # eager, capture, first replay, then 50 replays
            p.recompute()
            rows.append(report(p))
    with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0], use_graph=False) as p:
        p._engine.set_wait(mode)
        for _ in range(10):
            p.recompute()
            rows.append(report(p))
    for r in rows:
        check(r, want)


def test_bad_wait_mode_is_refused():
    e = nat.Engine(0)
    with pytest.raises(ValueError):
        e.set_wait("sleep")
    assert e._lib.pccm_set_wait(e._ctx, 7) != 0


@pytest.mark.parametrize("mode", ["spin", "event"])
def test_counter_moves_once_per_batch(pair_data, mode):
    a, b, na, nb, _ = pair_data
    e = nat.Engine(0)
    e.set_wait(mode)
    e.set_cloud(0, a)
    e.set_cloud(1, b)
    e.set_normals(0, na)
    e.set_normals(1, nb)
    req = [(nat.DIR_LEFT, nat.METRIC_D1), (nat.DIR_RIGHT, nat.METRIC_D1), (nat.DIR_LEFT, nat.METRIC_D2), (nat.DIR_RIGHT, nat.METRIC_D2)]
    eager = []
    for _ in range(3):                                      # eager batches
        e.drop_caches()
        e.nn_pair("grid")
        c0 = e.wait_counter()
        e.reduce_prefetch_many(req)
        eager.append(e.reduce_total_many(req))
        e.sync()
        assert e.wait_counter() == c0 + 1
    e.graph_begin()                                         # one batch captured; graph_end runs the graph once
    e.drop_caches()
    e.nn_pair("grid")
    e.reduce_prefetch_many(req)
    c0 = e.wait_counter()
    gid = e.graph_end()
    got = e.reduce_total_many(req)
    e.sync()
    assert e.wait_counter() == c0 + 1
    for k in range(10):                                     # replays
        c0 = e.wait_counter()
        e.graph_launch(gid)
        got = e.reduce_total_many(req)
        e.sync()
        assert e.wait_counter() == c0 + 1, k
        for g, w in zip(got, eager[0]):
            assert same_bits(np.array(g), np.array(w))
    e.graph_destroy(gid)


def test_two_contexts_on_two_threads(pair_data):
    a, b, na, nb, want0 = pair_data
    c, d = clouds("surface", 50_000, 40_000, seed=4)
    nc, nd = unit_normals(len(c), 3), unit_normals(len(d), 4)
    want1 = orc.OraclePair(c, d, nc, nd, method="kdtree", normal_index="neighbour").report(hausdorff=True, point_to_plane_=True, peak=1.0)
    with CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0], use_graph=True) as p0, \
            CloudPair(PointCloud(c, nc), PointCloud(d, nd), extent=[1.0, 1.0, 1.0], normal_index="neighbour", use_graph=True) as p1:
        start = threading.Barrier(2)
        got, errors = {0: [], 1: []}, []

        def run(k, p):
            try:
                start.wait()
                for _ in range(25):
                    p.recompute()
                    got[k].append(report(p))
            except BaseException as exc:                    # reported by the main thread
                errors.append(exc)

        th = [threading.Thread(target=run, args=(k, p)) for k, p in ((0, p0), (1, p1))]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not any(t.is_alive() for t in th)
        assert not errors, errors
        assert len(got[0]) == len(got[1]) == 25
        for k, want in ((0, want0), (1, want1)):
            for r in got[k]:
                check(r, want)


def test_device_error_surfaces_in_spin_mode(tmp_path):
    """tests/test_gpu_device_errors.py with the spin wait asked for explicitly."""
    build = tmp_path / "diag"
    make = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "open_pcc_metric_amd", "csrc"), "-j8", "DIAG=1", f"BUILD={build}"],
                          capture_output=True, text=True, timeout=900)
    assert make.returncode == 0, make.stdout[-2000:] + make.stderr[-2000:]
    child = ERROR_CHILD.replace("e = nat.Engine(0)\n", "e = nat.Engine(0)\ne.set_wait('spin')\n")
    assert "set_wait('spin')" in child
    script = tmp_path / "child.py"
    script.write_text(child)
    env = dict(os.environ, PCCM_ROOT=ROOT, PCCM_LIB=str(build / "libpccm.so"), PCCM_DIAG_CORRUPT_CS="1", PCCM_NO_TORCH="1")
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "STATE ERROR:" in out.stdout and "device error word" in out.stdout, out.stdout
    assert "RECOVERED True" in out.stdout, out.stdout
