"""What a grid build leaves behind (open_pcc_metric_amd/csrc/pccm_gridbuild.hip: k_bin_count, k_bin_scatter, k_bin_sort,
k_scan_lookback), structure by structure: cell starts, records and occupancy bitmaps of both clouds, the cell-sorted query
lists of sharded directions, the spatial orders -- read back through pccm_build_plan / pccm_build_fetch and held to the exact
integer and bitwise contract of tests/gridbuild_reference.py (tests/test_gridbuild_host.py shows that contract rejects the ways
a counting sort goes wrong).  The rows and their preconditions are in tests/gridbuild_check.py; rows that only a switch reaches
run in a child process per switch set, one after another (the library latches its switches once per process)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

# (kept in step with gridbuild_check.ROWS, which needs the library to import: test_rows_are_all_run checks it)
IN_PROCESS = ["quads_f32", "quads_f64", "tiles_f32", "tiles_f64", "faces", "trimmed", "streamed", "planted_bins", "bitmaps",
              "spatial_4095", "spatial_4096", "spatial_20011", "shards_f32", "shards_f64", "solo", "rebuilds", "degenerate", "validity"]
SWITCHED = {"tile256": ["tile256"], "scan_tile256": ["scan"], "threads256": ["threads256"]}


def _report(res):
    assert not res["fail"], f"row {res['row']}: " + " | ".join(res["fail"][:12])


def test_rows_are_all_run():
    import gridbuild_check as gc
    assert sorted(IN_PROCESS) == sorted(rid for rid, (env, _) in gc.ROWS.items() if not env)
    assert {env: sorted(rows) for env, rows in SWITCHED.items()} == \
        {env: sorted(rid for rid, (e, _) in gc.ROWS.items() if e == env) for env in gc.ENVS if env}


@pytest.mark.parametrize("rid", IN_PROCESS)
def test_gridbuild_row(rid):
    import gridbuild_check as gc
    _report(gc.run_row(rid))


@pytest.mark.parametrize("env", sorted(SWITCHED))
def test_gridbuild_rows_under_switches(env):
    import gridbuild_check as gc
    rows = SWITCHED[env]
    child = dict(os.environ)
    child.update(gc.ENVS[env])
    out = subprocess.run([sys.executable, os.path.join(HERE, "gridbuild_check.py")] + rows, env=child, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    results = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    assert [res["row"] for res in results] == rows
    for res in results:
        _report(res)
