"""Variant coverage: every row of the variant table (tests/variant_rows.py) reaches the kernel instantiations it names --
pccm_nn_path says which ran -- and gives the oracle's rows, distances, projections and NumPy's reductions bit for bit.
Rows that only a switch reaches run in a child process per switch set (the library latches its switches once per process)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import variant_rows as vr  # noqa: E402

pytestmark = pytest.mark.gpu


def _report(res):
    assert not res["fail"], f"row {res['row']}: " + " | ".join(res["fail"])


@pytest.mark.parametrize("rid", [rid for rid, r in vr.ROWS.items() if not r["env"]])
def test_variant_row(rid):
    import variants_check
    _report(variants_check.run_row(rid))


@pytest.mark.parametrize("env", [e for e in vr.ENVS if e])
def test_variant_rows_under_switches(env):
    rows = [rid for rid, r in vr.ROWS.items() if r["env"] == env]
    child = dict(os.environ)
    child.update(vr.ENVS[env])
    out = subprocess.run([sys.executable, os.path.join(HERE, "variants_check.py")] + rows, env=child, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    results = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    assert [res["row"] for res in results] == rows
    for res in results:
        _report(res)
