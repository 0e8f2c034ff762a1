"""The invalidation events of open_pcc_metric_amd/csrc/pccm_stale.h without a GPU: tests/stale_host_main.cpp makes a context
with every product valid, applies one event and checks product by product what may still claim validity ("What goes
stale when").  The program is built with the host sanitizers and run as a process of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
def test_every_event_leaves_each_product_as_the_table_says(tmp_path):
    exe = str(tmp_path / "stale_host")
    build = subprocess.run(
        [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "open_pcc_metric_amd", "csrc"),
         os.path.join(ROOT, "tests", "stale_host_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert " checks, 0 failed" in run.stdout
