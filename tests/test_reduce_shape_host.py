"""Which reduction kernel takes a job, without a GPU: tests/reduce_shape_host_main.cpp walks every layout a UnitJob can name
(576 jobs) through open_pcc_metric_amd/csrc/pccm_reduce_shape.h and prints the k_unit_lean shape the header picks, or `general`.
tests/golden/reduce_dispatch.txt is what job_shape() and lean_has() of pccm_point.hip answered for the same jobs before the
header replaced them (recorded from those two functions as they stood, not from the header).  The program is built with the
host sanitizers and run as a process of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
def test_every_job_goes_to_the_kernel_it_went_to_before(tmp_path):
    exe = str(tmp_path / "reduce_shape_host")
    build = subprocess.run(
        [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "open_pcc_metric_amd", "csrc"),
         os.path.join(ROOT, "tests", "reduce_shape_host_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    with open(os.path.join(ROOT, "tests", "golden", "reduce_dispatch.txt")) as f:
        want = f.read().splitlines()
    got = run.stdout.splitlines()
    assert len(want) == 576 and len(got) == 576
    differ = [(g, w) for g, w in zip(got, want) if g != w]
    assert not differ, differ[:8]
    lean = {g.split(": ")[1] for g in got} - {"general"}
    assert len(lean) == 18, sorted(lean)
