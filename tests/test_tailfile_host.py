"""The filed tails' capture rule without a GPU: tests/tailfile_host_main.cpp includes the host half of
open_pcc_metric_amd/csrc/pccm_tail_wave.h (the binning of a tail list by blocks of 4096 rows, tail_filing_allowed), is built with the
host sanitizers and run as a process of its own.  The defensive device error (a block list that overflows) is reachable only through
this rule: no test runs a kernel in a state known to overflow."""
import os
import re
import shutil
import subprocess

import pytest

from open_pcc_metric_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_pcc_metric_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def test_binning_and_capture_rule(tmp_path):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "tailfile_host")
    build = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "tailfile_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert re.search(r"tailfile host ok: \d{3,} checks", run.stdout), run.stdout[-2000:]


def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "pccm.h")).read()
    assert re.search(r"int pccm_set_tail_filing\(pccm_ctx \*ctx, int on\);", header)
    assert re.search(r"int pccm_graph_tail_filed\(pccm_ctx \*ctx, int graph_id, int \*filed\);", header)
    for name in ("pccm_set_tail_filing", "pccm_graph_tail_filed"):
        assert name in nat.SYMBOLS
    assert hasattr(nat.Engine, "set_tail_filing") and hasattr(nat.Engine, "graph_tail_filed")
