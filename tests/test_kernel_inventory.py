"""Host-only guard of the variant table (tests/variant_rows.py): every kernel instantiation of the built product library is
named there -- by the row of tests/test_gpu_variants.py that reaches it, or with the reason no row can -- and every name
there is a kernel of the library.  A new instantiation, or a row taken out, fails here on a CPU-only box.  And no test sets
one of the library's switches in-process: the library latches them on first use, so such a setting silently does nothing."""
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "open_pcc_metric_amd", "csrc")
sys.path.insert(0, HERE)
import variant_rows as vr  # noqa: E402

# the families whose variant the library picks from the data or a switch: each instantiation needs a row or a reason
SELECTABLE = ("k_brick_query<", "k_grid_query<", "k_grid_query_coop<", "k_grid_tail<", "k1_scan<", "k2_refine<", "k2b_fallback<",
              "k_vox_query<", "k_lattice_query<", "k_unit_lean<", "k_unit_jobs", "k_tie_mean<", "k_tie_exposure<")


def _strip(name):
    """'void pccm::__device_stub__k_x<a, b>(args)' -> 'k_x<a, b>' (how pccm_nn_path names kernels)."""
    name = re.sub(r"^void ", "", name).replace("pccm::__device_stub__", "", 1)
    depth = 0
    for i, c in enumerate(name):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            return name[:i]
    return name


def product_kernels():
    lib = os.path.join(CSRC, "libpccm.so")
    if not os.path.exists(lib):
        pytest.fail("libpccm.so is not built")
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-C", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        parts = line.split(" ", 2)
        if len(parts) == 3 and "__device_stub__" in parts[2]:
            names.add(_strip(parts[2]))
    return names


def test_every_instantiation_is_in_the_variant_table():
    kernels = product_kernels()
    assert len(kernels) >= 100
    by_row = {k for r in vr.ROWS.values() for k in r["expect"]}
    named = by_row | set(vr.UNREACHABLE) | set(vr.OTHER)
    assert sorted(kernels - named) == [], "kernels of libpccm.so the variant table does not name"
    assert sorted(named - kernels) == [], "names in the variant table that are no kernel of libpccm.so"
    selectable = {k for k in kernels if k.startswith(SELECTABLE)}
    assert sorted(k for k in selectable if k not in by_row and k not in vr.UNREACHABLE) == [], \
        "selectable variants need a row of tests/test_gpu_variants.py or a reason in UNREACHABLE"
    assert not set(vr.OTHER) & selectable
    assert not set(vr.UNREACHABLE) & by_row
    for k, reason in list(vr.UNREACHABLE.items()) + list(vr.OTHER.items()):
        assert len(reason) > 10, k


def test_rows_are_well_formed():
    for rid, r in vr.ROWS.items():
        assert r["kind"] in ("brick", "search", "ties", "reduce"), rid
        assert r["env"] in vr.ENVS and r["expect"], rid
    for env in vr.ENVS.values():
        assert all(k.startswith("PCCM_") for k in env)


def library_switches():
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        names |= set(re.findall(r'(?:getenv|PCCM_DIAG_ENV)\("(PCCM_[A-Z0-9_]+)"\)', open(path).read()))
    return names


def test_no_test_sets_a_switch_in_process():
    switches = library_switches()
    assert {"PCCM_GRID_COOP", "PCCM_BRICK", "PCCM_BRICK_CAP", "PCCM_NO_FUSE"} <= switches
    offenders = []
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        for no, line in enumerate(open(path), 1):
            for m in re.finditer(r'(?:setenv|putenv)\(\s*["\'](PCCM_[A-Z0-9_]+)["\']|os\.environ\[\s*["\'](PCCM_[A-Z0-9_]+)["\']\s*\]\s*=(?!=)',
                                 line):
                name = m.group(1) or m.group(2)
                if name in switches:
                    offenders.append(f"{os.path.basename(path)}:{no}: {name}")
    assert offenders == [], "switches are latched once per process: set them in a child's environment instead"
