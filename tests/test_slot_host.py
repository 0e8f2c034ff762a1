"""A reduction slot's shape, host layout and summation order without a GPU: tests/slot_host_main.cpp shards a column as
shard_of does, fills every rank's host buffer through SlotView with what the reduction kernels leave there (pairwise leaf sums,
half-chunk trees, raw tail values, a NaN where nothing may be read) and prints what the consumers of
open_pcc_metric_amd/csrc/pccm_slot.h make of it: slot_total, and the per-chunk and per-leaf exchange vectors summed over the
ranks and finished by pccm_finish_chunks / pccm_finish_sum.  Every printed sum, minimum and maximum must have the bits of
np.sum, np.min, np.max of the column, computed here.  The program is built with the host sanitizers, linked against libpccm.so
for the public finishers, and run as a process of its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_pcc_metric_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
SIZES = [1, 7, 8, 127, 128, 129, 8191, 8192, 8193, 16384, 16389, 28673]      # 28673 = 3 chunks + more than half a chunk
WORLDS = [1, 2, 3, 4, 7]


@pytest.fixture(scope="module")
def slot_host(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc is not installed")
    exe = str(tmp_path_factory.mktemp("slot_host") / "slot_host")
    build = subprocess.run(
        [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
         "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "slot_host_main.cpp"), "-x", "none",
         "-L", CSRC, "-lpccm", "-Wl,-rpath," + CSRC, "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def _bits(x):
    return "%016x" % int(np.float64(x).view(np.uint64))


def _squares(n):
    """squares of normals scaled over sixteen binades: a sloppy order of addition shows in the last bit"""
    rng = np.random.default_rng(1000 + n)
    return rng.standard_normal(n) ** 2 * 2.0 ** rng.integers(-8, 8, n)


def _zeros(n):
    """a -0.0 among exact zeros and squares (a signed projection column holds both zeros); from two rows on a negative value, so
    that the minimum is no zero whose sign NumPy's own order of comparison decides"""
    col = np.where(np.arange(n) % 3 == 0, _squares(n), 0.0)
    col[n // 2] = -0.0
    if n > 1:
        col[n - 1] = -0.75
    return col


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("column", [_squares, _zeros])
def test_consumers_reproduce_numpy_bit_for_bit(slot_host, tmp_path, column, n):
    col = np.ascontiguousarray(column(n), dtype="<f8")
    assert col.shape == (n,)
    path = tmp_path / "column.f64"
    col.tofile(path)
    run = subprocess.run([slot_host, str(path), str(n)] + [str(w) for w in WORLDS], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert " checks, 0 failed" in run.stdout
    want_sum, want_min, want_max = _bits(np.sum(col)), _bits(np.min(col)), _bits(np.max(col))
    got = {}
    for line in run.stdout.splitlines():
        f = line.split()
        if f and f[0] == "world":
            got[(int(f[1]), f[2])] = f[3:]
    for world in WORLDS:
        # whole chunks for every rank when there are enough of them, or one rank owns the whole column (one rank, or one leaf)
        aligned = n >= world * 8192 or world == 1 or n <= 128
        assert got[(world, "aligned")] == ["1" if aligned else "0"]
        assert ((world, "total") in got) == (world == 1)
        assert ((world, "chunks") in got) == aligned
        if world == 1:
            assert got[(world, "total")] == [want_sum, want_min, want_max], (n, world)
        if aligned:
            assert got[(world, "chunks")] == [want_sum], (n, world)
        assert got[(world, "leaves")] == [want_sum], (n, world)
        assert got[(world, "minmax")] == [want_min, want_max], (n, world)
    if n == 28673:
        assert [w for w in WORLDS if (w, "chunks") in got] == [1, 2, 3]
