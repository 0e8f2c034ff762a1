"""The voxel-brick search (k_vox_bricks -> k_vox_list -> k_vox_query<SELF, ROWS>, open_pcc_metric_amd/csrc/pccm_vox.hip) and the
per-thread lattice search (k_lattice_query<SELF>, pccm_lattice.hip) on the planted integer families of tests/vox_reference.py,
against its int64 brute force and the answers known by construction, bit for bit:

  A  every offset (dy, dz, dx) with 0 < |v|^2 <= 81 once, from in-cell (0, 0, 0), (7, 7, 7) and a random offset: every entry of
     c_vox_rows, targets next to the sentinel bits, the d2 = 64 / 65 hand-off, a grid of more than 262144 cells (k_vox_list
     with several words per thread);
  B  2, 11, 12, 13 and r3(d2) equidistant nearest voxels at distances out of c_vox_near and out of the sqrtf walk, every vector
     the winner and a loser: the tie list's boundary, the smallest-row rule;
  C  every voxel at or beyond d2 within Chebyshev radius 8, the farther ones with the smaller rows: a spurious table entry or a
     wrong dx picks a wrong row;
  D  1, 2, 3 and 70 points per voxel at scattered rows (minrow and its rank); a cloud against itself with 1 .. 3 points per
     voxel (s_dup);
  E  three crowded cells: 4608 records in a tile (the pieces of k_vox_bricks), 1536 queries per cell (the qb loop);
  F  the 26 directions from the corner, edge and face cells of a grid, grids of 1, 2 and 45 cells, negative coordinates.

Beyond the results, the split of work is pinned: nn_stats()["tail_queries"] of every search equals the count the reference
predicts (d2 > 64; with rows also more than 12 equidistant voxels), 0 included -- the tail kernels compute the same answers, so
nothing else notices a brick kernel that hands them what it should keep.  nn_stats()["splits"] holds every family on the grid
of 8-voxel cells.  tests/vox_planted_check.py runs the lattice kernel on the same families in a child with PCCM_VOX=0."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vox_planted_check as vpc  # noqa: E402
import vox_reference as vr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from open_pcc_metric_amd import _native as nat
    e = nat.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", vr.NAMES)
def test_planted_family_on_the_bricks(eng, name):
    c = vpc.check_bricks(eng, vr.family(name))
    print(json.dumps({name: c.figures}))
    assert c.fail == []


def test_family_a_through_the_lattice_kernel_in_process(eng):
    """A second, far blob (the `spread` trick of variant_rows.make_pair) gives a box the bricks do not cover."""
    c = vpc.check_lattice(eng, vr.far_blob(vr.family("A")))
    print(json.dumps({"A_spread": c.figures}))
    assert c.fail == []


def test_planted_families_on_the_lattice_kernel():
    """Families A, B, D and F with the voxel bricks switched off: one child process (the library latches PCCM_VOX on first use)."""
    child = dict(os.environ)
    child["PCCM_VOX"] = "0"
    out = subprocess.run([sys.executable, os.path.join(HERE, "vox_planted_check.py")], env=child, capture_output=True, text=True, timeout=600)
    assert out.returncode in (0, 1), out.stdout[-2000:] + out.stderr[-4000:]
    report = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(report["families"]))
    assert sorted(report["families"]) == sorted(vpc.LATTICE_FAMILIES)
    assert report["fail"] == []
