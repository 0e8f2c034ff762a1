"""The planted integer families of tests/vox_reference.py on the GPU.  tests/test_gpu_vox_planted.py calls check_bricks() and
check_lattice() in-process, and runs this file in one child process with PCCM_VOX=0 in the child's environment (the library
latches its switches once per process), which sends families A, B, D and F through the per-thread lattice kernel:
`python tests/vox_planted_check.py` prints one JSON line {"fail": [...], "families": {...}}.

Everything is exact integer arithmetic: distances, rows and error vectors are compared bit for bit, and the counters
(pccm_nn_stats: tail_queries of the voxel-brick kernel, fallback_queries of the lattice kernel) with the counts the reference
predicts -- a kernel that hands work it should keep to the kernels behind it computes the same answers and fails here."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from open_pcc_metric_amd import _native as nat  # noqa: E402
import vox_reference as vr  # noqa: E402

LATTICE_FAMILIES = ("A", "B", "D", "Dself") + tuple(vr.F_CASES)


class Checks:
    def __init__(self, name):
        self.name, self.fail, self.figures = name, [], {}

    def check(self, ok, what):
        if not ok:
            self.fail.append(f"{self.name}: {what}")

    def equal(self, got, want, what):
        got, want = np.asarray(got), np.asarray(want)
        ok = got.shape == want.shape and np.array_equal(got, want)
        bad = int(np.sum(got != want)) if got.shape == want.shape else -1
        first = int(np.flatnonzero(got != want)[0]) if bad > 0 else -1
        self.check(ok, f"{what}: {bad} of {want.size} differ" + (f", first at {first}: {got.reshape(-1)[first]} for {want.reshape(-1)[first]}" if bad > 0 else ""))


def _results(c, eng, fam, direction, rows, what):
    """d2 (and, with rows, the matched rows and the error vectors) of a direction against the reference, bit for bit."""
    want_row, want_d2, _ = fam.reference(direction)
    it, se = fam.cloud(direction)
    idx, d2 = eng.fetch_nn(direction, want_idx=rows)
    c.equal(d2, want_d2.astype(np.float64), f"{what}: d2 of direction {direction}")
    if direction == 0 and fam.d2 is not None:              # the answer by construction, where the generator knows it
        known = fam.d2 >= 0
        c.equal(d2[known], fam.d2[known].astype(np.float64), f"{what}: d2 by construction")
    if rows:
        c.equal(idx, want_row.astype(np.int32), f"{what}: rows of direction {direction}")
        if direction == 0 and fam.row is not None:
            known = fam.row >= 0
            c.equal(idx[known], fam.row[known].astype(np.int32), f"{what}: rows by construction")
        err = eng.error_vectors(direction)
        c.equal(err, it.astype(np.float64) - se.astype(np.float64)[want_row], f"{what}: error vectors of direction {direction}")


def check_bricks(eng, fam):
    """The four searches of a voxelised pair: distances only (k_vox_query<false, false>), the self search (<true, false>), with matched
    rows (<false, true>), and the self search with rows (k_lattice_query<true>).  -> Checks (fail: what went wrong; figures)."""
    c = Checks(fam.name)
    eng.set_cloud(0, fam.queries)
    eng.set_cloud(1, fam.searched)
    ref = {d: fam.reference(d) for d in (0, 1, 2)}
    want_tail = {(d, rows): int(vr.predicted_tail(ref[d][1], ref[d][2], rows).sum()) for d in (0, 1, 2) for rows in (False, True)}
    c.figures["sizes"] = [len(fam.queries), len(fam.searched)]
    c.figures["cells"] = fam.ncells()

    def search(what, dirs, kernel, rows):
        for d in dirs:
            path = eng.last_path(d)
            c.check(kernel in path, f"{what}: direction {d} ran {path}, not {kernel}")
            stats = eng.nn_stats(d)
            c.figures[f"tail {kernel} dir {d}"] = [want_tail[(d, rows)], stats["tail_queries"]]
            c.check(stats["tail_queries"] == want_tail[(d, rows)],
                    f"{what}: direction {d}: {stats['tail_queries']} queries went to the tail kernels, the reference predicts {want_tail[(d, rows)]}")
            c.check(stats["splits"] == fam.ncells(), f"{what}: direction {d} ran on a grid of {stats['splits']} cells, not the {fam.ncells()} of 8-voxel cells")

    # 1. distances only
    eng.nn_want_idx(False)
    eng.drop_caches()
    eng.nn_pair("grid")
    org, h, dim = eng.grid_geometry()
    c.check(np.array_equal(h, [8.0] * 3) and np.array_equal(org, fam.org) and np.array_equal(dim, fam.dims),
            f"grid {org} / {h} / {dim}, planned {fam.org} / 8 / {fam.dims}")
    if fam.offsets is not None:
        c.equal(fam.realised_offsets(org), fam.offsets, "in-cell offsets of the queries on the library's grid")
    search("distances only", (0, 1), "k_vox_query<false, false>", False)
    for d in (0, 1):
        _results(c, eng, fam, d, False, "distances only")
    # 2. the self search
    eng.nn(2, "grid")
    search("self search", (2,), "k_vox_query<true, false>", False)
    _results(c, eng, fam, 2, False, "self search")
    # 3. matched rows
    eng.nn_want_idx(True)
    eng.drop_caches()
    eng.nn_pair("grid")
    search("matched rows", (0, 1), "k_vox_query<false, true>", True)
    for d in (0, 1):
        _results(c, eng, fam, d, True, "matched rows")
    # 4. the self search with rows: distances on the bricks again, the rows through the lattice kernel
    eng.nn(2, "grid")
    search("self search before its rows", (2,), "k_vox_query<true, false>", False)
    _results(c, eng, fam, 2, True, "self search with rows")
    path = eng.last_path(2)
    c.check("k_lattice_query<true>" in path, f"self search with rows ran {path}, not k_lattice_query<true>")
    return c


def check_lattice(eng, fam):
    """A pair the voxel bricks do not serve (PCCM_VOX=0, or a box they do not cover): k_lattice_query<false> / <true>, results equal
    to the reference, and as many exact rescans as the reference has queries with nothing within kMaxRing cells of the grid."""
    c = Checks(fam.name)
    eng.set_cloud(0, fam.queries)
    eng.set_cloud(1, fam.searched)
    c.figures["sizes"] = [len(fam.queries), len(fam.searched)]
    eng.nn_want_idx(True)
    eng.drop_caches()
    for dirs, kernel in (((0, 1), "k_lattice_query<false>"), ((2,), "k_lattice_query<true>")):
        if dirs == (2,):
            eng.nn(2, "grid")
        else:
            eng.nn_pair("grid")
        org, h, dim = eng.grid_geometry()
        c.figures[f"grid {kernel}"] = [dim.tolist(), h.tolist()]
        for d in dirs:
            path = eng.last_path(d)
            c.check(kernel in path and not any(k.startswith("k_vox_query") for k in path), f"direction {d} ran {path}, not {kernel}")
            it, _ = fam.cloud(d)
            want = int(vr.lattice_fallback(it, fam.reference(d)[1], org, h, dim).sum())
            got = eng.nn_stats(d)["fallback_queries"]
            c.figures[f"fallback {kernel} dir {d}"] = [want, got]
            c.check(got == want, f"direction {d}: {got} exact rescans, the reference has {want} queries with nothing within {vr.MAX_RING} cells")
            _results(c, eng, fam, d, True, kernel)
    return c


def main():
    fail, families = [], {}
    eng = nat.Engine(0)
    try:
        for name in LATTICE_FAMILIES:
            c = check_lattice(eng, vr.family(name))
            fail += c.fail
            families[name] = c.figures
    finally:
        eng.close()
    print(json.dumps({"fail": fail, "families": families}), flush=True)
    return 1 if fail else 0


if __name__ == "__main__":
    sys.exit(main())
