"""Host-only checks of tests/gridbuild_reference.py, the contract tests/test_gpu_gridbuild.py holds the grid build to: a
structure built with a stable argsort passes, so does every permutation inside the cells, and each planted corruption -- the ways
a counting sort goes subtly wrong -- is rejected with a message that names it.  This is what shows the GPU test would fail for
a wrong kernel; no broken kernel ever runs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gridbuild_reference as gr  # noqa: E402


def _geometry(dim=(9, 7, 8), org=(-0.25, 0.0, 0.125), h=(0.2, 0.21, 0.17), morton=False):
    return {"org": np.array(org, np.float64), "h": np.array(h, np.float64), "dim": np.array(dim, np.int64), "morton": morton}


def _cloud(n, dtype, seed=0):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * np.array([1.3, 1.0, 0.9]) - np.array([0.25, 0.0, -0.125])
    p[::17, 0] = -0.0                       # negative zeros, to be kept bit for bit
    p[5:40] = p[4]                          # crowded cells of equal points (one inside the shard's rows)
    p[1100:1140] = p[1099]
    return p.astype(dtype)


CASES = [("f32", np.float32, 0, 3001, False), ("f64", np.float64, 0, 3001, False), ("shard", np.float32, 1024, 1500, False),
         ("bitmap", np.float32, 0, 150, True)]


def _case(name):
    _, dtype, row0, n, bitmap = next(c for c in CASES if c[0] == name)
    pts = _cloud(3001, dtype)
    g = _geometry()
    return pts, row0, n, g, gr.build_expected(pts, row0, n, g, bitmap=bitmap)


def _copy(f):
    return {k: (None if v is None else v.copy()) for k, v in f.items()}


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_a_correct_structure_passes_in_any_order_inside_the_cells(name):
    pts, row0, n, g, f = _case(name)
    assert gr.check_structure(pts, row0, n, g, f) == []
    c = gr.cells(pts[row0:row0 + n], g)
    assert len(np.unique(c)) > 20 and np.bincount(c).max() >= 30          # many cells, a crowded one, empty ones
    assert np.any(np.bincount(c, minlength=gr.ncells_of(g)) == 0)
    rng = np.random.default_rng(5)
    for _ in range(5):
        order = np.lexsort((rng.random(n), c))                             # cells sorted, a random order inside each
        assert not np.array_equal(order, np.argsort(c, kind="stable"))
        shuffled = gr.build_expected(pts, row0, n, g, order=order, bitmap=f["occ"] is not None)
        assert gr.check_structure(pts, row0, n, g, shuffled) == []


def _two_cells(f, n):
    """Positions of one record in each of two different non-empty cells."""
    cs = f["cell_start"].astype(np.int64)
    full = np.flatnonzero(np.diff(cs) > 0)
    return int(cs[full[1]]), int(cs[full[-2]])


def _named(fails, word):
    assert fails, "the corruption passed"
    assert any(word in m for m in fails), (word, fails)


@pytest.mark.parametrize("name", ["f32", "f64", "shard"])
def test_planted_corruptions_are_rejected(name):
    pts, row0, n, g, good = _case(name)
    cs = good["cell_start"].astype(np.int64)
    ncells = gr.ncells_of(g)
    # two records of different cells swapped
    f = _copy(good)
    p, q = _two_cells(good, n)
    f["rows"][[p, q]] = f["rows"][[q, p]]
    f["xyz"][[p, q]] = f["xyz"][[q, p]]
    _named(gr.check_structure(pts, row0, n, g, f), "segment")
    # a row replaced by a copy of another row of the same cell: the counts stay intact
    f = _copy(good)
    crowded = int(np.argmax(np.diff(cs)))
    p = int(cs[crowded])
    f["rows"][p] = f["rows"][p + 1]
    f["xyz"][p] = f["xyz"][p + 1]
    fails = gr.check_structure(pts, row0, n, g, f)
    _named(fails, "rows: not a permutation")
    assert not any(m.startswith(("cell_start", "segment")) for m in fails)
    # one cell_start entry off by one (of a non-empty cell, of an empty one)
    for cell in (int(np.flatnonzero(np.diff(cs) > 0)[3]), int(np.flatnonzero(np.diff(cs) == 0)[2])):
        for d in (1, -1):
            if cell == 0 or (d == -1 and cs[cell] == 0):
                continue
            f = _copy(good)
            f["cell_start"][cell] = np.uint32(int(cs[cell]) + d)
            _named(gr.check_structure(pts, row0, n, g, f), f"cell_start[{cell}]")
    # the last entry short by one
    f = _copy(good)
    f["cell_start"][ncells] -= np.uint32(1)
    _named(gr.check_structure(pts, row0, n, g, f), "cell_start[ncells]")
    # cell_start[0] not zero
    f = _copy(good)
    f["cell_start"][0] = 1
    _named(gr.check_structure(pts, row0, n, g, f), "cell_start[0]")
    # one coordinate one ulp off
    f = _copy(good)
    f["xyz"][n // 2, 1] = np.nextafter(f["xyz"][n // 2, 1], np.inf)
    _named(gr.check_structure(pts, row0, n, g, f), "xyz")
    # 0.0 stored for -0.0
    f = _copy(good)
    neg = np.flatnonzero(np.signbit(f["xyz"][:, 0]) & (f["xyz"][:, 0] == 0.0))
    assert len(neg) > 0
    f["xyz"][neg[0], 0] = 0.0
    fails = gr.check_structure(pts, row0, n, g, f)
    _named(fails, "xyz: 1 records")
    # a row from outside the job (the row just before it, just behind it)
    for r in (row0 - 1, row0 + n):
        if r < 0 or r >= len(pts):
            continue
        f = _copy(good)
        f["rows"][7] = r
        f["xyz"][7] = pts[r].astype(np.float64)
        _named(gr.check_structure(pts, row0, n, g, f), "outside the job")
    # a record lost: one fewer than the job's rows
    f = _copy(good)
    f["rows"], f["xyz"] = f["rows"][:-1], f["xyz"][:-1]
    _named(gr.check_structure(pts, row0, n, g, f), "rows:")


def test_bitmap_corruptions_are_rejected():
    pts, row0, n, g, good = _case("bitmap")
    ncells = gr.ncells_of(g)
    assert ncells % 32 != 0 and good["occ"] is not None and len(good["occ"]) == (ncells + 31) // 32
    counts = np.diff(good["cell_start"].astype(np.int64))
    full, empty = np.flatnonzero(counts > 0), np.flatnonzero(counts == 0)
    assert len(full) > 10 and len(empty) > 10
    for c in (full[0], full[-1], full[len(full) // 2]):
        f = _copy(good)
        f["occ"][c >> 5] &= ~np.uint32(1 << (c & 31))
        _named(gr.check_structure(pts, row0, n, g, f), f"bit clear for 1 occupied cells, first cell {c}")
    for c in (empty[0], empty[-1]):
        f = _copy(good)
        f["occ"][c >> 5] |= np.uint32(1 << (c & 31))
        _named(gr.check_structure(pts, row0, n, g, f), f"bit set for 1 empty cells, first cell {c}")
    # bits above ncells are nobody's business
    f = _copy(good)
    f["occ"][-1] |= np.uint32(1 << 31)
    assert ncells & 31 != 0 and gr.check_structure(pts, row0, n, g, f) == []
    # a bitmap that is too short
    f = _copy(good)
    f["occ"] = f["occ"][:-1]
    _named(gr.check_structure(pts, row0, n, g, f), "bitmap")


def test_spatial_order_and_its_morton_inversion():
    pts = _cloud(3001, np.float32, seed=3)
    lo, hi = pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64)
    g = {"org": lo, "h": (hi - lo) / 16 * (1.0 + 2.0 ** -40), "dim": np.array([16, 16, 16]), "morton": True}
    c = gr.cells(pts, g)
    # Morton numbers: bit k of x, y, z at bits 3k, 3k + 1, 3k + 2
    xyz = np.clip(np.floor((pts.astype(np.float64) - g["org"]) * (1.0 / g["h"])), 0, 15).astype(np.int64)
    want = np.zeros(len(pts), dtype=np.int64)
    for k in range(4):
        for a in range(3):
            want |= ((xyz[:, a] >> k) & 1) << (3 * k + a)
    assert np.array_equal(c, want) and c.max() < 4096
    good = gr.build_expected(pts, 0, len(pts), g)
    assert gr.check_structure(pts, 0, len(pts), g, good) == []
    gone = dict(good, cell_start=None)                       # the cell starts overwritten: rows, coordinates and the order remain
    assert gr.check_structure(pts, 0, len(pts), g, gone) == []
    p, q = _two_cells(good, len(pts))
    for f in (_copy(good), _copy(gone)):
        f["rows"][[p, q]] = f["rows"][[q, p]]
        f["xyz"][[p, q]] = f["xyz"][[q, p]]
        _named(gr.check_structure(pts, 0, len(pts), g, f), "morton order")
    # the same array against x-fastest numbering is no spatial order of that grid
    assert gr.check_structure(pts, 0, len(pts), dict(g, morton=False), good) != []


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_faces_corners_and_points_outside_a_trimmed_box(dtype):
    """Points exactly on org + k h (formed in the cloud's dtype, as variants_check.place_faces does), on the box's top corner and
    outside a trimmed box land in the cells cell_coord's arithmetic gives: worked here with Python floats, one operation at a
    time."""
    g = _geometry(dim=(9, 11, 6), org=(0.1, -0.3, 0.05), h=(0.013, 0.0171, 0.09))
    org, h, dim = g["org"], g["h"], g["dim"]
    rng = np.random.default_rng(11)
    k = np.stack([rng.integers(0, dim[a] + 1, size=400) for a in range(3)], axis=1).astype(np.float64)
    faces = (org + k * h).astype(dtype)
    top = (org + dim * h).astype(dtype)[None, :]
    outside = np.array([[1000.0, 0.0, 0.1], [-1000.0, -1000.0, -1000.0], [0.15, 1000.0, -1000.0], [org[0], org[1], org[2]]]).astype(dtype)
    pts = np.concatenate([faces, top, outside])
    got = gr.cells(pts, g)
    want = []
    for p in pts:
        c = []
        for a in range(3):
            d = float(np.float64(p[a]) - np.float64(org[a]))             # one rounding
            t = float(np.float64(d) * (np.float64(1.0) / np.float64(h[a])))   # inv_h rounded, then the product rounded
            c.append(int(min(max(np.floor(t), 0.0), float(dim[a] - 1))))
        want.append((c[2] * int(dim[1]) + c[1]) * int(dim[0]) + c[0])
    assert got.tolist() == want
    # the top corner and everything beyond it: the last cell; below the origin: the first
    assert got[len(faces)] == gr.ncells_of(g) - 1
    assert got[len(faces) + 2] == 0
    assert got[len(faces) + 1] % int(dim[0]) == int(dim[0]) - 1          # x = 1000: the last cell of its row
    assert got[-1] == 0                                                   # the origin itself: cell 0
    # a face value rounded to fp32 may fall on either side of the face: the cell is the arithmetic's, not k
    kk = np.clip(k, 0, dim - 1).astype(np.int64)
    naive = (kk[:, 2] * dim[1] + kk[:, 1]) * dim[0] + kk[:, 0]
    if dtype is np.float32:
        assert np.any(got[:len(faces)] != naive), "no face point fell below its face: the case tests nothing"
    # and a structure over these points passes, with every boundary cell holding its outliers
    f = gr.build_expected(pts, 0, len(pts), g)
    assert gr.check_structure(pts, 0, len(pts), g, f) == []
