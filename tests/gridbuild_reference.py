"""What a grid build (open_pcc_metric_amd/csrc/pccm_gridbuild.hip) must leave behind, as plain NumPy in float64 and int64: the
cell of every point, and a checker for the cell starts, records and occupancy bitmap a build wrote.  Host only; the cell
arithmetic is the one tests/vox_reference.py already holds.

The contract (check_structure), for a job over rows [row0, row0 + n) of a cloud and a grid of ncells cells:
  1. cell_start is the exclusive prefix sum of the cells' populations, relative to the job's first record: cell_start[0] == 0,
     cell_start[ncells] == n;
  2. the records' rows, sorted, are exactly row0 .. row0 + n - 1: nothing lost, doubled or taken from outside the job;
  3. every record lies in the segment of the cell of its row's point;
  4. every record's coordinates are bitwise those of its row (fp32 values widened for 16-byte records): -0.0 stays -0.0;
  5. bit c of the occupancy bitmap is set iff cell c holds a record, for c < ncells (nothing reads the bits above);
  6. a spatial order (Morton-numbered cells) satisfies 2 and 4 and its records' cell numbers never decrease.
The order of the records inside a cell is not part of the contract: no result depends on it."""
import numpy as np

from vox_reference import cell_coords


def _spread3(v):
    """x | y << 1 | z << 2 per bit, 10 bits per axis (spread3 in pccm_grid.h)."""
    v = v.astype(np.int64) & 0x3FF
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


def cells(points, geometry):
    """Cell number of every point (cell_linear in pccm_grid.h).  geometry: a mapping with org[3], h[3], dim[3] and, optionally,
    morton (cells numbered along a Z-order curve instead of x-fastest) -- what Engine.build_plan returns."""
    dim = np.asarray(geometry["dim"], np.int64)
    c = cell_coords(np.asarray(points).reshape(-1, 3), geometry["org"], geometry["h"], dim).astype(np.int64)
    if geometry.get("morton"):
        return _spread3(c[:, 0]) | (_spread3(c[:, 1]) << 1) | (_spread3(c[:, 2]) << 2)
    return (c[:, 2] * dim[1] + c[:, 1]) * dim[0] + c[:, 0]


def ncells_of(geometry):
    dim = np.asarray(geometry["dim"], np.int64)
    return int(dim[0] * dim[1] * dim[2])


def occupancy_words(cell_numbers, ncells):
    """The bitmap a build writes for these records: bit c & 31 of word c >> 5 is set iff cell c holds one."""
    bits = np.zeros(((ncells + 31) // 32) * 32, dtype=bool)
    bits[np.asarray(cell_numbers, np.int64)] = True
    return (bits.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def build_expected(points, row0, n, geometry, order=None, bitmap=False):
    """A correct structure for rows [row0, row0 + n) of `points`, as pccm_build_fetch would return it: records in cell order by a
    stable argsort (or in `order`, a permutation of arange(n) that keeps the cells sorted)."""
    pts = np.asarray(points)
    c = cells(pts[row0:row0 + n], geometry)
    if order is None:
        order = np.argsort(c, kind="stable")
    ncells = ncells_of(geometry)
    cs = np.zeros(ncells + 1, dtype=np.uint32)
    cs[1:] = np.cumsum(np.bincount(c, minlength=ncells))
    rows = (row0 + order).astype(np.int32)
    return {"rows": rows, "xyz": pts[rows].astype(np.float64), "cell_start": cs,
            "occ": occupancy_words(c, ncells) if bitmap else None}


def check_structure(points, row0, n, geometry, fetched):
    """-> list of failures (empty: the structure honours the contract above).  points: the whole cloud as it was handed to the
    library, in its dtype; fetched: rows, xyz, cell_start (None: not there to check -- a spatial order whose cell starts are
    gone) and occ (None: the structure keeps no bitmap)."""
    fail = []
    pts = np.asarray(points)
    rows = np.asarray(fetched["rows"]).astype(np.int64)
    xyz = np.asarray(fetched["xyz"], dtype=np.float64).reshape(-1, 3)
    cs = fetched.get("cell_start")
    occ = fetched.get("occ")
    ncells = ncells_of(geometry)
    morton = bool(geometry.get("morton"))
    if len(rows) != n or len(xyz) != n:
        return [f"rows: {len(rows)} records and {len(xyz)} coordinates for a job of {n} rows"]
    want_cells = cells(pts[row0:row0 + n], geometry)       # by row of the job
    counts = np.bincount(want_cells, minlength=ncells)
    # 2. the rows
    outside = (rows < row0) | (rows >= row0 + n)
    if np.any(outside):
        fail.append(f"rows: {int(outside.sum())} records carry a row outside the job's [{row0}, {row0 + n}), first {int(rows[outside][0])}"
                    f" at position {int(np.flatnonzero(outside)[0])}")
    if not np.array_equal(np.sort(rows), np.arange(row0, row0 + n)):
        seen = np.bincount(rows[~outside] - row0, minlength=n)
        fail.append(f"rows: not a permutation of the job's rows: {int(np.sum(seen == 0))} lost, {int(np.sum(seen > 1))} doubled")
    ok = ~outside
    # 4. the coordinates, bit for bit
    want_xyz = pts[rows[ok]].astype(np.float64)
    diff = np.any(want_xyz.view(np.int64) != np.ascontiguousarray(xyz[ok]).view(np.int64), axis=1)
    if np.any(diff):
        p = int(np.flatnonzero(ok)[np.flatnonzero(diff)[0]])
        fail.append(f"xyz: {int(diff.sum())} records differ bitwise from their row's point, first at position {p}: "
                    f"{xyz[p].tolist()} for row {int(rows[p])} = {pts[rows[p]].astype(np.float64).tolist()}")
    rec_cells = np.full(n, -1, dtype=np.int64)
    rec_cells[ok] = want_cells[rows[ok] - row0]
    # 1. the cell starts
    if cs is not None:
        cs = np.asarray(cs).astype(np.int64)
        want_cs = np.zeros(ncells + 1, dtype=np.int64)
        want_cs[1:] = np.cumsum(counts)
        if len(cs) != ncells + 1:
            fail.append(f"cell_start: {len(cs)} entries for {ncells} cells")
        else:
            if cs[0] != 0:
                fail.append(f"cell_start[0] = {int(cs[0])}, not 0")
            if cs[ncells] != n:
                fail.append(f"cell_start[ncells] = {int(cs[ncells])}, not the job's {n} records")
            bad = np.flatnonzero(cs != want_cs)
            if len(bad):
                fail.append(f"cell_start: {len(bad)} entries differ from the prefix sum of the cells' populations, first "
                            f"cell_start[{int(bad[0])}] = {int(cs[bad[0]])}, want {int(want_cs[bad[0]])}")
            # 3. every record in its cell's segment (the segment a position lies in: the last cell that starts at or before it,
            # so empty cells, which share their start with the next one, are passed over)
            seg = np.searchsorted(cs, np.arange(n), side="right") - 1
            wrong = ok & (seg != rec_cells)
            if np.any(wrong):
                p = int(np.flatnonzero(wrong)[0])
                fail.append(f"segment: {int(wrong.sum())} records lie outside their cell's segment, first position {p} (row "
                            f"{int(rows[p])}, cell {int(rec_cells[p])}) in the segment of cell {int(seg[p])}")
    # 5. the bitmap
    if occ is not None:
        occ = np.asarray(occ).astype(np.uint32)
        if len(occ) < (ncells + 31) // 32:
            fail.append(f"bitmap: {len(occ)} words for {ncells} cells")
        else:
            got = ((occ[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)[:ncells]
            clear = np.flatnonzero(~got & (counts > 0))
            extra = np.flatnonzero(got & (counts == 0))
            if len(clear):
                fail.append(f"bitmap: bit clear for {len(clear)} occupied cells, first cell {int(clear[0])}")
            if len(extra):
                fail.append(f"bitmap: bit set for {len(extra)} empty cells, first cell {int(extra[0])}")
    # 6. a spatial order: cell numbers along the array never decrease
    if morton:
        down = np.flatnonzero(ok[1:] & ok[:-1] & (rec_cells[1:] < rec_cells[:-1]))
        if len(down):
            p = int(down[0])
            fail.append(f"morton order: the cell number decreases at {len(down)} places, first from {int(rec_cells[p])} at position "
                        f"{p} to {int(rec_cells[p + 1])}")
    return fail
