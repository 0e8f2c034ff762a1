"""Host-only checks of tests/vox_reference.py, the planted integer cases tests/test_gpu_vox_planted.py holds the voxel-brick and
lattice searches to: every generator's answer by construction equals the int64 brute force, no family leaves a probe out, the
grid every family plans is the one its points span, and the predicted tail sets are what k_vox_query's contract says (a best
d2 <= 64 is final; with rows, at most 12 equidistant nearest voxels)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vox_reference as vr  # noqa: E402

R3 = {1: 6, 2: 12, 3: 8, 5: 24, 6: 24, 9: 30, 17: 48, 18: 36, 26: 72, 41: 96, 64: 6}
EMPTY_D2 = [7, 15, 23, 28, 31, 39, 47, 55, 60, 63]

# queries and searched points of every family: nothing is filtered, so a generator that drops a probe fails here
SIZES = {"A": (9210, 18420), "C": (55, None), "E": (4608, 2304), "E4": (6144, 3072), "F_border": (2 + 8 * 8 + 12 * 12 + 6 * 18,) * 2, "F_1x1x1": (3, 3),
         "F_2x1x1": (6, 6), "F_5x3x3": (2 + 4 * 8 + 4 * 12 + 4 * 8 + 0, None), "F_negative": (2 + 8 * 8 + 12 * 12 + 6 * 18,) * 2,
         "Dself": (len(vr.D_SELF_STEPS) * 36 + 1,) * 2}


def test_brute_force_on_a_case_worked_by_hand():
    s = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 2, 0], [5, 5, 5], [0, 0, 0]], dtype=np.float32)
    q = np.array([[1, 0, 0], [0, 1, 0], [5, 5, 4], [0, 0, 0]], dtype=np.float32)
    row, d2, nvox = vr.brute_nn(q, s)
    assert row.tolist() == [0, 0, 4, 0] and d2.tolist() == [1, 1, 1, 0] and nvox.tolist() == [2, 2, 1, 1]
    row, d2, nvox = vr.brute_nn(s, s, skip_same_index=True)
    assert row.tolist() == [5, 0, 3, 2, 1, 0] and d2.tolist() == [0, 4, 0, 0, 59, 0] and nvox.tolist() == [1, 1, 1, 1, 2, 1]
    assert vr.predicted_tail([64, 65, 3, 3], [1, 1, 12, 13], rows=False).tolist() == [False, True, False, False]
    assert vr.predicted_tail([64, 65, 3, 3], [1, 1, 12, 13], rows=True).tolist() == [False, True, False, True]


def test_sums_of_three_squares():
    for d2, want in R3.items():
        assert vr.r3(d2) == want, d2
    assert [d2 for d2 in range(1, 65) if vr.r3(d2) == 0] == EMPTY_D2
    for d2 in vr.B_NEAR + vr.B_WALK:
        assert vr.r3(d2) >= 2


def test_family_a_counts():
    vs = vr.vectors_upto(81)
    n2 = (vs * vs).sum(axis=1)
    assert (int(np.sum(n2 > 0)), int(np.sum((n2 > 0) & (n2 <= 64))), int(np.sum(n2 > 64))) == (3070, 2108, 962)
    fam = vr.family("A")
    assert (len(fam.queries), len(fam.searched)) == (9210, 18420)
    assert len(np.unique(fam.queries, axis=0)) == 9210 and len(np.unique(fam.searched, axis=0)) == 18420
    # 8-voxel cells over the box: more than the 262144 that give k_vox_list several words per thread, within vox_feasible's 2^24
    assert fam.dims.tolist() == [130, 130, 130] and 262144 < fam.ncells() <= 1 << 24
    # each vector from in-cell (0, 0, 0), (7, 7, 7) and one more offset
    assert int(np.sum(np.all(fam.offsets == 0, axis=1))) >= 3070 and int(np.sum(np.all(fam.offsets == 7, axis=1))) >= 3070
    row, d2, nvox = fam.reference(0)
    v = fam.searched[row].astype(np.int64) - fam.queries.astype(np.int64)
    for o in ((0, 0, 0), (7, 7, 7)):
        got = {tuple(x) for x in v[np.all(fam.offsets == o, axis=1)]}
        assert got == {tuple(x) for x in vs[n2 > 0]}, o
    assert np.all(nvox == 1) and np.array_equal(d2, (v * v).sum(axis=1))
    assert int(vr.predicted_tail(d2, nvox, rows=False).sum()) == 2886 == int(vr.predicted_tail(d2, nvox, rows=True).sum())


@pytest.mark.parametrize("name", vr.NAMES)
def test_construction_equals_brute_force(name):
    fam = vr.family(name)
    if name in SIZES:
        nq, ns = SIZES[name]
        assert len(fam.queries) == nq and (ns is None or len(fam.searched) == ns)
    assert fam.queries.dtype == np.float32 and fam.searched.dtype == np.float32
    lo = np.minimum(fam.queries.min(axis=0), fam.searched.min(axis=0))
    hi = np.maximum(fam.queries.max(axis=0), fam.searched.max(axis=0))
    assert np.array_equal(lo, fam.org) and np.array_equal(np.floor((hi - lo) / 8.0) + 1, fam.dims)
    assert np.all(fam.dims <= 2048) and fam.ncells() <= 1 << 24 and np.abs(np.concatenate([lo, hi])).max() < 4194304      # vox_feasible
    if fam.offsets is not None:
        assert np.array_equal(fam.realised_offsets(), fam.offsets)
    row, d2, nvox = fam.reference(0)
    assert len(row) == len(fam.queries) and row.min() >= 0 and row.max() < len(fam.searched) and nvox.min() >= 1
    if fam.d2 is not None:
        known = fam.d2 >= 0
        assert np.array_equal(d2[known], fam.d2[known]) and np.array_equal(nvox[known], fam.nvox[known])
        known = fam.row >= 0
        assert np.array_equal(row[known], fam.row[known])
    for direction in (1, 2):
        r, d, nv = fam.reference(direction)
        it, se = fam.cloud(direction)
        assert len(r) == len(it) and np.array_equal(((it.astype(np.int64) - se.astype(np.int64)[r]) ** 2).sum(axis=1), d) and nv.min() >= 1


def test_family_b_ties():
    fam = vr.family("B")
    assert np.all(fam.d2 >= 0) and np.all(fam.row >= 0)               # every probe is known by construction (the anchor: d2 = 0)
    row, d2, nvox = fam.reference(0)
    for dd in vr.B_NEAR + vr.B_WALK:
        ts = vr.tie_counts(dd)
        assert set(ts) == {t for t in (2, 11, 12, 13, vr.r3(dd)) if t <= vr.r3(dd)}
        assert sorted(set(nvox[d2 == dd].tolist())) == ts, dd
    # every vector of every d2 <= 16 wins once and loses once
    v = fam.searched[row].astype(np.int64) - fam.queries.astype(np.int64)
    for dd in vr.B_NEAR:
        won = {tuple(x) for x in v[d2 == dd]}
        assert won == {tuple(x) for x in vr.vectors_at(dd)}, dd
        sel = np.flatnonzero(d2 == dd)
        lost = set()
        for i in sel:
            near = fam.searched[((fam.searched.astype(np.int64) - fam.queries[i].astype(np.int64)) ** 2).sum(axis=1) == dd]
            lost |= {tuple(x) for x in near.astype(np.int64) - fam.queries[i].astype(np.int64)} - {tuple(v[i])}
        assert lost == won, dd
    tail = vr.predicted_tail(d2, nvox, rows=True)
    assert np.array_equal(tail, nvox > 12) and int(tail.sum()) == int(np.sum(fam.nvox > 12)) > 0
    assert not vr.predicted_tail(d2, nvox, rows=False).any()


def test_family_c_holds_every_farther_voxel():
    fam = vr.family("C")
    row, d2, nvox = fam.reference(0)
    assert sorted(d2.tolist()) == [0] + [d for d in range(1, 65) if d not in EMPTY_D2]
    assert np.array_equal(nvox[d2 > 0], [vr.r3(int(d)) for d in d2[d2 > 0]])
    for i in np.flatnonzero(d2 > 0):
        rel = fam.searched[fam.sprobe == fam.qprobe[i]].astype(np.int64) - fam.queries[i].astype(np.int64)
        n2 = (rel * rel).sum(axis=1)
        g = np.arange(-8, 9)
        box = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        assert len(rel) == int(np.sum((box * box).sum(axis=1) >= d2[i])) and n2.min() == d2[i]
        rows = np.flatnonzero(fam.sprobe == fam.qprobe[i])
        assert rows[n2 > d2[i]].max() < rows[n2 == d2[i]].min()       # every farther voxel has a smaller row than every nearest one
    assert np.array_equal(vr.predicted_tail(d2, nvox, rows=True), nvox > 12)


def test_family_d_points_per_voxel():
    fam = vr.family("D")
    row, d2, nvox = fam.reference(0)
    _, counts = np.unique(fam.searched, axis=0, return_counts=True)
    assert set(counts.tolist()) == {1, 2, 3, 70}
    assert set(nvox[d2 > 0].tolist()) == {2, 6, 8, 12}
    self_fam = vr.family("Dself")
    r, d, nv = self_fam.reference(2)
    _, inv, counts = np.unique(self_fam.queries, axis=0, return_inverse=True, return_counts=True)
    assert set(counts.tolist()) == {1, 2, 3}
    shared = counts[inv.reshape(-1)] > 1
    assert np.array_equal(d == 0, shared) and np.all(r != np.arange(len(r)))
    assert np.all(r[shared] == [np.flatnonzero((inv.reshape(-1) == inv.reshape(-1)[i]) & (np.arange(len(r)) != i)).min() for i in np.flatnonzero(shared)])


def test_family_e_is_crowded():
    fam = vr.family("E")
    cells, counts = np.unique(fam.queries.astype(np.int64) // 8, axis=0, return_counts=True)
    assert counts.tolist() == [1536, 1536, 1536] and len(fam.queries) > 4096 and fam.dims.tolist() == [4, 1, 1]
    row, d2, nvox = fam.reference(0)
    assert set(d2.tolist()) == {0, 1, 2} and nvox.max() == 6
    wide = vr.family("E4")
    cells, counts = np.unique(wide.queries.astype(np.int64) // 8, axis=0, return_counts=True)
    assert counts.tolist() == [1536] * 4 and wide.dims.tolist() == [5, 1, 1]      # the last cell's records start at 4608 > kVoxMinCap
    assert set(wide.reference(0)[1].tolist()) == {0, 1, 2}


def test_family_f_cells_and_directions():
    fam = vr.family("F_border")
    cell = (fam.queries.astype(np.int64) - fam.org) // 8
    on_border = np.sum((cell == 0) | (cell == fam.dims - 1), axis=1)
    probes = np.ones(len(cell), dtype=bool)
    anchors = np.all(fam.queries == fam.searched[fam.row], axis=1) & (np.all(cell == 0, axis=1) | np.all(cell == fam.dims - 1, axis=1)) & (fam.d2 == 0) \
        & np.all((fam.offsets == 0) | (fam.offsets == 7), axis=1)
    assert int(anchors.sum()) == 2
    probes &= ~anchors
    assert sorted(np.unique(on_border[probes]).tolist()) == [1, 2, 3]                      # face, edge and corner cells
    assert [len(np.unique(cell[probes & (on_border == k)], axis=0)) for k in (3, 2, 1)] == [8, 12, 6]
    row, d2, nvox = fam.reference(0)
    step = (fam.searched[row].astype(np.int64) - fam.org) // 8 - cell
    for c in np.unique(cell[probes], axis=0):
        here = probes & np.all(cell == c, axis=1)
        inside = [d for d in vr.vectors_upto(3) if np.abs(d).max() <= 1 and np.all(c + d >= 0) and np.all(c + d < fam.dims)]
        assert sorted(map(tuple, step[here])) == sorted(map(tuple, inside)), c                # the neighbour lies in every cell around
    neg = vr.family("F_negative")
    assert neg.org.tolist() == [-37, -8, -1000] and np.array_equal(neg.queries - neg.org.astype(np.float32), fam.queries)
    assert [vr.family(n).ncells() for n in ("F_1x1x1", "F_2x1x1", "F_5x3x3")] == [1, 2, 45]


def test_lattice_fallback_prediction():
    # a grid of 10 cells of edge 4 along x: from cell 5 three rings reach 12 + the in-cell part; the outer faces are infinitely far
    q = np.array([[22.0, 0, 0], [22.0, 0, 0], [2.0, 0, 0], [38.0, 0, 0]])
    got = vr.lattice_fallback(q, [13.9 ** 2, 14.1 ** 2, 30.0 ** 2, 100.0], org=[0, 0, 0], h=[4, 1, 1], dim=[10, 1, 1])
    assert got.tolist() == [False, True, True, False]


def test_far_blob_keeps_the_answers():
    fam = vr.family("A")
    far = vr.far_blob(fam)
    assert far.dims[0] > 2048 and len(far.queries) == len(fam.queries)
    moved = far.queries[:, 0] != fam.queries[:, 0]
    assert int(moved.sum()) == len(fam.queries) // 8
    assert np.array_equal(far.reference(0)[0], fam.row) and np.array_equal(far.reference(0)[1], fam.d2)
    for d, (it, se) in enumerate(((far.queries, far.searched), (far.searched, far.queries))):
        for got, want in zip(far.reference(d), vr.brute_nn(it, se)):
            assert np.array_equal(got, want), d
    assert not np.array_equal(far.reference(2)[1], fam.reference(2)[1])


def _table(source, name):
    import re
    body = re.search(name + r"\[[^\]]*\]\s*=\s*\{(.*?)\};", source, re.S).group(1)
    return [int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\d+", re.sub(r"//.*", "", body))]


def test_the_kernel_tables_by_enumeration():
    """c_vox_rows, c_vox_near and c_vox_near_start of pccm_vox.hip, read from the source: every (dy, dz) within 8 exactly once in
    order of dy^2 + dz^2, every (dz, dy, dx >= 0) at exactly d2 <= 16 exactly once, the lists of d2 = 7 and 15 empty."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "open_pcc_metric_amd", "csrc", "pccm_vox.hip")).read()
    rows, near, start = _table(src, "c_vox_rows"), _table(src, "c_vox_near"), _table(src, "c_vox_near_start")
    assert (len(rows), len(near), len(start)) == (200, 153, 18)
    got = [(e >> 16, ((e >> 8) & 0xff) - 8, (e & 0xff) - 8) for e in rows[:197]]
    g = range(-8, 9)
    assert sorted(got) == sorted((dy * dy + dz * dz, dy, dz) for dy in g for dz in g if dy * dy + dz * dz <= 64)
    assert [e[0] for e in got] == sorted(e[0] for e in got)
    assert all(e >> 16 > 64 + 64 for e in rows[197:])                                   # padding: rows beyond anybody's reach
    assert start[0] == 0 and start[-1] == len(near) and start == sorted(start)
    for d2 in range(17):
        lst = [((c & 0x1f) - 8, ((c >> 5) & 0x1f) - 8, c >> 10) for c in near[start[d2]:start[d2 + 1]]]
        want = [tuple(int(x) for x in v) for v in vr.vectors_at(d2) if v[2] >= 0] if d2 else [(0, 0, 0)]
        assert sorted(lst) == sorted(want), d2
    assert start[7] == start[8] and start[15] == start[16]
