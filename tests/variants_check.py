"""Runs rows of the variant table (tests/variant_rows.py) on the GPU: the searches and reductions of each row against the
oracle bit for bit, and the kernels pccm_nn_path reports against the row's expectation.  tests/test_gpu_variants.py calls
run_row() in-process for rows without switches and runs this file in a child process, one per switch set, for the others:
`python tests/variants_check.py ROW [ROW ...]` prints one JSON line per row."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from open_pcc_metric_amd import _native as nat  # noqa: E402
from oracle import oracle as orc  # noqa: E402
import nn_reference  # noqa: E402
import variant_rows as vr  # noqa: E402


def _same(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


class Row:
    def __init__(self, rid):
        self.rid = rid
        self.row = vr.ROWS[rid]
        self.fail = []
        self.paths = set()

    def check(self, ok, what):
        if not ok:
            self.fail.append(what)

    def note(self, eng, which):
        self.paths.update(eng.last_path(which))


def _check_nn(r, eng, d, it, se, self_search, want, second_witness=False):
    b, e = eng.shard_range(d)
    idx, d2 = eng.fetch_nn(d)
    widx, wd2 = want
    r.check(np.array_equal(idx, widx[b:e]), f"dir {d}: idx differs from the oracle at {int(np.sum(idx != widx[b:e]))} rows")
    r.check(_same(d2, wd2[b:e]), f"dir {d}: d2 differs from the oracle at {int(np.sum(d2 != wd2[b:e]))} rows")
    if second_witness:
        ridx, rd2 = nn_reference.nn_brute(it, se, skip_same_index=self_search)
        r.check(np.array_equal(ridx, widx) and _same(rd2, wd2), f"dir {d}: the oracle's kd-tree disagrees with the brute reference")
        r.check(np.array_equal(idx, ridx[b:e]), f"dir {d}: idx differs from the brute reference")
    return idx


def on_faces(q, org, h):
    """Rows of q whose every coordinate is a cell face org + k h of the grid, rounded to q's dtype."""
    k = np.rint((q.astype(np.float64) - org) / h)
    return np.all(q == (org + k * h).astype(q.dtype), axis=1)


def place_faces(r, eng, a, b, rows, engine):
    """Move the queries a[rows['fq']] exactly onto cell faces -- org + k h per axis, rounded to the cloud's dtype -- of the grid the
    library builds for this pair (pccm_grid_geometry), away from the box's ends and the empty slab; repeated until the grid the
    moved queries produce is the one they were placed on."""
    fq = rows["fq"]
    rng = np.random.default_rng(fq.start + len(a))
    for _ in range(4):
        eng.set_cloud(0, a)
        eng.set_cloud(1, b)
        eng.nn_pair(engine)
        org, h, dim = eng.grid_geometry()
        if np.all(on_faces(a[fq], org, h)):
            return a
        t = fq.stop - fq.start
        k = np.stack([rng.integers(2, dim[ax] - 2, size=t) for ax in range(3)], axis=1).astype(np.float64)
        p = org + k * h
        bad = (p[:, 2] > vr.SLAB[0] - 2 * h[2]) & (p[:, 2] < vr.SLAB[1] + 2 * h[2])
        p[bad, 2] = org[2] + np.floor((0.8 - org[2]) / h[2]) * h[2]
        a = a.copy()
        a[fq] = p.astype(a.dtype)
    r.check(False, "the face queries do not lie on the grid's faces")
    return a


def run_search(r, eng, a, b, rows, normals, engine, shard, second_witness, nrm_mode="neighbour"):
    if shard:
        eng.set_shard(*shard)
    if "fq" in rows and engine != "brute":
        a = place_faces(r, eng, a, b, rows, engine)
    eng.set_cloud(0, a)
    eng.set_cloud(1, b)
    want = {0: orc.nn(a, b, method="kdtree"), 1: orc.nn(b, a, method="kdtree"), 2: orc.nn(a, a, skip_same_index=True, method="kdtree")}
    for flavour in normals:
        na, nb = vr._unit(len(a), 5, flavour == "f64"), vr._unit(len(b), 6, flavour == "f64")
        eng.set_normals(0, na)
        eng.set_normals(1, nb)
        for d in (0, 1):
            eng.nn_fuse(d, nrm_mode)
        eng.drop_caches()
        eng.nn_pair(engine)
        for d in (0, 1):
            r.note(eng, d)
        for d, (it, se, nse) in enumerate(((a, b, nb), (b, a, na))):
            _check_nn(r, eng, d, it, se, False, want[d], second_witness)
            lo, hi = eng.shard_range(d)
            proj = eng.point_metric(d, nat.METRIC_PROJ, nrm_mode)
            wproj = orc.point_to_plane(it, se, want[d][0], nse, normal_index=nrm_mode)[lo:hi]
            r.check(_same(proj, wproj), f"dir {d} ({flavour} normals): projections differ from the oracle")
            if not shard:
                (s1, mn1, mx1), (s2, mn2, mx2) = eng.reduce_total_many([(d, nat.METRIC_D1), (d, nat.METRIC_D2)], nrm_mode)
                c1, c2 = want[d][1], wproj * wproj
                r.check(_same(s1, np.sum(c1)) and mn1 == np.min(c1) and mx1 == np.max(c1), f"dir {d}: D1 reduction differs from NumPy")
                r.check(_same(s2, np.sum(c2)) and mn2 == np.min(c2) and mx2 == np.max(c2), f"dir {d}: D2 reduction differs from NumPy")
    if not normals:
        eng.drop_caches()
        eng.nn_pair(engine)
        for d, (it, se) in enumerate(((a, b), (b, a))):
            r.note(eng, d)
            _check_nn(r, eng, d, it, se, False, want[d], second_witness)
    if "fq" in rows and engine != "brute":
        org, h, _ = eng.grid_geometry()
        r.check(np.all(on_faces(a[rows["fq"]], org, h)), "face queries are off the faces of the grid the search ran on")
        if "xr_a" in rows and len(a) >= 60_000:        # volumetric: the holes leave queries whose neighbour is beyond ring 1
            far = int(np.sum(want[0][1] > (2 * h.max()) ** 2)) + int(np.sum(want[1][1] > (2 * h.max()) ** 2))
            r.check(far >= 10, f"only {far} queries have their neighbour beyond ring 1")
    eng.nn(2, engine)
    r.note(eng, 2)
    _check_nn(r, eng, 2, a, a, True, want[2], second_witness)


def run_ties(r, eng, a, b):
    eng.set_cloud(0, a)
    eng.set_cloud(1, b)
    eng.set_ties("mean")
    eng.nn_pair("grid")
    for d, (it, se) in enumerate(((a, b), (b, a))):
        widx, wd2 = nn_reference.nn_brute(it, se)
        idx, d2 = eng.fetch_nn(d)
        r.check(np.array_equal(idx, widx) and _same(d2, wd2), f"dir {d}: rows under ties='mean' differ from the brute reference")
        k = eng.tie_counts(d)
        # the tie sets by brute force: every searched point at exactly the nearest squared distance
        se64, it64 = np.asarray(se, np.float64), np.asarray(it, np.float64)
        wk = np.empty(len(it64), dtype=np.int64)
        for s in range(0, len(it64), 256):
            q = it64[s:s + 256]
            dd = ((q[:, 0:1] - se64[:, 0]) ** 2 + (q[:, 1:2] - se64[:, 1]) ** 2) + (q[:, 2:3] - se64[:, 2]) ** 2
            wk[s:s + 256] = np.sum(dd == wd2[s:s + 256, None], axis=1)
        r.check(np.array_equal(k, wk), f"dir {d}: tie counts differ from brute force at {int(np.sum(k != wk))} rows")
        r.check(int(np.sum(wk >= 2)) > 100, f"dir {d}: the data has too few exact ties to test them")
        ex = eng.tie_exposure(d)
        r.note(eng, d)
        tied = int(np.sum(wk >= 2))
        if ex["not_enumerated"] == 0:                   # every tie set enumerated: the counts are exact
            r.check(ex["queries"] == len(it64) and ex["tied"] == tied and ex["max_multiplicity"] == int(wk.max()),
                    f"dir {d}: tie exposure {ex} against {tied} tied queries, largest tie set {int(wk.max())}")
        else:
            r.check(ex["queries"] == len(it64) and ex["tied"] + ex["not_enumerated"] >= tied >= ex["tied"] and
                    ex["max_multiplicity"] <= int(wk.max()), f"dir {d}: tie exposure {ex} against {tied} tied queries")
    eng.set_ties("pick")


def run_reduce(r, eng, a, b):
    """Batches as test_reduction_batches_of_every_shape builds them, for every record layout a search leaves: 32- and 16-byte
    records, matched records with fp32-exact or fp64 normals, row- or neighbour-indexed, distances only, plain columns."""
    want = {0: orc.nn(a, b, method="kdtree"), 1: orc.nn(b, a, method="kdtree")}
    eng.set_cloud(0, a)
    eng.set_cloud(1, b)
    D1, D2, PR = nat.METRIC_D1, nat.METRIC_D2, nat.METRIC_PROJ
    batches = [[(0, D1)], [(1, D2)], [(0, D1), (0, D2), (1, D1), (1, D2)], [(0, D1), (1, D2)], [(0, PR), (1, PR)],
               [(0, D1), (0, PR)], [(1, D2), (1, D1)]]
    for engine in ("grid", "brute"):
        for flavour in ("f32", "f64", None):
            for mode in ("neighbour", "row"):
                for want_idx in (True, False):
                    if flavour is None and mode == "row":
                        continue
                    na = nb = None
                    if flavour:
                        # row-indexed normals need a row for every query of the other cloud
                        la, lb = (len(a), len(b)) if mode == "neighbour" else (max(len(a), len(b)),) * 2
                        na, nb = vr._unit(la, 7, flavour == "f64"), vr._unit(lb, 8, flavour == "f64")
                        eng.set_normals(0, na)
                        eng.set_normals(1, nb)
                    for fuse in ((mode, None) if flavour else (None,)):
                        for d in (0, 1):
                            eng.nn_fuse(d, fuse)
                        eng.nn_want_idx(want_idx)
                        cols = {}
                        for d, (it, se, nse) in enumerate(((a, b, nb), (b, a, na))):
                            cols[(d, D1)] = want[d][1]
                            if flavour:
                                p = orc.point_to_plane(it, se, want[d][0], nse, normal_index=mode)
                                cols[(d, PR)], cols[(d, D2)] = p, p * p
                        for batch in batches:
                            if not flavour and any(met != D1 for _, met in batch):
                                continue
                            eng.drop_caches()
                            eng.nn_pair(engine)
                            got = eng.reduce_total_many(batch, mode)
                            r.note(eng, nat.PATH_REDUCE)
                            for (d, met), (total, mn, mx) in zip(batch, got):
                                col = cols[(d, met)]
                                r.check(_same(total, np.sum(col)) and mn == np.min(col) and mx == np.max(col),
                                        f"{engine} {flavour} {mode} idx={want_idx} fuse={fuse}: batch {batch}, column {(d, met)} differs from NumPy")
    eng.nn_want_idx(True)
    for d in (0, 1):
        eng.nn_fuse(d, None)


def run_row(rid):
    r = Row(rid)
    row = r.row
    gen = dict(row["gen"])
    shard = gen.pop("shard", None)
    lengths = gen.pop("lengths", None)
    a, b, rows = vr.make_pair(**gen)
    eng = nat.Engine(0)
    try:
        eng.nn_want_idx(row.get("want_idx", True))
        if row["kind"] == "brick":
            run_search(r, eng, a, b, rows, ("f32", "f64"), "auto", shard, False)
        elif row["kind"] == "search":
            small = len(a) * len(b) <= 20_011 * 20_011
            run_search(r, eng, a, b, rows, (), row.get("engine", "auto"), shard, small)
        elif row["kind"] == "ties":
            run_ties(r, eng, a, b)
        elif row["kind"] == "reduce":
            for n, m in lengths:                        # column lengths at and around the 128-row leaves and 8192-row chunks
                a, b, _ = vr.make_pair(n, m, seed=gen.get("seed", 0))
                run_reduce(r, eng, a, b)
        r.check(not any(k == "..." for k in r.paths), "a path log overflowed")
    finally:
        eng.close()
    missing = [k for k in row["expect"] if k not in r.paths]
    r.check(not missing, f"variants not reached: {missing}; the paths named {sorted(r.paths)}")
    return {"row": rid, "fail": r.fail, "paths": sorted(r.paths)}


if __name__ == "__main__":
    for rid in sys.argv[1:]:
        print(json.dumps(run_row(rid)), flush=True)
