"""Rows of tests/test_gpu_gridbuild.py: each runs searches on the GPU with the grid engine forced, reads back every structure the
grid build left (Engine.build_plan / build_fetch: cell starts, records, occupancy bitmap of both clouds, shard query lists,
spatial orders) and holds it to tests/gridbuild_reference.check_structure.  Every row asserts its own precondition -- the tile
count, the bin populations, the path the build took -- from the plan the library reports or from the fetched cell starts.
test_gpu_gridbuild.py calls run_row() in-process for rows without switches and runs this file in a child process, one per
switch set, for the others: `python tests/gridbuild_check.py ROW [ROW ...]` prints one JSON line per row."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from open_pcc_metric_amd import _native as nat  # noqa: E402
import gridbuild_reference as gref  # noqa: E402
import variant_rows as vr  # noqa: E402
from vox_reference import cell_coords  # noqa: E402

G0, G1, SL, SR, SS, P0, P1 = (nat.BUILD_GRID0, nat.BUILD_GRID1, nat.BUILD_SHARD_LEFT, nat.BUILD_SHARD_RIGHT, nat.BUILD_SHARD_SELF,
                              nat.BUILD_SP0, nat.BUILD_SP1)
NAMES = {G0: "grid/cloud 0", G1: "grid/cloud 1", SL: "shard LEFT", SR: "shard RIGHT", SS: "shard SELF", P0: "spatial order 0",
         P1: "spatial order 1"}
CLOUD_OF = {G0: 0, G1: 1, SL: 0, SR: 1, SS: 0, P0: 0, P1: 1}
KREG = 2048          # kRegRecs: records a bin of k_bin_sort keeps in registers; larger bins are streamed twice

# switch sets: one child process each (the library latches its switches once per process)
ENVS = {
    "": {},
    "tile256": {"PCCM_BUILD_TILE": "256"},
    "scan_tile256": {"PCCM_BUILD_SCAN": "1", "PCCM_BUILD_TILE": "256"},
    "threads256": {"PCCM_BUILD_THREADS": "256"},
}


class Row:
    def __init__(self, rid):
        self.rid = rid
        self.fail = []
        self.info = {}

    def check(self, ok, what):
        if not ok:
            self.fail.append(what)


def missing(eng, which):
    try:
        eng.build_plan(which)
    except nat.PccmStateError:
        return True
    return False


def check_left(r, eng, clouds, label, expect):
    """Every structure the library says is there, against the contract; `expect`: the structures this step must have left.
    -> {structure: fetched}"""
    found = {}
    for which in NAMES:
        if missing(eng, which):
            continue
        f = eng.build_fetch(which)
        plan = f["plan"]
        pts = clouds[CLOUD_OF[which]]
        r.check(plan["ncells"] == gref.ncells_of(plan), f"{label}: {NAMES[which]}: ncells {plan['ncells']} is not the product of dim")
        for m in gref.check_structure(pts, plan["row0"], plan["n"], plan, f):
            r.fail.append(f"{label}: {NAMES[which]}: {m}")
        found[which] = f
    for which in expect:
        r.check(which in found, f"{label}: {NAMES[which]} is not there to check")
    return found


def bin_populations(f):
    cs, lg, ncells = f["cell_start"].astype(np.int64), f["plan"]["lg"], f["plan"]["ncells"]
    edges = np.minimum(np.arange(0, f["plan"]["nbin"] + 1, dtype=np.int64) << lg, ncells)
    return np.diff(cs[edges])


def uniform(n, seed, f64=False):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3)) if f64 else rng.random((n, 3), dtype=np.float32)


def search_pair(r, eng, a, b, label, expect=(G0, G1)):
    eng.set_cloud(0, a)
    eng.set_cloud(1, b)
    eng.nn_pair("grid")
    return check_left(r, eng, (a, b), label, expect)


# ---- default switches -------------------------------------------------------------------------------------------------------
def row_quads(r, eng, f64):
    """n % 4 of 1, 3, 2, 0; one tile exactly full, two tiles; a last bin of fewer than 2^lg cells."""
    ragged = False
    for n, m in ((3001, 2999), (3002, 4096), (8192, 8193)):
        a, b = uniform(n, n, f64), uniform(m, m + 1, f64)
        found = search_pair(r, eng, a, b, f"{n}+{m}")
        for which in found:
            p = found[which]["plan"]
            r.check(p["rec32"] == (0 if f64 else 1), f"{n}+{m}: {NAMES[which]}: rec32 = {p['rec32']}")
            ragged = ragged or p["ncells"] % (1 << p["lg"]) != 0
            r.info[f"{n}+{m}/{which}"] = [p["ncells"], p["lg"], p["nbin"], p["tiles"], p["tile_rows"]]
        if n == 8192 and G0 in found and G1 in found:
            p0, p1 = found[G0]["plan"], found[G1]["plan"]
            r.check(p0["tiles"] == 1 and p0["tile_rows"] == 8192, f"8192 rows are not one full tile: {p0['tiles']} x {p0['tile_rows']}")
            r.check(p1["tiles"] == 2, f"8193 rows are not two tiles: {p1['tiles']} x {p1['tile_rows']}")
    r.check(ragged, "no build had a last bin of fewer than 2^lg cells (ncells % 2^lg == 0 in all of them)")


def row_tiles(r, eng, f64):
    """Three tiles per job, the last one short."""
    found = search_pair(r, eng, uniform(20_011, 1, f64), uniform(19_997, 2, f64), "20011+19997")
    for which, f in found.items():
        p = f["plan"]
        r.check(p["tiles"] == 3 and (p["tiles"] - 1) * p["tile_rows"] < p["n"] < p["tiles"] * p["tile_rows"],
                f"{NAMES[which]}: {p['tiles']} tiles of {p['tile_rows']} rows for {p['n']} rows")
        r.check(p["rec32"] == (0 if f64 else 1) and p["scan"] == 0, f"{NAMES[which]}: rec32 {p['rec32']}, scan {p['scan']}")


def row_faces(r, eng):
    """500 rows on cell faces (org + k h per axis, formed in the cloud's dtype as variants_check.place_faces does), the two corners
    of the bounding box and a -0.0; built, read, moved and rebuilt until the geometry is the one the points were placed on."""
    from variants_check import on_faces
    a, b = uniform(6000, 21), uniform(6000, 22)
    a[500], a[501], a[502] = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (-0.0, 0.5, 0.5)
    rng = np.random.default_rng(23)
    found = {}
    for _ in range(4):
        found = search_pair(r, eng, a, b, "faces")
        org, h, dim = eng.grid_geometry()
        if np.all(on_faces(a[:500], org, h)):
            break
        k = np.stack([rng.integers(1, dim[ax], size=500) for ax in range(3)], axis=1).astype(np.float64)
        a = a.copy()
        a[:500] = (org + k * h).astype(a.dtype)
    else:
        r.check(False, "the face rows do not lie on the faces of the grid the search ran on")
    if G0 in found:
        p = found[G0]["plan"]
        r.check(np.array_equal(p["org"], eng.grid_geometry()[0]) and np.array_equal(p["h"], eng.grid_geometry()[1]),
                "the plan's geometry is not pccm_grid_geometry's")
        r.check(np.all(on_faces(a[:500], p["org"], p["h"])), "face rows off the faces")
        c = gref.cells(a[500:503], p)
        r.check(c[0] == 0 and c[1] == p["ncells"] - 1, f"the box's corners are in cells {c[:2].tolist()} of {p['ncells']}")
        at = np.flatnonzero(found[G0]["rows"] == 502)
        r.check(len(at) == 1 and np.signbit(found[G0]["xyz"][at[0], 0]), "the -0.0 coordinate did not come back as -0.0")


def row_trimmed(r, eng):
    """Eight outliers at +-1000: the grid covers a quantile box, the outliers are clamped into its boundary cells."""
    a, b = uniform(20_008, 31), uniform(20_000, 32)
    a[-8:] = np.array([[sx, sy, sz] for sx in (-1000, 1000) for sy in (-1000, 1000) for sz in (-1000, 1000)], dtype=np.float32)
    found = search_pair(r, eng, a, b, "trimmed")
    if G0 in found:
        p = found[G0]["plan"]
        top = p["org"] + p["dim"] * p["h"]
        r.check(np.all(p["org"] > a.min(axis=0)) and np.all(top < a.max(axis=0)),
                f"the grid's box {p['org'].tolist()} .. {top.tolist()} is not inside the data's +-1000")
        c = cell_coords(a[-8:], p["org"], p["h"], p["dim"])
        r.check(np.all((c == 0) | (c == p["dim"] - 1)), "an outlier is not in a boundary cell")
        at = np.isin(found[G0]["rows"], np.arange(20_000, 20_008))
        r.check(int(at.sum()) == 8, "the outliers' records are not all there")


def row_streamed(r, eng):
    """Bins above and below kRegRecs records: a clump of 2500 points inside a cube of edge 1e-6 and 300 exact duplicates."""
    a, b = uniform(20_000, 41), uniform(20_000, 42)
    rng = np.random.default_rng(43)
    a[:2500] = (0.5 + rng.random((2500, 3)) * 1e-6).astype(np.float32)
    a[2500:2800] = a[3000:3300]
    found = search_pair(r, eng, a, b, "clump")
    if G0 in found:
        pop = bin_populations(found[G0])
        r.info["clump bins"] = [int(pop.max()), int(pop[pop > 0].min()), len(pop)]
        r.check(np.any(pop > KREG), f"no bin holds more than {KREG} records (largest {int(pop.max())})")
        r.check(np.any((pop > 0) & (pop <= KREG)), f"no non-empty bin holds at most {KREG} records")


def planted_bins():
    """A voxelised cloud whose 8-voxel cells form 64 x 16 x 8 = 8 layers of 1024 cells: with bins of 2^10 cells a layer is a bin.
    Layer 0 holds exactly 2048 points, layer 1 exactly 2049, every other layer 64 (so that no quantile box trims the far
    layers away: a trimmed box takes the pair off the voxel bricks); the box's two corners are among them."""
    rng = np.random.default_rng(51)
    layers = []
    for z, count in enumerate((KREG, KREG + 1, 64, 64, 64, 64, 64, 64)):
        v = rng.permutation(512 * 128 * 8 - 2)[:count - 1] + 1           # distinct voxels of the layer, its two corners left out
        p = np.stack([v % 512, (v // 512) % 128, 8 * z + v // (512 * 128)], axis=1)
        layers.append(np.concatenate([p, [[0, 0, 8 * z]] if z < 7 else [[511, 127, 63]]]))
    a = np.concatenate(layers).astype(np.float32)
    assert len(np.unique(a, axis=0)) == len(a) == 2 * KREG + 1 + 6 * 64
    return a[rng.permutation(len(a))]


def row_planted_bins(r, eng):
    """One bin of exactly kRegRecs records (the register path's largest) and one of kRegRecs + 1 (the smallest streamed one), on a
    voxel-brick grid where populations can be planted exactly."""
    a = planted_bins()
    b = a[np.random.default_rng(52).permutation(len(a))]
    found = search_pair(r, eng, a, b, "planted bins")
    for which in (G0, G1):
        if which not in found:
            continue
        p = found[which]["plan"]
        r.check(np.all(p["h"] == 8.0) and p["has_occ"] == 1, f"{NAMES[which]}: not a voxel-brick grid: h {p['h'].tolist()}")
        pop = bin_populations(found[which])
        r.info[f"planted/{which}"] = [p["lg"], p["nbin"], pop.tolist()]
        r.check(KREG in pop.tolist() and KREG + 1 in pop.tolist(), f"{NAMES[which]}: bins of {pop.tolist()} records, lg {p['lg']}: no "
                f"pair of exactly {KREG} and {KREG + 1}")


def row_bitmaps(r, eng):
    """Occupancy bitmaps: a spread integer pair (the lattice search reads them) and a dense one (the voxel bricks are built from
    them); crowded cells make the bins smaller than 2^10 cells; a cell count that is no multiple of 64 reaches the ballot tail."""
    a, b, _ = vr.make_pair(10_000, 10_000, voxel=True, spread=True)
    found = search_pair(r, eng, a, b, "spread")
    odd = False
    for which, f in found.items():
        r.check(f["plan"]["has_occ"] == 1 and f["occ"] is not None, f"spread: {NAMES[which]} has no bitmap")
        odd = odd or f["plan"]["ncells"] % 64 != 0
        r.info[f"spread/{which}"] = [f["plan"]["ncells"], f["plan"]["lg"]]
    g = np.arange(32)
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(61)
    block = block[rng.permutation(len(block))]
    sub = block[rng.random(len(block)) < 0.7]
    found = search_pair(r, eng, block, sub, "dense")
    for which, f in found.items():
        r.check(f["plan"]["has_occ"] == 1 and f["occ"] is not None, f"dense: {NAMES[which]} has no bitmap")
        r.check(f["plan"]["lg"] < 10, f"dense: {NAMES[which]}: lg = {f['plan']['lg']}: the crowded-cell rule did not shrink the bins")
        odd = odd or f["plan"]["ncells"] % 64 != 0
        r.info[f"dense/{which}"] = [f["plan"]["ncells"], f["plan"]["lg"]]
    r.check(odd, "ncells is a multiple of 64 in both pairs: the ballot tail of write_cell_starts did not run")


def row_spatial(r, eng, n):
    """The spatial order at its 4096-point threshold: made by the first drop_caches behind a search, read by the next build."""
    a, b = uniform(n, 70 + n), uniform(n, 71 + n)
    search_pair(r, eng, a, b, f"{n}: first search")
    eng.drop_caches()
    want = n >= 4096
    found = check_left(r, eng, (a, b), f"{n}: after drop_caches", (P0, P1) if want else ())
    r.check((P0 in found) == want and (P1 in found) == want, f"{n}: spatial orders there: {P0 in found}, {P1 in found}; expected {want}")
    if want and P1 in found:
        r.check(found[P1]["cell_start"] is not None, f"{n}: the cell starts of the spatial order just made are not there")
        p = found[P1]["plan"]
        r.check(p["morton"] == 1 and p["rec32"] == 1 and np.all(p["dim"] == 1 << p["bits"]) and p["read_sp"] == 0,
                f"{n}: spatial order's plan: {p['morton']}, {p['rec32']}, {p['dim'].tolist()}, bits {p['bits']}")
    eng.nn_pair("grid")
    found = check_left(r, eng, (a, b), f"{n}: second search", (G0, G1, P0, P1) if want else (G0, G1))
    for which in (G0, G1):
        if which in found:
            r.check(found[which]["plan"]["read_sp"] == int(want), f"{n}: {NAMES[which]}: read_sp = {found[which]['plan']['read_sp']}")
    for which in (P0, P1):
        if which in found:
            r.check(found[which]["cell_start"] is None, f"{n}: {NAMES[which]}: cell starts claimed after a build overwrote them")


def row_shards(r, eng, f64):
    """World 3, every rank: one sharded direction rides in the grid build's launches (fp32), two are sorted by a build of their
    own; the shard's rows are exactly [begin, end) of pccm_shard_range."""
    a, b = uniform(20_011, 81, f64), uniform(19_997, 82, f64)
    eng.set_cloud(0, a)
    eng.set_cloud(1, b)
    for rank in range(3):
        eng.set_shard(rank, 3)
        for d, shard, grid in ((nat.DIR_LEFT, SL, G1), (nat.DIR_RIGHT, SR, G0)):
            label = f"rank {rank} dir {d}"
            eng.drop_caches()
            eng.nn(d, "grid")
            found = check_left(r, eng, (a, b), label, (shard, grid))
            begin, end = eng.shard_range(d)
            if shard in found:
                p = found[shard]["plan"]
                r.check(p["row0"] == begin and p["n"] == end - begin and end > begin, f"{label}: shard rows [{p['row0']}, +{p['n']}), range [{begin}, {end})")
                if f64:
                    r.check(p["rec32"] == 0 and p["njobs"] == 1, f"{label}: fp64 shard: rec32 {p['rec32']}, {p['njobs']} jobs")
                else:      # the riding form: the searched cloud and the shard in one build
                    r.check(p["rec32"] == 1 and p["njobs"] == 2 and p["job"] == 1 and p["job_row0_1"] == begin and p["job_row0_0"] == 0,
                            f"{label}: the shard did not ride in the grid build: {p['njobs']} jobs, job {p['job']}, rows from {p['job_row0_1']}")
                    r.check((begin != 0) == (rank != 0), f"{label}: shard begins at {begin}")
                    if grid in found:
                        q = found[grid]["plan"]
                        r.check(q["njobs"] == 2 and q["job"] == 0, f"{label}: searched cloud's build: {q['njobs']} jobs, job {q['job']}")
        eng.drop_caches()
        eng.nn_pair("grid")
        label = f"rank {rank} both directions"
        found = check_left(r, eng, (a, b), label, (G0, G1, SL, SR))
        for d, shard in ((nat.DIR_LEFT, SL), (nat.DIR_RIGHT, SR)):
            begin, end = eng.shard_range(d)
            if shard in found:
                p = found[shard]["plan"]
                r.check(p["row0"] == begin and p["n"] == end - begin, f"{label}: shard {d} rows [{p['row0']}, +{p['n']}), range [{begin}, {end})")
                r.check(p["njobs"] == 2 and p["job"] == d, f"{label}: the two shards were not sorted as two jobs of one build: {p['njobs']}, {p['job']}")


def row_solo(r, eng):
    """The k-NN grid over one cloud alone: 32-byte records from fp32 data, a geometry of its own, records behind cloud 0's."""
    a, b = uniform(60_000, 91), uniform(5000, 92)
    found = search_pair(r, eng, a, b, "pair")
    pair_h = found[G1]["plan"]["h"] if G1 in found else None
    eng.estimate_normals(1, 30)
    found = check_left(r, eng, (a, b), "solo", (G1,))
    r.check(G0 not in found, "cloud 0's records are claimed although the solo build reused the buffers")
    if G1 in found:
        p = found[G1]["plan"]
        r.check(p["rec32"] == 0 and p["n"] == 5000 and p["njobs"] == 1, f"solo: rec32 {p['rec32']}, n {p['n']}, jobs {p['njobs']}")
        r.check(pair_h is not None and np.all(p["h"] != pair_h), f"solo: cells of {p['h'].tolist()}, the pair's {pair_h}: not a geometry of its own")


def row_rebuilds(r, eng):
    """One engine, builds of 60 000, 3001, 20 011 points and the first again: cursors left at zero, stale toff rows, fewer bins."""
    sizes = ((60_000, 59_999), (3001, 2999), (20_011, 19_997), (60_000, 59_999))
    nbin = []
    for k, (n, m) in enumerate(sizes):
        found = search_pair(r, eng, uniform(n, 100 + n), uniform(m, 101 + m), f"build {k} ({n}+{m})")
        nbin.append(found[G0]["plan"]["nbin"] if G0 in found else -1)
        if G0 in found:
            r.check(found[G0]["plan"]["scan"] == 0, f"build {k}: not the cursor build")
    r.info["nbin"] = nbin
    r.check(0 < nbin[1] < nbin[0] and nbin[3] == nbin[0], f"bins per build {nbin}: the second build does not have fewer bins than the first")


def row_degenerate(r, eng):
    """One point, identical points, a plane; and a context whose other cloud was never set (pccm_set_cloud takes no empty cloud)."""
    search_pair(r, eng, uniform(1, 111), uniform(3001, 112), "one point")
    same = np.tile(np.array([[1.5, -2.0, 3.25]]), (2000, 1))
    found = search_pair(r, eng, same, same[:1500], "identical")
    if G0 in found:
        r.check(found[G0]["plan"]["ncells"] == 1, f"identical points in {found[G0]['plan']['ncells']} cells")
    pa, pb = uniform(4000, 113, True), uniform(3500, 114, True)
    pa[:, 2] = pb[:, 2] = 0.25
    found = search_pair(r, eng, pa, pb, "plane")
    if G0 in found:
        r.check(found[G0]["plan"]["dim2"] == 1 and found[G0]["plan"]["ncells"] > 1, f"plane: dim {found[G0]['plan']['dim'].tolist()}")
    lone = nat.Engine(0)
    try:
        a = uniform(3001, 115)
        lone.set_cloud(0, a)
        lone.nn(nat.DIR_SELF, "grid")
        found = check_left(r, lone, (a, None), "cloud 1 never set", (G0,))
        r.check(G1 not in found, "a cloud that was never set has a grid")
    finally:
        lone.close()


def row_validity(r, eng):
    """When a structure can be asked for: never before it was built, not after pccm_drop_caches or a later build overwrote it,
    not during graph capture; and a captured build leaves, at every replay, what an eager one leaves."""
    a, b = uniform(20_011, 151), uniform(19_997, 152)
    for which in NAMES:
        r.check(missing(eng, which), f"fresh context: {NAMES[which]} is claimed")
    for bad in (-1, len(NAMES)):
        try:
            eng.build_plan(bad)
            r.check(False, f"structure {bad} was accepted")
        except ValueError:
            pass
    search_pair(r, eng, a, b, "whole clouds")
    for which in (SL, SR, SS, P0, P1):
        r.check(missing(eng, which), f"whole clouds, first search: {NAMES[which]} is claimed")
    eng.drop_caches()
    found = check_left(r, eng, (a, b), "after drop_caches", (P0, P1))
    r.check(G0 not in found and G1 not in found, "the grid is claimed after pccm_drop_caches")
    eng.set_shard(1, 3)
    eng.nn(nat.DIR_LEFT, "grid")
    check_left(r, eng, (a, b), "shard LEFT", (SL, G1))
    eng.nn(nat.DIR_SELF, "grid")                            # its shard is sorted into the same scratch
    found = check_left(r, eng, (a, b), "shard SELF", (SS, G0))
    r.check(SL not in found, "shard LEFT is claimed after a later sort overwrote the scratch")
    eng.set_shard(0, 1)
    eng.drop_caches()
    eng.nn_pair("grid")
    eng.graph_begin()
    eng.drop_caches()
    eng.nn_pair("grid")
    try:
        eng.build_plan(G0)
        r.check(False, "pccm_build_plan answered during graph capture")
    except nat.PccmStateError:
        pass
    eng.graph_abort()
    r.check(missing(eng, G0) and missing(eng, G1), "the grid of an abandoned capture, which never ran, is claimed")
    eng.nn_pair("grid")
    eng.graph_begin()
    eng.drop_caches()
    eng.nn_pair("grid")
    gid = eng.graph_end()
    found = check_left(r, eng, (a, b), "captured build", (G0, G1))
    for which in (G0, G1):
        if which in found:
            r.check(found[which]["plan"]["read_sp"] == 1, f"captured build: {NAMES[which]} did not read the spatial order")
    for k in range(2):
        eng.graph_launch(gid)
        check_left(r, eng, (a, b), f"replay {k}", (G0, G1))
    eng.graph_destroy(gid)


# ---- under switches ---------------------------------------------------------------------------------------------------------
def row_tile256(r, eng):
    found = search_pair(r, eng, uniform(20_011, 121), uniform(19_997, 122), "20011+19997")
    for which, f in found.items():
        p = f["plan"]
        r.check(p["tile_rows"] == 256 and p["tiles"] == -(-p["n"] // 256) and p["tiles"] > p["nbin"],
                f"{NAMES[which]}: {p['tiles']} tiles of {p['tile_rows']} rows, {p['nbin']} bins")
    found = search_pair(r, eng, uniform(300_007, 123), uniform(1000, 124), "300007+1000")
    if G0 in found:
        p = found[G0]["plan"]
        r.check(p["tile_rows"] > 256 and p["tiles"] < 1024 and p["tiles"] == -(-p["n"] // p["tile_rows"]),
                f"the tile cap: {p['tiles']} tiles of {p['tile_rows']} rows")


def row_scan(r, eng):
    found = search_pair(r, eng, uniform(3001, 131), uniform(2999, 132), "3001+2999")
    for which, f in found.items():
        p = f["plan"]
        r.check(p["scan"] == 1 and p["scan_tiles"] == 1, f"{NAMES[which]}: scan {p['scan']}, {p['scan_tiles']} scan tiles")
    for f64 in (False, True):
        found = search_pair(r, eng, uniform(100_003, 133, f64), uniform(99_001, 134, f64), f"100003+99001 f64={f64}")
        for which, f in found.items():
            p = f["plan"]
            r.check(p["scan"] == 1 and p["scan_tiles"] >= 2 and p["rec32"] == (0 if f64 else 1),
                    f"f64={f64}: {NAMES[which]}: scan {p['scan']}, {p['scan_tiles']} scan tiles: the look-back has no predecessor")
            r.info[f"scan/{int(f64)}/{which}"] = [p["nbin"], p["tiles"], p["scan_tiles"]]


# the smallest thin-shell pair found (bisection between 90 000 and 130 000 points, to within 250) whose grid has more than 512
# bins: 100 312 points give 81^3 = 531 441 cells, 519 bins of 2^10; 100 156 give 80^3 cells, 500 bins
SHELL_N = 100_312


def shell(n, seed):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return (0.5 + 0.45 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def row_threads256(r, eng):
    found = search_pair(r, eng, shell(SHELL_N, 141), shell(SHELL_N - 4, 142), "shell")
    for which, f in found.items():
        p = f["plan"]
        r.info[f"shell/{which}"] = [p["ncells"], p["lg"], p["nbin"]]
        r.check(p["nbin"] > 512, f"{NAMES[which]}: {p['nbin']} bins: the loop behind the two prefetched toff words did not run")


ROWS = {
    "quads_f32": ("", lambda r, e: row_quads(r, e, False)),
    "quads_f64": ("", lambda r, e: row_quads(r, e, True)),
    "tiles_f32": ("", lambda r, e: row_tiles(r, e, False)),
    "tiles_f64": ("", lambda r, e: row_tiles(r, e, True)),
    "faces": ("", row_faces),
    "trimmed": ("", row_trimmed),
    "streamed": ("", row_streamed),
    "planted_bins": ("", row_planted_bins),
    "bitmaps": ("", row_bitmaps),
    "spatial_4095": ("", lambda r, e: row_spatial(r, e, 4095)),
    "spatial_4096": ("", lambda r, e: row_spatial(r, e, 4096)),
    "spatial_20011": ("", lambda r, e: row_spatial(r, e, 20_011)),
    "shards_f32": ("", lambda r, e: row_shards(r, e, False)),
    "shards_f64": ("", lambda r, e: row_shards(r, e, True)),
    "solo": ("", row_solo),
    "rebuilds": ("", row_rebuilds),
    "degenerate": ("", row_degenerate),
    "validity": ("", row_validity),
    "tile256": ("tile256", row_tile256),
    "scan": ("scan_tile256", row_scan),
    "threads256": ("threads256", row_threads256),
}


def run_row(rid):
    r = Row(rid)
    eng = nat.Engine(0)
    try:
        ROWS[rid][1](r, eng)
    finally:
        eng.close()
    return {"row": rid, "fail": r.fail, "info": r.info}


if __name__ == "__main__":
    for rid in sys.argv[1:]:
        print(json.dumps(run_row(rid)), flush=True)
