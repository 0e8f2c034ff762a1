"""The variant table: every kernel instantiation of the product library (libpccm.so without DIAG) names either the row of
tests/test_gpu_variants.py that reaches it or why no row can.  The library picks variants from the data and from a few
environment switches it latches once per process, never from the caller, so a row is a seeded data set (plus, where only a
switch reaches a variant, the switch set of a child process) and the kernels pccm_nn_path must report for it.

tests/test_kernel_inventory.py checks this table against the built library on a CPU-only box; tests/test_gpu_variants.py runs
the rows on the GPU (tests/variants_check.py in a child process for the switch sets) against the oracle."""
import numpy as np

# switch sets: one child process each (the switches are latched once per process: never set them in the test process)
ENVS = {
    "": {},
    "brick22": {"PCCM_BRICK": "2,2"},
    "brick22_mid": {"PCCM_BRICK": "2,2", "PCCM_BRICK_CAP": "2600"},
    "brick22_large": {"PCCM_BRICK": "2,2", "PCCM_BRICK_CAP": "3300"},
    "cap_mid": {"PCCM_BRICK_CAP": "2600"},
    "cap_large": {"PCCM_BRICK_CAP": "3300"},
    "build_scan": {"PCCM_BUILD_SCAN": "1"},
}


def _brick(self_, by, bz, pl, n32=True):
    return f"k_brick_query<{'true' if self_ else 'false'}, {by}, {bz}, {pl}, false, 0, {'true' if n32 or self_ else 'false'}>"


def _bricks(by, bz, pl):
    """The three brick kernels of one shape and plane: pair search with fp32-exact normals, with fp64 normals, self search."""
    return [_brick(False, by, bz, pl, True), _brick(False, by, bz, pl, False), _brick(True, by, bz, pl)]


# Rows.  kind "brick": a pair search with fp32-exact fused normals, again with fp64 normals, then the self search; kind "search":
# the pair and the self search of one cloud flavour; kind "reduce": reduction batches of every shape.
#   gen: the data generator (make_pair) and its arguments; env: the switch set; expect: kernels the paths must name
ROWS = {
    # ---- LDS-brick kernel (cooperative path over fp32-exact volumetric clouds) --------------------------------------------
    "brick42_small": dict(kind="brick", env="", gen=dict(n=100_003, m=99_001), expect=_bricks(4, 2, 2176) + ["k_grid_tail<pccm::Rec32, false>", "k_grid_tail<pccm::Rec32, true>"]),
    "brick42_mid": dict(kind="brick", env="cap_mid", gen=dict(n=100_003, m=99_001), expect=_bricks(4, 2, 3008)),
    "brick42_large": dict(kind="brick", env="cap_large", gen=dict(n=100_003, m=99_001), expect=_bricks(4, 2, 3584)),
    "brick44_small": dict(kind="brick", env="", gen=dict(n=160_001, m=150_007, shard=(1, 2)), expect=_bricks(4, 4, 2176)),
    "brick44_mid": dict(kind="brick", env="cap_mid", gen=dict(n=160_001, m=150_007, shard=(1, 2)), expect=_bricks(4, 4, 3008)),
    "brick44_large": dict(kind="brick", env="cap_large", gen=dict(n=160_001, m=150_007, shard=(0, 2)), expect=_bricks(4, 4, 3584)),
    "brick22_small": dict(kind="brick", env="brick22", gen=dict(n=100_003, m=99_001), expect=_bricks(2, 2, 2176)),
    "brick22_mid": dict(kind="brick", env="brick22_mid", gen=dict(n=100_003, m=99_001), expect=_bricks(2, 2, 3008)),
    "brick22_large": dict(kind="brick", env="brick22_large", gen=dict(n=100_003, m=99_001), expect=_bricks(2, 2, 3584)),
    # unequal sizes: more staged records per brick of the denser cloud, from the data alone
    "brick42_unequal": dict(kind="brick", env="", gen=dict(n=240_007, m=40_009), expect=[_brick(False, 4, 2, 3584), _brick(False, 4, 2, 3584, False)]),
    # ---- the other query kernels ----------------------------------------------------------------------------------------
    # (these rows run seeded random clouds; what the stop rule of k_grid_query*, k_brick_query and k_grid_tail must settle, must
    # not settle and must hand to the exact rescan, query by query and count by count, and the thread-per-query half of
    # k_grid_tail behind a tail list longer than 2^18: tests/test_gpu_grid_planted.py)
    # fp64 volumetric clouds (not fp32-exact): the cooperative kernel on GridRec records, tails on GridRec
    "coop_f64": dict(kind="search", env="", gen=dict(n=200_001, m=190_003, f64=True),
                     expect=["k_grid_query_coop<false>", "k_grid_query_coop<true>", "k_grid_tail<pccm::GridRec, false>",
                             "k_grid_tail<pccm::GridRec, true>"]),
    # ... and their grid built by round 2's histogram + look-back scan (PCCM_BUILD_SCAN=1) instead of the bin cursors
    "build_scan_f64": dict(kind="search", env="build_scan", gen=dict(n=200_001, m=190_003, f64=True, seed=2),
                           expect=["k_bin_count<false, false>", "k_scan_lookback", "k_bin_scatter<pccm::GridRec, false, false>",
                                   "k_grid_query_coop<false>"]),
    # surfaces (fewer than 40 points per x-row): the per-thread kernel, fp32-exact or not
    "thread_rec32": dict(kind="search", env="", gen=dict(n=60_001, m=58_007, surface=True),
                         expect=["k_grid_query<pccm::Rec32, false>", "k_grid_query<pccm::Rec32, true>"]),
    "thread_gridrec": dict(kind="search", env="", gen=dict(n=60_001, m=58_007, surface=True, f64=True),
                           expect=["k_grid_query<pccm::GridRec, false>", "k_grid_query<pccm::GridRec, true>"]),
    # integer clouds: voxel bricks (compact box) and the lattice kernel (a box the voxel bricks do not cover)
    "vox": dict(kind="search", env="", gen=dict(n=50_000, m=50_000, voxel=True),
                expect=["k_vox_query<false, true>", "k_vox_query<true, false>"]),
    "vox_norows": dict(kind="search", env="", want_idx=False, gen=dict(n=50_000, m=50_000, voxel=True, seed=1),
                       expect=["k_vox_query<false, false>"]),
    "lattice": dict(kind="search", env="", gen=dict(n=40_000, m=40_000, voxel=True, spread=True),
                    expect=["k_lattice_query<false>", "k_lattice_query<true>"]),
    # the brute-force engine: fp32 scan, fp64 refine, exact rescan of what it could not certify (what the certificate must flag and
    # must not flag, row by row: tests/test_gpu_brute_planted.py)
    "brute": dict(kind="search", env="", engine="brute", gen=dict(n=20_011, m=19_997, ties=True),
                  expect=["k1_scan<8, false>", "k1_scan<8, true>", "k2_refine<false>", "k2_refine<true>", "k2b_fallback<false>",
                          "k2b_fallback<true>"]),
    # a tie-heavy 20k pair on the grid engine (per-thread kernel: ~34 points per x-row; the clump would send "auto" to the brute
    # engine), witnessed by tests/nn_reference.py as well
    "ties_grid": dict(kind="search", env="", engine="grid", gen=dict(n=20_011, m=19_997, ties=True), expect=["k_grid_query<pccm::Rec32, false>"]),
    # ties="mean": the virtual neighbours and the tie exposure, per record layout
    "ties_rec32": dict(kind="ties", env="", gen=dict(n=20_011, m=19_997, ties=True),
                       expect=["k_tie_mean<pccm::Rec32>", "k_tie_exposure<pccm::Rec32>"]),
    "ties_gridrec": dict(kind="ties", env="", gen=dict(n=20_011, m=19_997, ties=True, f64=True),
                         expect=["k_tie_mean<pccm::GridRec>", "k_tie_exposure<pccm::GridRec>"]),
    # ---- reductions: every k_unit_lean shape kLeanShapes (pccm_reduce_shape.h) lists, and the general kernel -----------
    "reduce_shapes": dict(kind="reduce", env="", gen=dict(n=8192 * 8 + 127, m=8192 * 7 + 129,
                                                        lengths=[(8192 * 8 + 127, 8192 * 7 + 129), (8192 * 8, 8192 * 7 + 1),
                                                                 (8192 * 8 - 1, 128 * 40), (8192 + 128, 8191), (128 * 41 + 1, 127 * 41)]),
                          expect=["k_unit_lean<1, 1, 0>", "k_unit_lean<2, 0, 0>", "k_unit_lean<2, 1, 0>", "k_unit_lean<2, 2, 0>",
                                  "k_unit_lean<4, 0, 0>", "k_unit_lean<4, 1, 0>", "k_unit_lean<4, 2, 0>", "k_unit_lean<2, 0, 1>",
                                  "k_unit_lean<2, 2, 1>", "k_unit_lean<2, 0, 2>", "k_unit_lean<2, 2, 2>", "k_unit_lean<2, 1, 3>",
                                  "k_unit_lean<2, 0, 4>", "k_unit_lean<2, 2, 4>", "k_unit_lean<2, 0, 5>", "k_unit_lean<2, 2, 5>",
                                  "k_unit_jobs"]),
}

# Instantiations no row reaches, and why.  Kernels outside the selectable families (ingest, grid build, colour, normals,
# extent, publish ...) are listed with the suite that runs them: they have one variant each, or their variant follows from
# the row layout the search families above already pin.
UNREACHABLE = {
    "k1_scan<4, false>": "4-query tiles exist for PCCM_SCAN_QT=4, a switch only diagnostic builds read",
    "k1_scan<4, true>": "4-query tiles exist for PCCM_SCAN_QT=4, a switch only diagnostic builds read",
    "k_unit_lean<2, 1, 1>": "a lone D1 column of matched records is always 'distances only' (defer 3); a D2 column only joins it as column 1",
    "k_unit_lean<2, 1, 2>": "a lone D1 column of matched records is always 'distances only' (defer 3); a D2 column only joins it as column 1",
}

OTHER = {
    # grid build <fp32 records, bin cursors (else round 2's look-back scan)>; the fp64 look-back build has row 'build_scan_f64'
    "k_bin_count<false, true>": "grid build of fp64 clouds: rows 'coop_f64', 'thread_gridrec'; what the build leaves, structure by structure: test_gpu_gridbuild",
    "k_bin_count<true, false>": "look-back scan build of fp32 clouds: test_gpu_ab_paths (PCCM_BUILD_SCAN=1); test_gpu_gridbuild (its scan rows)",
    "k_bin_count<true, true>": "grid build of fp32 clouds: every fp32 grid row; what the build leaves, structure by structure: test_gpu_gridbuild",
    "k_bin_scatter<pccm::GridRec, false, true>": "grid build of fp64 clouds: rows 'coop_f64', 'thread_gridrec'; records, tiles and shards: test_gpu_gridbuild",
    "k_bin_scatter<pccm::Rec32, true, false>": "look-back scan build of fp32 clouds: test_gpu_ab_paths (PCCM_BUILD_SCAN=1); test_gpu_gridbuild (its scan rows)",
    "k_bin_scatter<pccm::Rec32, true, true>": "grid build of fp32 clouds: every fp32 grid row; records, tiles, shards and the spatial order: test_gpu_gridbuild",
    "k_bin_sort<pccm::GridRec>": "grid build: every fp64 row above; cell starts, records and cursors left at zero: test_gpu_gridbuild",
    "k_bin_sort<pccm::Rec32>": "grid build: every fp32 row above; cell starts, records, bitmaps and cursors left at zero: test_gpu_gridbuild",
    "k_scan_lookback": "look-back scan of the build's histogram: row 'build_scan_f64'; one tile and tiles with predecessors: test_gpu_gridbuild (its scan rows)",
    "k_tie_mean_scan": "ties='mean': test_gpu_ties_mean",
    "k_count_isolated<pccm::Rec32>": "grid scale decision: every fp32 row above",
    "k_count_isolated<pccm::GridRec>": "grid scale decision: every fp64 row above",
    "k_vox_bricks": "voxel bricks: row 'vox'; planted per-voxel rows, tiles of more than 4096 records: test_gpu_vox_planted.py",
    "k_vox_list": "voxel bricks: row 'vox'; grids of 1 .. 2.2M cells (several words per thread): test_gpu_vox_planted.py",
    "k_ingest_points<float>": "every fp32 row",
    "k_ingest_points<double>": "every fp64 row",
    "k_ingest_normals<float>": "every row with fp32-exact normals",
    "k_ingest_normals<double>": "every row with fp64 normals",
    "k_color_rows<true>": "colours, the packed byte tables: test_gpu_color, test_gpu_color_planted (the byte decision, mixed pairs)",
    "k_color_rows<false>": "colours as doubles: test_gpu_color, test_gpu_color_planted (off-byte values, NaN and inf)",
    "k_colors_from_u8": "colours: test_gpu_color, test_gpu_color_planted (uchar beside double clouds)",
    "k_colsum_approx": "colours: test_gpu_color, test_gpu_color_planted (planted columns, two jobs of unequal chunk counts, maxima)",
    "k_colsum_chain": "colours: test_gpu_color, test_gpu_color_planted (planted columns, two jobs of unequal chunk counts, maxima)",
    "k_colsum_units": "colours: test_gpu_color, test_gpu_color_planted (planted columns, two jobs of unequal chunk counts)",
    "k_rgb8_pack": "colours: test_gpu_color, test_gpu_color_planted (values one ulp off, -0.0, out of range, NaN; kind changes)",
    "k_axis_hist": "box trimming: test_gpu_edges",
    "k_cell_hist": "grid scale decision: every grid row",
    "k_count_occupied": "grid scale decision: every grid row",
    "k_extreme_rows": "extent: test_gpu_extent_kernels (planted extremes, the fp32 bound), test_extent",
    "k_outside_planes": "extent: test_gpu_extent_kernels (exact integer plane tests), test_extent",
    "k_obb_frames": "extent: test_gpu_extent_kernels (one frame at a time, exact ties, whole hulls), test_extent",
    "k_knn_cov_wave": "k-NN search, a wave per point: test_gpu_normals (normals), test_gpu_pointssim_features, test_gpu_p2d (lists)",
    "k_knn_normals": "k-NN search, a thread per point: test_gpu_normals (normals), test_gpu_pointssim_features, test_gpu_p2d (lists)",
    "k_knn_normals_full": "k-NN search, full scan: test_gpu_normals (normals), test_gpu_pointssim_features, test_gpu_p2d (lists)",
    "k_normals_from_cov": "normal estimation, the eigenvectors of the wave search's covariances: test_gpu_normals",
    "k_ssim_curvature": "PointSSIM curvatures from the neighbour lists: test_gpu_pointssim, test_gpu_pointssim_features",
    "k_ssim_features": "PointSSIM features, one launch per attribute: test_gpu_pointssim, test_gpu_pointssim_features",
    "k_p2d_geometry": "point-to-distribution, the Mahalanobis column: test_gpu_p2d",
    "k_p2d_color": "point-to-distribution, the colour and joint columns: test_gpu_p2d_color",
    "k_carry_count": "carried normals, rows per target: test_gpu_carry; colour averages of merged duplicates: test_gpu_merge",
    "k_carry_place": "carried normals, list segments and the queue of long lists: test_gpu_carry, test_gpu_merge",
    "k_carry_scatter_walk": "carried normals, short lists filled and long lists walked in one launch: test_gpu_carry, test_gpu_merge",
    "k_carry_sum": "carried normals, short lists summed in row order and fallback rows: test_gpu_carry, test_gpu_merge",
    "k_merge_probe<false>": "merged duplicates, the insert into the table of representatives: test_gpu_merge",
    "k_merge_probe<true>": "merged duplicates, every row's representative and the waves' masks: test_gpu_merge",
    "k_merge_scan_waves": "merged duplicates, the ordered scan over waves of rows: test_gpu_merge",
    "k_merge_scan_top": "merged duplicates, the ordered scan over groups of 64 waves: test_gpu_merge",
    "k_merge_gather": "merged duplicates, the map and the merged rows: test_gpu_merge",
    "k_point_jobs": ("per-point columns formed from a search result, and nothing else -- unfused point-to-plane columns: row "
                     "'reduce_shapes'; per-point projections (pccm_point_metric): the 'brick' rows, test_gpu_round2, "
                     "test_gpu_point_columns; error vectors (pccm_error_vectors): test_gpu_parity, test_gpu_point_columns; angular "
                     "and PointSSIM similarity columns: test_gpu_angular, test_gpu_pointssim"),
    "k_publish": "every reduction batch",
    "k_unpack": "plain columns from result records: every row",
}


def rows_naming(kernel):
    return [rid for rid, r in ROWS.items() if kernel in r["expect"]]


def _unit(n, seed, f64=False):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v if f64 else v.astype(np.float32)


SLAB = (0.31, 0.42)      # z range left empty in both volumetric clouds: empty bricks
WORKGROUP_MAX = 1024     # threads of the brick kernel's largest workgroup
LDS_RECORDS_MAX = 3580   # records the largest LDS plane stages (kPlaneLarge - 4)


def _dyadic_off_slab(rng, t):
    """t points on the 1/64 lattice inside [0.125, 0.875)^3, none in the empty slab."""
    p = rng.integers(8, 56, size=(t, 3)) / 64.0
    bad = (p[:, 2] > SLAB[0] - 0.02) & (p[:, 2] < SLAB[1] + 0.02)
    p[bad, 2] = 0.75
    return p


def make_pair(n, m, seed=0, f64=False, surface=False, voxel=False, spread=False, ties=False):
    """Two clouds of n and m points with the edges these kernels get wrong, each in rows of its own:
      a[qc]  a clump of queries, more than a brick's workgroup holds (n >= 60k)
      b[sc]  a clump of searched points, more than any LDS plane stages (m >= 60k)
      a[xr], b[xr]  long x-runs: points along one row of cells
      a[tb]  tie bases on the 1/64 lattice, b[tp] four points at exactly 1/4096 from each: distinct points at one distance
      b[du]  duplicates of other rows of b: equal points at different rows
      a[fq]  queries that variants_check.place_faces() puts exactly on the grid's cell faces (org + k h, in the cloud's dtype)
      holes in both clouds: queries there have their neighbour beyond ring 1; an empty z slab: empty bricks
      ties=True: a[-2 du:] two copies of b[du]'s sources: exact ties in the other direction too.
    Returns (a, b, rows): rows maps each edge to its rows (slices)."""
    rng = np.random.default_rng(1000 + seed + n + 7 * m)
    rows = {}
    if voxel:
        scale = 3000.0 if spread else 120.0
        v = rng.standard_normal((3 * n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        a = np.unique(np.round(scale + scale * 0.8 * v), axis=0)[:n]
        b = np.unique(np.round(a + rng.normal(0, 0.7, a.shape)), axis=0)[:m]
        if spread:                                    # a second blob far away: a box the voxel bricks do not cover
            a[: len(a) // 8] += 40_000.0
            b[: len(b) // 8] += 40_000.0
        return a.astype(np.float32), b.astype(np.float32), rows
    dt = np.float64 if f64 else np.float32
    if surface:
        def sph(k):
            v = rng.standard_normal((k, 3))
            return 0.5 + 0.45 * v / np.linalg.norm(v, axis=1, keepdims=True)
        a, b = sph(n), sph(m)
    else:
        a, b = rng.random((n, 3)), rng.random((m, 3))
        for pts in (a, b):                            # empty slab
            inside = (pts[:, 2] > SLAB[0]) & (pts[:, 2] < SLAB[1])
            pts[inside, 2] += SLAB[1] - SLAB[0] + 0.01
        for pts, c in ((b, (0.7, 0.7, 0.7)), (a, (0.25, 0.7, 0.2))):     # holes
            far = np.linalg.norm(pts - np.array(c), axis=1) < 0.15
            pts[far] = rng.random((int(far.sum()), 3)) * 0.2 + 0.05
    # disjoint rows for the edges
    def take(arr_rows, size):
        lo = arr_rows[0]
        arr_rows[0] += size
        return slice(lo, lo + size)
    ca, cb = [0], [0]
    t = min(2000, n // 20, m // 20)
    nd = min(1000, m // 20)
    if not surface:
        if n >= 60_000:
            rows["qc"] = take(ca, 3000)
        if m >= 60_000:
            rows["sc"] = take(cb, 4000)
        r = min(3000, n // 20, m // 20)
        rows["xr_a"], rows["xr_b"] = take(ca, r), take(cb, r)
    rows["tb"], rows["fq"] = take(ca, t), take(ca, t)
    rows["tp"] = slice(m - 4 * t, m)
    rows["du"] = slice(m - 4 * t - nd, m - 4 * t)
    rows["du_src"] = take(cb, nd)
    if ties:
        rows["tie_a"] = slice(n - 2 * nd, n)
    assert ca[0] <= (n - 2 * nd if ties else n) and cb[0] <= rows["du"].start, "edge rows overlap"
    if "qc" in rows:
        a[rows["qc"]] = 0.55 + rng.random((3000, 3)) * 0.004
    if "sc" in rows:
        b[rows["sc"]] = 0.55 + rng.random((4000, 3)) * 0.004
    if "xr_a" in rows:
        k = rows["xr_a"].stop - rows["xr_a"].start
        a[rows["xr_a"]] = np.c_[rng.random(k), np.full(k, 0.5), np.full(k, 0.125)]
        b[rows["xr_b"]] = np.c_[rng.random(k), np.full(k, 0.5), np.full(k, 0.1875)]
    base = _dyadic_off_slab(rng, t)
    a[rows["tb"]] = base
    a[rows["fq"]] = _dyadic_off_slab(rng, t)          # (place_faces moves them onto faces)
    d = 1.0 / 4096
    for ax, sgn, off in ((0, 1, 0), (0, -1, 1), (1, 1, 2), (2, -1, 3)):
        p = base.copy()
        p[:, ax] += sgn * d
        b[m - (off + 1) * t:m - off * t] = p
    b[rows["du"]] = b[rows["du_src"]]
    if ties:
        a[n - nd:] = b[rows["du_src"]]
        a[n - 2 * nd:n - nd] = b[rows["du_src"]]
    a, b = a.astype(dt), b.astype(dt)
    check_edges(a, b, rows)
    return a, b, rows


def check_edges(a, b, rows):
    """Every edge the rows claim is in the data (face queries: variants_check.place_faces checks them on the grid)."""
    if "qc" in rows:
        q = a[rows["qc"]]
        assert len(q) > WORKGROUP_MAX and np.ptp(q, axis=0).max() < 0.005, "query clump"
    if "sc" in rows:
        s = b[rows["sc"]]
        assert len(s) > LDS_RECORDS_MAX and np.ptp(s, axis=0).max() < 0.005, "searched clump"
    if "xr_a" in rows:
        assert len(np.unique(a[rows["xr_a"]][:, 1:], axis=0)) == 1 and rows["xr_a"].stop - rows["xr_a"].start >= 100, "x-run"
    base = a[rows["tb"]].astype(np.float64)
    tp = b[rows["tp"]].astype(np.float64).reshape(4, -1, 3)
    dist = np.stack([np.sum((tp[k] - base) ** 2, axis=1) for k in range(4)])
    assert np.all(dist == (1.0 / 4096) ** 2), "four searched points at one distance from every tie base"
    du, src = b[rows["du"]], b[rows["du_src"]]
    assert len(du) > 0 and np.array_equal(du, src), "duplicate rows"
    if "xr_a" in rows:                                 # volumetric: the slab is empty
        for pts in (a, b):
            assert not np.any((pts[:, 2] > SLAB[0]) & (pts[:, 2] < SLAB[1])), "empty slab"
