/*
 * pccm.h -- C ABI of libpccm.so, the MI355X (gfx950) engine under open_pcc_metric_amd.
 *
 * The reference (aaletov/open-pcc-metric v0.1.2) is pure Python over the open3d wheel and has
 * no C ABI / FFI of its own; its "operator interface" for this path is the Python object
 * protocol of open_pcc_metric/cloud_pair.py.  Each entry point below names the reference
 * interface it stands under (paths relative to the reference checkout).  The Python binding a
 * maintainer would add is shown in INTEGRATION.md (ctypes, ~40 lines).
 *
 * Conventions
 *   - every function returns PCCM_OK (0) or a negative PCCM_E_* code; the message of the last
 *     failure on the calling thread is pccm_last_error().  No C++ exception crosses the ABI.
 *   - point/normal arrays are packed row-major [n][3], dtype PCCM_F32 or PCCM_F64, in host
 *     memory (on_device = 0) or device memory of the context's GPU (on_device = 1).  The
 *     library copies what it needs; callers keep ownership of everything they pass in or out.
 *   - cloud 0 = origin cloud ("A"), cloud 1 = reconstructed cloud ("B")  (cloud_pair.py:54-59).
 *   - direction PCCM_DIR_LEFT iterates A and searches B (cloud_pair.py:67-72), PCCM_DIR_RIGHT
 *     iterates B and searches A (cloud_pair.py:73-78), PCCM_DIR_SELF iterates A and searches A
 *     for the nearest point with a different row index (cloud_pair.py:108-109).
 *   - a context serves one caller at a time: every entry point holds the context's (recursive) mutex for its whole
 *     duration, so threads that share one are serialised, not corrupted; different contexts run concurrently.
 *   - one context drives one GPU.  Multi-GPU = one process (and context) per GPU, each with
 *     pccm_set_shard(rank, world); the only cross-rank data are the small vectors documented at
 *     pccm_reduce(), which the host exchanges with an RCCL all-reduce (DESIGN.md section e).
 */
#ifndef PCCM_H
#define PCCM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCCM_VERSION 100 /* 0.1.0 */

/* error codes */
#define PCCM_OK 0
#define PCCM_E_ARG (-1)    /* bad argument (null, size, non-finite or too large coordinates) -> ValueError */
#define PCCM_E_NODEV (-2)  /* no usable HIP device */
#define PCCM_E_HIP (-3)    /* HIP runtime error */
#define PCCM_E_OOM (-4)    /* device or host allocation failed */
#define PCCM_E_STATE (-5)  /* call order: clouds / normals / nn result not set yet */
#define PCCM_E_RANGE (-6)  /* row index outside the other cloud's normals: the reference's IndexError
                              at metric.py:148-152 */

/* dtypes */
#define PCCM_F32 0
#define PCCM_F64 1

/* directions */
#define PCCM_DIR_LEFT 0
#define PCCM_DIR_RIGHT 1
#define PCCM_DIR_SELF 2

/* nearest-neighbour engines (all exact; they differ only in speed) */
#define PCCM_ENGINE_AUTO 0  /* the grid, unless the pair of clouds is one no uniform grid can separate (clumps, partial overlap) */
#define PCCM_ENGINE_BRUTE 1 /* LDS-tiled fp32 scan + fp64 certification/refine */
#define PCCM_ENGINE_GRID 2  /* uniform-grid ring search */

/* which normal row the D2 projection uses */
#define PCCM_NORMAL_ROW 0       /* row i of the other cloud (what the reference does, metric.py:130,148-152) */
#define PCCM_NORMAL_NEIGHBOUR 1 /* row nn(i) of the other cloud */

/* per-point quantities */
#define PCCM_METRIC_D1 0   /* EuclideanDistance(point_to_plane=False): squared NN distance, metric.py:175-177 */
#define PCCM_METRIC_D2 1   /* EuclideanDistance(point_to_plane=True): projection squared, metric.py:179 */
#define PCCM_METRIC_PROJ 2 /* ErrorVector(point_to_plane=True): signed projection, metric.py:146-153 */
/* Plane-to-plane angular similarity (Alexiou & Ebrahimi, ICME 2018) of directions 0 and 1 (the self search: PCCM_E_ARG).
 * a = the iterating cloud's normal of row i, b = the searched cloud's normal of the MATCHED row nn(i) -- normal_mode does not
 * apply and is ignored -- both fp64, every operation separately rounded (no FMA):
 *   dot = (a0*b0 + a1*b1) + a2*b2,  na2 = (a0*a0 + a1*a1) + a2*a2,  nb2 likewise,  den = sqrt(na2 * nb2)
 *   s   = 0                                    if den == 0 (a zero-length normal counts as perpendicular)
 *   s   = 1 - (2 * acos(c)) / M_PI             otherwise, c = min(|dot| / den, 1)
 * s is 1 for parallel and antiparallel normals (estimated normals are unoriented), 0 for perpendicular ones.  Under
 * PCCM_TIES_MEAN the value of row i is the mean of s over its tie set, (((s_j1 + s_j2) + s_j3) + ...) / k (not s of the averaged
 * normal: unoriented normals of opposite sign would cancel).  Both clouds need normals (PCCM_E_STATE otherwise).  Accepted by
 * pccm_point_metric and every pccm_reduce* call; a plain column, reduced like D1. */
#define PCCM_METRIC_ANGULAR 3
/* PointSSIM similarity (Alexiou & Ebrahimi, ICME Workshops 2020) of one attribute, directions 0 and 1 (the self search:
 * PCCM_E_ARG).  F = the feature columns pccm_ssim_features made, a = F_it(i), b = F_se(nn(i)) of the MATCHED row (normal_mode
 * does not apply and is ignored), every operation separately rounded:
 *   s = 1 - |a - b| / (max(|a|, |b|) + 2^-52)
 * PCCM_E_STATE unless both clouds hold that attribute's features at the same k, and under PCCM_TIES_MEAN.  Accepted by
 * pccm_point_metric and every pccm_reduce* call; a plain column, reduced like D1. */
#define PCCM_METRIC_SSIM_GEOMETRY 4
#define PCCM_METRIC_SSIM_NORMAL 5
#define PCCM_METRIC_SSIM_CURVATURE 6
#define PCCM_METRIC_SSIM_COLOR 7
/* Point-to-distribution value M (pccm_p2d_build) of directions 0 and 1 (the self search: PCCM_E_ARG): the stored column of the
 * direction, which depends on neither the matched rows nor the tie policy; normal_mode is ignored.  PCCM_E_STATE while the
 * columns are not built.  Accepted by pccm_point_metric and every pccm_reduce* call; a plain column, reduced like D1 (the
 * direction needs a search result, like every reduction: the slot takes its row range and generation from it). */
#define PCCM_METRIC_P2D 8
/* The colour value M_Y and the joint value M_J of pccm_p2d_build_attrs (PCCM_P2D_COLOR): stored columns exactly like
 * PCCM_METRIC_P2D, with the same rules; PCCM_E_STATE while they are not built (a geometry-only build, or new colours since). */
#define PCCM_METRIC_P2D_COLOR 9
#define PCCM_METRIC_P2D_JOINT 10
/* The point spacings r (pccm_resolution_build) of the cloud the direction ITERATES: direction 0 reads cloud 0's column, direction
 * 1 cloud 1's (the self search: PCCM_E_ARG).  A stored column exactly like PCCM_METRIC_P2D: neither the matched rows, the tie
 * policy nor normal_mode enter it, and the direction needs a search result (the slot takes its row range and generation from
 * it).  PCCM_E_STATE while that cloud's column is not built.  Accepted by pccm_point_metric and every pccm_reduce* call; a plain
 * column, reduced like D1. */
#define PCCM_METRIC_RESOLUTION 11
/* Squared reflectance error of directions 0 and 1 (the self search: PCCM_E_ARG).  a = the iterating cloud's reflectance of row i,
 * b = the searched cloud's reflectance of the MATCHED row nn(i) -- normal_mode does not apply and is ignored -- both fp64 with the
 * values as given (pccm_set_reflectance*), each operation separately rounded:
 *   d = a - b,  val = d * d
 * PCCM_E_STATE unless both clouds hold one reflectance per point, and under PCCM_TIES_MEAN.  Accepted by pccm_point_metric and
 * every pccm_reduce* call; a plain column, reduced like D1. */
#define PCCM_METRIC_REFLECTANCE 12

/* kernel classes for pccm_profile_get() */
#define PCCM_K_INGEST 0
#define PCCM_K_SCAN 1     /* brute-force fp32 scan (dominant kernel of PCCM_ENGINE_BRUTE) */
#define PCCM_K_REFINE 2   /* fp64 certification + winner refine */
#define PCCM_K_FALLBACK 3 /* exact rescan of flagged queries (uncertified fp32 winners; queries the grid's rings left open) */
#define PCCM_K_POINT 4    /* fused gather + error vector + projection */
#define PCCM_K_REDUCE 5   /* leaf sums / max / min */
#define PCCM_K_GRID_BUILD 6
#define PCCM_K_GRID_QUERY 7  /* k_grid_query_coop: ring 1 of both directions (dominant kernel of PCCM_ENGINE_GRID) */
#define PCCM_K_GRID_FINISH 8 /* k_grid_tail: rings 2..3 of the unsettled queries + the exact rescan of what they leave */
#define PCCM_K_COUNT 9

typedef struct pccm_ctx pccm_ctx;

int pccm_version(void);
const char *pccm_last_error(void);

/* Number of HIP devices visible to the process (0 and PCCM_OK when there is none). */
int pccm_device_count(int *n);

/* Create a context on `device`.  `hip_stream` may be NULL (the library creates its own
 * non-blocking stream) or a hipStream_t the caller owns (e.g. torch's current stream). */
int pccm_ctx_create(int device, void *hip_stream, pccm_ctx **out);
int pccm_ctx_destroy(pccm_ctx *ctx);
/* Back to the state after pccm_ctx_create -- no clouds, shard 0 of 1, no graphs, profiling off -- but with every
 * device allocation (and the grid decisions a look-alike pair may inherit) kept: for callers that run one pair
 * after the other through the same context instead of paying context teardown and fresh allocations per pair. */
int pccm_ctx_reset(pccm_ctx *ctx);

/* Replaces CloudPair.__init__'s capture of the two clouds, cloud_pair.py:54-59.
 * Coordinates must be finite with |x| <= 1e15.  Invalidates earlier nn results. */
int pccm_set_cloud(pccm_ctx *ctx, int which, const void *xyz, int64_t n, int dtype, int on_device);

/* Replaces np.asarray(cloud.normals), metric.py:92-98.  n must equal the cloud's point count
 * for PCCM_NORMAL_NEIGHBOUR; PCCM_NORMAL_ROW only needs the rows it indexes. */
int pccm_set_normals(pccm_ctx *ctx, int which, const void *nrm, int64_t n, int dtype, int on_device);

/* The same for HOST normals, announced now and uploaded later: the library notes the pointer (the array must stay alive and
 * unchanged until pccm_flush_uploads returns or another call replaces the cloud or its normals) and moves the data when a
 * call needs it -- or at pccm_flush_uploads -- on a copy stream of its own.  Searches whose results are matched records never
 * read normals, so a caller that announces, starts the searches and then flushes has the upload run beside them:
 * handler.py:57-58 of the reference reads both files, then cloud_pair.py:61-80 does everything else; nothing in it orders the
 * normals before the searches.  Non-finite normals are reported by the call that uploads them (PCCM_E_ARG), not by this one. */
int pccm_set_normals_deferred(pccm_ctx *ctx, int which, const void *nrm, int64_t n, int dtype);
int pccm_flush_uploads(pccm_ctx *ctx);

/* How arrays of the CALLER cross PCIe (uploads of clouds, normals, colours; downloads of rows, distances, normals ...).
 * off (default; pccm_ctx_reset restores it): handed to the HIP runtime as they are -- which pins the caller's pages and keeps the
 * mapping cached: fastest (43 GB/s), but when the caller later FREES such an array the driver evicts and restores every GPU
 * queue of the process, and a kernel that is running stands still for 13-27 ms (measured).
 * on: through pinned buffers of the context's own, copied by a few host threads (25 GB/s): for callers that load, use and
 * free their clouds in a loop (CloudPair.with_reconst, evaluate_pairs with loader items, the command line with several
 * --pcloud).  No counterpart in the reference. */
int pccm_set_io_staged(pccm_ctx *ctx, int on);

/* Replaces clouds[k].estimate_normals(), cloud_pair.py:61-64 (Open3D EstimateNormals, default
 * KDTreeSearchParamKNN(knn = 30)): per point, the eigenvector of the smallest eigenvalue of the
 * covariance of its knn nearest points of the same cloud (itself included).  Open3D's own arithmetic
 * and sign convention cannot be pinned without it; here the component of largest
 * magnitude is positive.  The normals stay on the device; pccm_get_normals copies [n][3] doubles out. */
int pccm_estimate_normals(pccm_ctx *ctx, int which, int knn);
int pccm_get_normals(pccm_ctx *ctx, int which, double *out);
/* Carry cloud `from`'s normals over to the other cloud, to = 1 - from, the way MPEG's pc_error gives a decoded cloud the
 * reference's normals (scaleNormals with averageNormals), from the two directional searches the context holds.  F = the search
 * that iterates cloud `from` (PCCM_DIR_LEFT for from = 0), G = the other one; nn_F(i), nn_G(j) = their matched rows under
 * PCCM_TIES_PICK (the smallest row on exact ties).  Per row j of cloud `to`, with S_j = { i : nn_F(i) = j } = i_1 < ... < i_m:
 *   m >= 1: per component in fp64 s = n_from[i_1], then s = s + n_from[i_r] for r = 2..m, every add rounded separately, and
 *           the result s / (double)m, one correctly rounded division (m = 1 gives the source normal back bit for bit, signed
 *           zeros included);
 *   m = 0:  n_from[nn_G(j)], copied bit for bit (a point that is nobody's nearest neighbour takes its own nearest point's).
 * The result is NOT renormalised (as the averaged normals of PCCM_TIES_MEAN are not).  It becomes cloud `to`'s normals on the
 * device exactly as if pccm_estimate_normals had made them: one per point, pending reductions that read normals and captured
 * graphs go stale, pccm_get_normals(to) returns them.  The operation follows pc_error's normal carrying; parity with that program
 * is NOT pinned: it is not available to this project's tests, it sums in single precision, and its tie order is its kd-tree's.
 * *built (may be null) = 1 when work was done, 0 when cloud `to` already holds normals carried from the same two search results
 * and the same source normals -- such a call does nothing and is allowed between pccm_graph_begin and pccm_graph_end.  Carried
 * normals are dropped (cloud `to` has no normals again) when either cloud gets new points or cloud `from` gets new normals;
 * pccm_set_normals* or pccm_estimate_normals on `to` replace them.  A search that ran without matched rows (pccm_nn_want_idx
 * off) is repeated with them.
 * PCCM_E_ARG: from is not 0 or 1.  PCCM_E_STATE: a cloud is missing; cloud `from` has no normal for every row (announced normals
 * are uploaded first); either directional search has no result; a sharded context; PCCM_TIES_MEAN; a build during graph capture. */
int pccm_carry_normals(pccm_ctx *ctx, int from, int *built);
/* Merge the rows of cloud `which` that share their coordinates, in place on the device, the way MPEG's pc_error treats both clouds
 * before any metric (dropDuplicates).  The key of a row is its three fp64 coordinates as stored (an fp32 upload widened exactly),
 * compared with == per component: -0.0 equals +0.0, nothing is quantised or shifted, and two points one ulp apart in one coordinate
 * are distinct.  Rows with equal keys form a group i_1 < ... < i_m with representative i_1.  The merged cloud has one row per group
 * in ascending order of representative (a stable compaction, n' rows); each row holds
 *   the representative's coordinates, bit for bit (its -0.0 survives);
 *   its normal bit for bit, in both modes, when the cloud has one normal per point;
 *   its reflectance, when the cloud has one, by the rule at pccm_set_reflectance;
 *   when the cloud has colours: PCCM_DUP_DROP the representative's colour bit for bit; PCCM_DUP_AVERAGE per component in fp64
 *   s = c[i_1], then s = s + c[i_r] for r = 2..m, every add rounded separately, and the result s / (double)m, one correctly rounded
 *   division (m = 1 gives the colour back bit for bit) -- the convention of pccm_carry_normals.
 * pccm_get_merge_map returns map[i] = the merged row of original row i's group (n entries; multiplicities and representatives
 * follow from it).  The operation follows pc_error's; parity with that program is NOT pinned: it is not available to this
 * project's tests and it averages in its own arithmetic.
 * A cloud without duplicates (n' == n) is left untouched: no array is rewritten, no result goes stale, the map is the identity.
 * Otherwise the context is in the state pccm_set_cloud(which, merged, n', PCCM_F64, on_device) followed by pccm_set_normals /
 * pccm_set_colors with the merged arrays would have left: search results of every direction that touches the cloud, carried
 * normals in either direction, PointSSIM features, point-to-distribution columns, tie lists and pending reductions are gone and
 * captured graphs are stale.  Announced normals (pccm_set_normals_deferred) are uploaded first.  *n_out (may be null) = n'.  The
 * map stays on the device until the cloud gets new points or pccm_ctx_reset; for a cloud that was never merged pccm_get_merge_map
 * returns the identity, and *n_before (may be null) = the rows the map has (`out` may be null to ask for it alone).  The call does
 * not depend on the tie policy.
 * pccm_get_points / pccm_get_colors copy the stored fp64 rows [n][3] out, as pccm_get_normals does.
 * PCCM_E_ARG: which is not 0 or 1; mode is not PCCM_DUP_DROP or PCCM_DUP_AVERAGE.  PCCM_E_STATE: the cloud is missing; it has
 * normals, colours or reflectance whose count is neither 0 nor n; a sharded context; a call between pccm_graph_begin and pccm_graph_end;
 * pccm_get_colors on a cloud without colours. */
#define PCCM_DUP_DROP 1
#define PCCM_DUP_AVERAGE 2
int pccm_merge_duplicates(pccm_ctx *ctx, int which, int mode, int64_t *n_out);
int pccm_get_merge_map(pccm_ctx *ctx, int which, int32_t *out, int64_t *n_before);
int pccm_get_points(pccm_ctx *ctx, int which, double *out);
int pccm_get_colors(pccm_ctx *ctx, int which, double *out);

/* Voxel occupancy of the two resident clouds ("Voxel occupancy"), without any search.
 * For each of n voxel sizes (finite, > 0): out[3*k+0] = occupied voxels of cloud 0, [3*k+1] = of cloud 1, [3*k+2] = occupied by both.
 * Voxel (a, b, c) is [a v, (a+1) v) x ... on the absolute lattice: floor(coordinate / v).
 * The key of a row is floor(c / v) + 0.0 per component of its stored fp64 coordinates: the correctly rounded quotient (never a
 * product with 1 / v), -0.0 folded onto 0.0, kept and compared as doubles -- what np.floor(x / v) gives.  Both clouds' rows go into
 * one open-addressed table per size (the table of pccm_merge_duplicates with this key); every count is an integer and none depends
 * on scheduling.  The sizes run one after the other on the stream and the call waits once.  It keeps nothing in the context,
 * changes no cloud and no result, and does not depend on the tie policy.
 * PCCM_E_ARG: a null pointer; n outside 1..4; a voxel size that is not finite and > 0; clouds of 2^32 - 1 rows or more together.
 * PCCM_E_STATE: a cloud is missing; a sharded context; a call between pccm_graph_begin and pccm_graph_end. */
int pccm_voxel_occupancy(pccm_ctx *ctx, int n, const double *voxels, int64_t *out);

/* PointSSIM features ("PointSSIM") of cloud `which`: per point p, N_k(p) = the k points of the same cloud first
 * in ascending (d2, row) order (p itself included; all of them when the cloud has fewer than k), and per attribute the variance
 * with divisor m - 1 of m values over N_k(p), fp64, sums left to right in neighbourhood order, every operation separately rounded:
 *   PCCM_SSIM_GEOMETRY   distances sqrt(d2(p, q_j)), j >= 1
 *   PCCM_SSIM_NORMAL     PCCM_METRIC_ANGULAR of n_p and n_{q_j}, j >= 1 (needs the cloud's normals)
 *   PCCM_SSIM_CURVATURE  c(q_j) = lambda_min / trace of the covariance of N_k(q_j) (0 for a zero trace), j >= 0
 *   PCCM_SSIM_COLOR      the luma of q_j (first row of transform_colors' "ycc" matrix), j >= 0 (needs the cloud's colours)
 * F = 0 when m < 2.  attrs: a mask of PCCM_SSIM_*; k in 2..64.  The columns stay with the cloud in HBM until its points, normals
 * or colours change; a call whose attributes are already there at the same k does no work (*built = 0, else 1; built may be
 * null).  PCCM_E_STATE when the normals or colours the mask needs are absent. */
#define PCCM_SSIM_GEOMETRY 1
#define PCCM_SSIM_NORMAL 2
#define PCCM_SSIM_CURVATURE 4
#define PCCM_SSIM_COLOR 8
int pccm_ssim_features(pccm_ctx *ctx, int which, int k, int attrs, int *built);
/* one feature column (attr: a single PCCM_SSIM_* flag) of cloud `which`: n doubles */
int pccm_get_ssim_features(pccm_ctx *ctx, int which, int attr, double *out);

/* Point-to-distribution columns ("Point-to-distribution"; after Javaheri et al., IEEE SPL 2020) of directions 0
 * and 1: n_A and n_B doubles in HBM.  Direction A -> B, per point p of A, fp64, every operation separately rounded, sums left
 * to right in the order written:
 *   N    = the k points of B first in ascending (d2, row) order, d2 = ((dx*dx) + (dy*dy)) + dz*dz, d = p - q; all of B when it
 *          has fewer than k points; kk = |N|, q_0, q_1, ... in that order (an exact k-NN search of A's points in B's cells)
 *   e_j  = q_j - p;  S1_a = sum_j e_j,a;  S2_ab = sum_j (e_j,a * e_j,b);  m_a = S1_a / kk;  C_ab = S2_ab / kk - m_a * m_b
 *   t    = (C00 + C11) + C22;  lam = t * 2^-10;  c_aa = C_aa + lam, off-diagonal c_ab = C_ab   (a ridge relative to the trace: flat
 *          neighbourhoods stay invertible, M stays invariant under uniform scaling, cond(c) <= 3 * 2^10 + 1)
 *   f00 = c11*c22 - c12*c12, f01 = c02*c12 - c01*c22, f02 = c01*c12 - c02*c11, f11 = c00*c22 - c02*c02, f12 = c01*c02 - c00*c12,
 *   f22 = c00*c11 - c01*c01;  det = (c00*f00 + c01*f01) + c02*f02;  v_a = (f_a0*m0 + f_a1*m1) + f_a2*m2;
 *   quad = (m0*v0 + m1*v1) + m2*v2;  M(p) = sqrt(max(quad / det, 0))
 *   !(t > 0) or !(det > 0) (all of N is one location):  M(p) = 0 when m0 == m1 == m2 == 0, +inf otherwise
 * k in 4..64 (PCCM_E_ARG).  Needs both clouds and no search result; PCCM_E_STATE for a missing cloud, a sharded context, or a
 * build during graph capture.  A call that finds the columns at the same k does no work (*built = 0, else 1; built may be null)
 * and is allowed during capture.  New points in either cloud drop both columns.  A build makes pending reductions of directions
 * 0 and 1 stale and, when a column moves, captured graphs too.  The pair's grid is rebuilt (as by pccm_ssim_features). */
int pccm_p2d_build(pccm_ctx *ctx, int k, int *built);
/* What pccm_p2d_build_attrs builds (bit flags).  The geometry column is always built; PCCM_P2D_COLOR stands for the colour
 * column and the joint column together. */
#define PCCM_P2D_GEOMETRY 1
#define PCCM_P2D_COLOR 2
/* pccm_p2d_build with a choice of columns (pccm_p2d_build(ctx, k, built) is attrs = PCCM_P2D_GEOMETRY).  PCCM_P2D_COLOR adds, per
 * direction, the colour and the joint column ("Point-to-distribution: colour and joint"; after Javaheri et al.,
 * IEEE MMSP 2021) over exactly the neighbourhood N of the geometry column.  Direction A -> B, p = row i of A, fp64, every
 * operation separately rounded, sums from 0.0 left to right in neighbourhood order:
 *   y(c) = fma(0.0722, c_b, fma(0.2126, c_r, 0.7152 * c_g))   (the luma of PCCM_SSIM_COLOR)
 *   e_j  = y(rgb_B[q_j]) - y(rgb_A[i]);  S1 = sum_j e_j;  S2 = sum_j (e_j * e_j);  m = S1 / kk;  V = S2 / kk - m * m
 *   v    = max(V, 0) + 2^-20;  M_Y(p) = |m| / sqrt(v)  (always finite);  M_J(p) = sqrt(M_G(p) * M_G(p) + M_Y(p) * M_Y(p)),
 *   M_G the geometry column's value (+inf propagates).
 * PCCM_E_ARG for a bad k or unknown attrs bits; PCCM_E_STATE as pccm_p2d_build, and when PCCM_P2D_COLOR is asked for and either
 * cloud has no colours.  A call that finds all requested columns at the same k does no work (*built = 0) and is allowed during
 * capture; one that finds the geometry columns but not the colour columns it asks for builds those (*built = 1) and leaves the
 * geometry columns as they are.  One build runs one k-NN search per direction, whatever the attrs.  New points in either cloud
 * drop all columns; pccm_set_colors / pccm_set_colors_u8 on either cloud drop the colour and joint columns of both directions and
 * keep the geometry columns. */
int pccm_p2d_build_attrs(pccm_ctx *ctx, int k, int attrs, int *built);
/* the neighbourhoods behind direction dir's column: out[n][k] rows of the searched cloud in ascending (d2, row) order (entries
 * from count[i] on are -1), count[n].  Searches again (the build keeps no lists); PCCM_E_STATE while the columns are not built. */
int pccm_get_p2d_neighbours(pccm_ctx *ctx, int dir, int32_t *out, int32_t *count);

/* Point spacings of cloud `which` ("Resolution-adaptive PSNR"; after Javaheri et al., ICIP 2020): r[n] doubles in
 * HBM, the mean distance of every point to its K nearest neighbours in its own cloud.  Per point p, fp64, every operation
 * separately rounded:
 *   N(p) = the first m = min(K + 1, n) points of the cloud in ascending (d2, row) order, d2 = ((dx*dx) + (dy*dy)) + dz*dz on the
 *          stored coordinates: q_0 (distance 0), q_1, ... -- exactly PointSSIM's N_k at k = K + 1
 *   r(p) = (sum_{j = 1 .. m - 1} sqrt(d2(p, q_j))) / (double)(m - 1), the sum from 0.0 left to right in list order (one correctly
 *          rounded square root and one add per entry, then one division);  r(p) = 0 when m < 2.
 * r(p) depends only on the sorted multiset of the m smallest squared distances: equal d2 give equal square roots, so neither
 * the order of exact ties nor which of several tied rows survives the cut at entry K can change a bit of it.  The column
 * therefore does not depend on the row order of the cloud (a permutation of the rows permutes r) nor on the tie policy.
 * The intrinsic resolution of the cloud is np.sum(r) / n (the plain-column reduction of PCCM_METRIC_RESOLUTION).  K = 10 is
 * this project's default; the paper's own choice is not available here and parity with its authors' code is NOT pinned.
 * K in 1..63 (the list has K + 1 entries).  The column stays with the cloud until the cloud gets new points (pccm_set_cloud, a
 * pccm_merge_duplicates that removes rows, pccm_ctx_reset); new normals or colours, and anything that happens to the other
 * cloud, leave it alone.  A call that finds the column at the same K does no work (*built = 0, else 1; built may be null) and is
 * allowed during graph capture.  A build makes pending reductions stale and, when the column moves, captured graphs too; the
 * pair's grid is rebuilt (as by pccm_ssim_features).
 * PCCM_E_ARG: which is not 0 or 1; K outside 1..63.  PCCM_E_STATE: the cloud is missing; a sharded context; a build during graph
 * capture. */
int pccm_resolution_build(pccm_ctx *ctx, int which, int K, int *built);
/* the spacing column of cloud `which`: n doubles (PCCM_E_STATE while it is not built) */
int pccm_get_resolution(pccm_ctx *ctx, int which, double *out);

/* Query-axis shard of this context: rank r of `world` owns, in every direction, the rows
 * [begin, end) of the iterating cloud returned by pccm_shard_range (boundaries are multiples
 * of 8192 rows -- whole chunks of NumPy's sum: pccm_reduce_chunks_many -- when the cloud has a chunk for every rank,
 * else of 128 rows, so that reduction leaves never straddle ranks).  Default: rank 0 of 1. */
int pccm_set_shard(pccm_ctx *ctx, int rank, int world);
/* The same per direction: `world` ranks share the rows of direction `dir` and this context is number `rank` of them;
 * world = 0: this context owns NO rows of that direction (another group of ranks searches it) -- its searches and
 * reductions of `dir` are empty and contribute zeros to the exchange.  Lets the ranks of a node split by DIRECTION
 * first (cloud_pair.py:67-72 on one half, :73-78 on the other), so that every rank builds the search structure of one
 * cloud only. */
int pccm_set_shard_dir(pccm_ctx *ctx, int dir, int rank, int world);
int pccm_shard_range(pccm_ctx *ctx, int dir, int64_t *begin, int64_t *end);

/* Replaces get_neighbour_cloud(), cloud_pair.py:10-42 (and, for PCCM_DIR_SELF, Open3D's
 * compute_nearest_neighbor_distance behind cloud_pair.py:108-109): exact 1-NN of every row
 * of the shard, squared L2 distance d2 = ((dx*dx)+(dy*dy))+(dz*dz) in fp64, exact ties to the
 * smallest row index.  Asynchronous on the context's stream; results stay on the device. */
int pccm_nn(pccm_ctx *ctx, int dir, int engine);

/* PCCM_DIR_LEFT and PCCM_DIR_RIGHT together -- what CloudPair.__init__ does at cloud_pair.py:67-78.
 * Same results as two pccm_nn() calls; the grid engine fuses both directions into the same launches. */
int pccm_nn_pair(pccm_ctx *ctx, int engine);

/* Fuse the point-to-plane projection of direction `dir` (0 or 1) into the search: every settled query then also
 * leaves err . normal_other[row] (normal_mode PCCM_NORMAL_ROW: row i of the searched cloud's normals, what
 * metric.py:146-153 of the reference computes; PCCM_NORMAL_NEIGHBOUR: row nn(i)), so that the D2 reductions
 * (metric.py:179, 226-228, 366) need no second pass over the points.  normal_mode -1 switches it off.  A request
 * that cannot be honoured at search time (no normals set, row-indexed normals shorter than the iterating cloud)
 * is ignored; the reductions then take the separate pass and report the reference's IndexError (PCCM_E_RANGE).
 * Purely an optimisation: results are bit-identical either way.  Takes effect at the next pccm_nn / pccm_nn_pair. */
int pccm_nn_fuse(pccm_ctx *ctx, int dir, int normal_mode);

/* Whether the searches keep the matched row of every point (default: on).  Off, a search leaves 16 bytes per point
 * (squared distance + fused projection) instead of 32 -- half the scattered stores, and columns the reductions read
 * densely -- which is all that GeoMSE / GeoPSNR / Hausdorff need (metric.py:213-247, 353-386).  Whoever needs the rows
 * later (pccm_nn_fetch with idx, pccm_error_vectors, the colour calls: cloud_pair.py:34-42, 90-100, 120-124) gets them
 * anyway: the library repeats the search of that direction with the rows on.  Purely an optimisation. */
int pccm_nn_want_idx(pccm_ctx *ctx, int on);

/* Copy the shard's results to the host (either pointer may be NULL).  idx[i] is the row in
 * the searched cloud, d2[i] the squared distance: the (idxs, sqrdists) of cloud_pair.py:32-33
 * and the value behind get_left/right_neighbour_distances(), cloud_pair.py:102-106. */
int pccm_nn_fetch(pccm_ctx *ctx, int dir, int32_t *idx, double *d2);

/* get_left/right_error_vector(), cloud_pair.py:90-100: out[i][:] = iter[i] - search[nn(i)]. */
int pccm_error_vectors(pccm_ctx *ctx, int dir, double *out);

/* Diagnostic (opt-in, not on the report's path): how much of the point-to-plane result hangs on the ORDER OF EXACT TIES.
 * get_neighbour_cloud() keeps idx[-1] of a one-neighbour nanoflann search (cloud_pair.py:22-23) -- whichever of several
 * equidistant nearest points the tree meets; this library keeps the smallest row.  D1 is the same either way; the projection
 * err . normal (metric.py:146-153) is not.  For the shard's rows of direction `dir` (0 or 1; the search must have run):
 *   out[0] queries, out[1] queries with >= 2 equidistant nearest neighbours, out[2] / out[3] the sum over the queries of the
 *   SMALLEST / LARGEST squared projection over all their nearest neighbours, out[4] the same sum for the library's own picks,
 *   out[5] queries whose tie set was not enumerated (outliers far from the searched cloud: counted with their pick alone),
 *   out[6] the largest tie multiplicity seen.
 * out[2] / n_iter <= any admissible D2 MSE (the reference's included) <= out[3] / n_iter; tie-free data: out[1] = 0 and
 * out[2] = out[3] = out[4].  normal_mode -1: counts only (no normals needed).  Sums are plain fp64 accumulations. */
int pccm_tie_exposure(pccm_ctx *ctx, int dir, int normal_mode, double out[8]);

/* Which of several EXACTLY equidistant nearest points stands for the matched point of directions 0 and 1 (the self search is
 * not affected).  The reference keeps whichever one nanoflann's traversal meets (cloud_pair.py:22-23), so its point-to-plane
 * and colour rows depend on the order of the points in the files.
 *   PCCM_TIES_PICK (default; pccm_ctx_reset restores it): the point of the smallest row -- idx[] of pccm_nn_fetch.
 *   PCCM_TIES_MEAN: a virtual neighbour built from the tie set T_i = { j : d2(a_i, b_j) == d2_i }, rows ascending j_1 < ... < j_k:
 *     position c_i = (((b_j1 + b_j2) + b_j3) + ... ) / k per component in fp64 (sequential adds, one correctly rounded division
 *     by (double)k; k = 1 gives b_j1 exactly); colour: the same mean of the searched cloud's rgb doubles (bytes: k / 255.0),
 *     the scheme transform applies to the mean; normal under PCCM_NORMAL_NEIGHBOUR: the same mean of its normals, not
 *     renormalised (PCCM_NORMAL_ROW: row i, as always).  Error vectors, projections, D2 and every colour call read it; the
 *     squared distances, the D1 reductions and the matched rows of pccm_nn_fetch are those of PCCM_TIES_PICK (every tie
 *     shares d2_i).  Not order dependent: a permutation of the searched cloud leaves it as it is (up to the rounding of the
 *     sums).  Takes effect at the next pccm_nn / pccm_nn_pair.  Searches under MEAN cannot be captured (pccm_graph_begin:
 *     PCCM_E_STATE); run them eagerly. */
#define PCCM_TIES_PICK 0
#define PCCM_TIES_MEAN 1
int pccm_set_ties(pccm_ctx *ctx, int policy);
/* The size k of every tie set of the shard's rows of direction `dir` (0 or 1), as pccm_nn_fetch lays out its rows; the search
 * must have run under PCCM_TIES_MEAN (else PCCM_E_STATE). */
int pccm_tie_counts(pccm_ctx *ctx, int dir, int32_t *k);

/* Per-point metric vector of the shard (PCCM_METRIC_*), metric.py:124-179; PCCM_METRIC_ANGULAR and
 * PCCM_METRIC_SSIM_*, PCCM_METRIC_P2D*, PCCM_METRIC_RESOLUTION and PCCM_METRIC_REFLECTANCE ignore normal_mode. */
int pccm_point_metric(pccm_ctx *ctx, int dir, int metric, int normal_mode, double *out);

/* Fused reduction of a per-point metric over the shard: the np.sum / np.max of
 * GeoMSE.calculate (metric.py:226-228), GeoHausdorffDistance.calculate (metric.py:366) and
 * the np.min / np.max of BoundarySqrtDistances (metric.py:187-188; apply sqrt to both).
 *
 *   xvec    [pccm_xvec_len(n_iter)] doubles, zero except for this shard's entries:
 *           first 64 * (n_iter / 8192) sums of aligned 128-row leaves, accumulated exactly as
 *           NumPy's pairwise sum does, then the (n_iter % 8192) raw values of the last,
 *           partial 8192-row chunk.  Summing the xvecs of all ranks element-wise (RCCL
 *           all-reduce; x + 0 is exact) gives the full vector; pccm_finish_sum() then
 *           returns bit for bit what np.sum of the whole per-point array returns.
 *   minmax  [2]: min and max over the shard (+inf / -inf for an empty shard).
 *
 * pccm_reduce_prefetch() only enqueues the kernels and the copy of the small result arrays into
 * pinned host memory (no host wait); a later pccm_reduce() with the same arguments consumes it.
 * Prefetching every column a report needs right after pccm_nn() makes the host wait once per pair.
 */
int64_t pccm_xvec_len(int64_t n_iter);
int pccm_reduce_prefetch(pccm_ctx *ctx, int dir, int metric, int normal_mode);
/* n <= 8 columns at once: one kernel evaluates every point-to-plane column, one kernel reduces all of them. */
int pccm_reduce_prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes);
int pccm_reduce(pccm_ctx *ctx, int dir, int metric, int normal_mode, double *xvec, double *minmax);
int pccm_finish_sum(const double *xvec, int64_t n_iter, double *sum);
/* Unsharded shortcut (world = 1): out = {np.sum, np.min, np.max} of the whole column in one call. */
int pccm_reduce_total(pccm_ctx *ctx, int dir, int metric, int normal_mode, double out[3]);
/* The same for up to 8 columns in one call (out[k][3]): one wait for the GPU and one trip through the FFI per report instead
 * of one per column -- the np.sum / np.max of every GeoMSE / GeoHausdorffDistance row (metric.py:226-228, 366). */
int pccm_reduce_total_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, double *out);

/* Ranked (generalized) Hausdorff distance: the ks[i]-th smallest element (1-based; nearest rank, equal elements count
 * separately) of the column GeoHausdorffDistance.calculate takes the np.max of (metric.py:353-366) -- PCCM_METRIC_D1 or
 * PCCM_METRIC_D2 of direction 0 or 1, under the context's tie policy.  out[i] is an element of the column, bit for bit
 * np.partition(column, k - 1)[k - 1]; k = n_iter gives the np.max pccm_reduce_total reports.  The column is ranked in HBM by
 * the kernel that reduces it, from the values that reduction forms: a most-significant-bits-first radix select over the
 * order keys of the doubles (bit pattern with the sign flipped, negative values inverted -- the columns here hold no negative
 * value, no -0.0 and no NaN, the keys order any finite column), 11 bits per launch; no column and no per-row scratch is
 * allocated or copied.  n <= 8 selections per call, like a reduction batch.
 *   pccm_select_prefetch_many  enqueues the launches (and the columns' reductions where nobody has); capturable into a
 *                              hipGraph between pccm_graph_begin / pccm_graph_end like pccm_reduce_prefetch.
 *   pccm_select_many           consumes them (enqueuing first what nobody prefetched) and waits once.
 * PCCM_E_ARG: PCCM_DIR_SELF, any other metric, k < 1 or k > n_iter, a cloud of 2^32 rows or more (counts are 32 bits wide);
 * PCCM_E_STATE: no search result yet, a sharded context; PCCM_METRIC_D2 without the normals it needs: PCCM_E_STATE /
 * PCCM_E_RANGE exactly where pccm_reduce_total gives them. */
int pccm_select_prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const int64_t *ks);
int pccm_select_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const int64_t *ks,
                     double *out /*[n]*/);

/* The inverse query: out[i] is the number of rows of the column whose value is <= xs[i] -- np.count_nonzero(column <= xs[i]) --
 * for PCCM_METRIC_D1 or PCCM_METRIC_D2 of direction 0 or 1, under the context's tie policy.  With xs[i] = tau * tau on a D1
 * column this is the number of points within tau of the other cloud: the numerator of the precision / recall behind an
 * F-score, and at tau = 0 the number of points reproduced exactly.  The comparison is the IEEE one on the values the column's
 * reduction sums and pccm_select_many ranks (0.0 <= -0.0 holds; +inf counts every row, -inf none); the column is read once, in
 * HBM, in whatever form the search left it, by a further mode of the kernel that reduces it: no column is allocated or copied.
 * n <= 8 counts per call; more than four thresholds on one column take two passes over it.
 *   pccm_count_prefetch_many  enqueues the launches (and the columns' reductions where nobody has); capturable into a
 *                             hipGraph between pccm_graph_begin / pccm_graph_end like pccm_select_prefetch_many.
 *   pccm_count_many           consumes them (enqueuing first what nobody prefetched) and waits once.
 * PCCM_E_ARG: PCCM_DIR_SELF, any other metric, a NaN threshold, a cloud of 2^32 rows or more (counts are 32 bits wide on the
 * device); PCCM_E_STATE: no search result yet, a sharded context; PCCM_METRIC_D2 without the normals it needs: PCCM_E_STATE /
 * PCCM_E_RANGE exactly where pccm_reduce_total gives them. */
int pccm_count_prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const double *xs);
int pccm_count_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const double *xs,
                    int64_t *out /*[n]*/);

/* Mapped reductions: out[3 i ..] = np.sum, np.min, np.max of f(column), bit for bit, for PCCM_METRIC_D1 or PCCM_METRIC_D2 of
 * direction 0 or 1 under the context's tie policy, without the column or f(column) ever being stored.  maps[i] says what f is,
 * applied in this order:
 *   PCCM_MAP_CLAMP  min(value, xs[i])  (np.minimum(column, xs[i]); xs[i] is read with this bit alone)
 *   PCCM_MAP_ROOT   the correctly rounded square root (np.sqrt)
 * so PCCM_MAP_ROOT on a D1 column sums the unsquared nearest-neighbour distances (Chamfer-L1's numerator), PCCM_MAP_CLAMP at
 * tau * tau the squared distances truncated at tau, and both bits the truncated distances, sqrt(min(value, tau * tau)).  The map
 * is a mode of the general reduction kernel (k_unit_jobs): it reads the column once, in HBM, in whatever form the search left
 * it, and sums in NumPy's order like the plain reduction does.  n <= 8 per call.
 *   pccm_reduce_map_prefetch_many  enqueues the launch (and the columns' plain reductions where nobody has); capturable into
 *                                  a hipGraph between pccm_graph_begin / pccm_graph_end like pccm_count_prefetch_many.
 *   pccm_reduce_map_total_many     consumes them (enqueuing first what nobody prefetched) and waits once.
 * xs[i] = +inf clamps nothing (the plain total's bits); xs[i] <= 0 is allowed.
 * PCCM_E_ARG: PCCM_DIR_SELF, any other metric (PCCM_METRIC_PROJ has negative values), maps[i] outside 1..3 (0: use
 * pccm_reduce_total_many), a NaN xs[i] under PCCM_MAP_CLAMP; PCCM_E_STATE: no search result yet, a sharded context;
 * PCCM_METRIC_D2 without the normals it needs: PCCM_E_STATE / PCCM_E_RANGE exactly where pccm_reduce_total gives them. */
#define PCCM_MAP_CLAMP 1
#define PCCM_MAP_ROOT 2
int pccm_reduce_map_prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const int *maps,
                                  const double *xs);
int pccm_reduce_map_total_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const int *maps,
                               const double *xs, double *out /*[3 n]*/);

/* Match counts: out[j] = the number of shard rows of direction dir (0 or 1) whose matched row is j --
 * np.bincount(idx, minlength=n_searched) over the idx pccm_nn_fetch gives, as n_searched uint32 words (the searched cloud's
 * rows).  Counted on the GPU with integer atomics, once per search and direction and kept until the direction's results change;
 * the matched rows are read where the search left them (result records or the plain idx column), and a search that left them out
 * (pccm_nn_want_idx off, the voxel-brick search) is repeated with the rows on, as for pccm_carry_normals.
 * PCCM_E_ARG: dir is not 0 or 1, a null out.  PCCM_E_STATE: no search result yet, a sharded context, a search that ran under
 * PCCM_TIES_MEAN (a virtual neighbour has no row), a call during graph capture. */
int pccm_match_counts(pccm_ctx *ctx, int dir, uint32_t *out /*[n_searched]*/);

/* Density-aware Chamfer terms (Wu et al., NeurIPS 2021): out[3 i ..] = np.sum, np.min, np.max of
 *   t = 1 - exp(-alphas[i] * s) / m[idx]        s = sqrt(d2) (squared[i] == 0: the paper's equation) or d2 (squared[i] == 1)
 * over the PCCM_METRIC_D1 column d2 of direction dirs[i] (0 or 1), idx its matched rows and m the direction's match counts
 * (pccm_match_counts).  On the device: s = squared ? d2 : sqrt_rn(d2); a = mul_rn(-alpha, s); e = exp(a) (the fp64 device exp);
 * q = div_rn(e, (double)m); t = sub_rn(1.0, q) -- every operation but exp correctly rounded --, summed in NumPy's order.  So
 * alpha = 0 gives np.sum(1.0 - 1.0 / m[idx]) bit for bit (the left row / n = 1 - distinct matched rows / n: a coverage number),
 * a huge alpha (1e300) np.sum(np.where(s > 0, 1.0, 1.0 - 1.0 / m[idx])) bit for bit, and any other alpha differs from NumPy by
 * what the two exp implementations differ by.  Every m that is gathered is >= 1 (the row that gathers it counted itself), so
 * every term lies in [0, 1].  The term is the map PCCM_MAP_DENSITY of the general reduction kernel (k_unit_jobs), applied behind
 * the optional root and never combined with a clamp: it reads the column once, in HBM, gathers the counts through the matched
 * rows, and stores no column; pccm_reduce_map_* keeps refusing maps outside 1..3.  n <= 8 per call (n == 0: PCCM_OK).
 *   pccm_reduce_density_prefetch_many  makes the counts where the search's are not there yet (a memset and one launch) and
 *                                      enqueues the mapped launch behind them; capturable between pccm_graph_begin /
 *                                      pccm_graph_end like pccm_reduce_map_prefetch_many (a search without matched rows cannot
 *                                      be repeated there: PCCM_E_STATE).
 *   pccm_reduce_density_total_many     consumes them (enqueuing first what nobody prefetched) and waits once.
 * PCCM_E_ARG: n outside 0..8, a null array with n > 0 or a null out, PCCM_DIR_SELF, squared[i] outside 0 / 1, alphas[i] NaN,
 * negative or infinite.  PCCM_E_STATE: no search result yet, a sharded context, a search that ran under PCCM_TIES_MEAN. */
#define PCCM_MAP_DENSITY 4
int pccm_reduce_density_prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *squared, const double *alphas);
int pccm_reduce_density_total_many(pccm_ctx *ctx, int n, const int *dirs, const int *squared, const double *alphas,
                                   double *out /*[3 n]: np.sum, np.min, np.max of the terms*/);

/* Alignment moments: the sums a Kabsch step of point-to-point ICP is made from.  For shard row i of direction dirs[r] (0 or 1),
 * j its matched row (PCCM_TIES_PICK), d2 the PCCM_METRIC_D1 value the plain reduction forms and w = (d2 <= caps[r]) -- the IEEE
 * comparison, so a cap of +inf keeps every row --, with u_a = sub_rn(x_it[i][a], pivot[a]) and v_b = sub_rn(x_se[j][b], pivot[b])
 * from the two clouds' stored fp64 coordinates, the term of kinds[r] is
 *   0..2       w ? u_a : 0.0                    (a = kind)
 *   3..5       w ? v_b : 0.0                    (b = kind - 3)
 *   6 + 3a + b w ? mul_rn(u_a, v_b) : 0.0
 *   15         w ? d2 : 0.0
 * and out[3 r ..] = np.sum, np.min, np.max of that term column -- np.sum(np.where(w, term, 0.0)) bit for bit: the terms are
 * summed in NumPy's pairwise order by the leaf reduction like every other column (the extrema order -0.0 below 0.0, which NumPy's
 * do not: a product column holds both as soon as a point has a coordinate of the pivot).  The term is the map PCCM_MAP_MOMENT of the
 * general reduction kernel (k_unit_jobs): it reads the D1 column once, gathers the matched point through the matched row (read
 * where the search left it; a search that left the rows out is repeated, as for the density map) and stores no column.  The
 * requests of one call share the pivot; pending requests made with another pivot are given up.  n <= 8 per call (n == 0:
 * PCCM_OK); prefetch and total behave like pccm_reduce_density_*_many, capture included.
 * PCCM_E_ARG: n outside 0..8, a null array with n > 0 or a null out, PCCM_DIR_SELF, a kind outside 0..15, a NaN cap, a null or
 * non-finite pivot.  PCCM_E_STATE: no search result yet, a sharded context, a search that ran under PCCM_TIES_MEAN, a search
 * that has to be repeated during graph capture. */
#define PCCM_MAP_MOMENT 8
int pccm_reduce_moment_prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *kinds, const double *caps, const double pivot[3]);
int pccm_reduce_moment_total_many(pccm_ctx *ctx, int n, const int *dirs, const int *kinds, const double *caps, const double pivot[3],
                                  double *out /*[3 n]: np.sum, np.min, np.max of the terms*/);

/* Move a resident cloud: every row of cloud `which` (0 or 1) becomes A x + t for the row-major 3 x 4 matrix m = [A | t], in fp64 on
 * the stored coordinates and with one rounding per operation:
 *   x' = ((a00 x + a01 y) + a02 z) + t0, likewise y' and z'.
 * A cloud with one normal per point has them mapped by A alone, n' = (a00 nx + a01 ny) + a02 nz per component (announced normals
 * -- pccm_set_normals_deferred -- are uploaded first).  That is right for a rotation; the call does NOT test that A is orthogonal.
 * The context is left as pccm_set_cloud(which, X', n, PCCM_F64, ...) followed by pccm_set_normals(N') would leave it -- the ingest
 * statistics (fp32-exactness, integer coordinates, largest magnitude, bounding box), the fp32 copies and their padding are made
 * again by the ingest kernels, which do the arithmetic as a mode --, except that colours, packed colours, reflectance and the
 * merge map STAY.  Search results of every direction that touches the cloud are dropped (moving cloud 1 keeps the self search of
 * cloud 0), with PointSSIM features, spacings, point-to-distribution columns, the spatial order and carried normals of either cloud.
 * An m that is exactly the identity (==) is a no-op: nothing is rewritten and nothing goes stale.
 * PCCM_E_ARG: which is not 0 or 1, m is null or has a non-finite entry, or a coordinate could exceed 1e15 -- judged on the host
 * from the cloud's largest magnitude and the rows' absolute sums, before anything is written.  PCCM_E_STATE: no such cloud, a
 * normal count that is neither 0 nor n, a sharded context, a call between pccm_graph_begin and pccm_graph_end. */
int pccm_transform_cloud(pccm_ctx *ctx, int which, const double m[12]);

/* The bounding box of cloud `which` (0 or 1) as the ingest found it: lo[a] / hi[a] = the smallest / largest fp64 coordinate of
 * axis a (-0.0 orders below 0.0).  No device work.  PCCM_E_ARG: which is not 0 or 1, a null pointer.  PCCM_E_STATE: no such cloud. */
int pccm_get_bounds(pccm_ctx *ctx, int which, double lo[3], double hi[3]);

/* Sharded contexts whose rows start and end on whole 8192-row chunks (pccm_set_shard / pccm_set_shard_dir do that
 * whenever every rank can have a chunk): the exchange vector shrinks to ONE number per chunk -- NumPy adds the
 * chunks of a column one after the other, and the GPU has finished each chunk's pairwise tree -- plus the raw values
 * of the last, partial chunk.  cvecs: the columns' vectors one after the other, pccm_cvec_len(n_iter) doubles each,
 * zero except for this shard's entries (SUM them over the ranks); minmax[2k], [2k+1]: this shard's extrema of column k.
 * pccm_finish_chunks() gives np.sum of the whole column from a summed vector.  PCCM_E_STATE when the shard is not
 * chunk-aligned (then use pccm_reduce / pccm_finish_sum).  Stands under metric.py:226-228, 366 like pccm_reduce. */
int64_t pccm_cvec_len(int64_t n_iter);
int pccm_reduce_chunks_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, double *cvecs,
                            double *minmax);
int pccm_finish_chunks(const double *cvec, int64_t n_iter, double *sum);

/* How the calls that hand reduced numbers to the caller (pccm_reduce, pccm_reduce_total[_many], pccm_reduce_chunks_many: the
 * np.sum / np.max of metric.py:226-228, 366, where the reference has its numbers at once) wait for the GPU.
 *   PCCM_WAIT_SPIN (default): one wave behind a batch's last reduction kernel bumps the context's completion counter, a word
 *     in host memory, once the batch's numbers are there, and the calling thread spins on it.  The host sees the numbers
 *     about 13 us sooner than through the runtime's event completion.  After 2 ms of spinning it waits on the batch's
 *     event instead, so a fault or a hang still comes back as a HIP error.
 *   PCCM_WAIT_EVENT: hipEventSynchronize on the batch's event (the thread sleeps: for oversubscribed hosts).
 * Either way, the device error word is checked behind the wait.  Per context; pccm_ctx_reset keeps it. */
#define PCCM_WAIT_SPIN 0
#define PCCM_WAIT_EVENT 1
int pccm_set_wait(pccm_ctx *ctx, int mode);
/* The context's completion counter: the number of reduction batches whose numbers have reached the host so far. */
int pccm_wait_counter(pccm_ctx *ctx, uint64_t *out);

/* Colours of cloud `which` ([n][3] RGB in [0, 1] as Open3D holds them; n = the cloud's point count):
 * replaces np.asarray(cloud.colors) behind get_left/right_colors(), cloud_pair.py:114-118. */
int pccm_set_colors(pccm_ctx *ctx, int which, const void *rgb, int64_t n, int dtype, int on_device);

/* The same from the uchar colours point-cloud files hold: rgb[n][3] bytes, widened on the device as k / 255.0 -- the
 * division o3d.io.read_point_cloud (and io.py) perform on the host, bit for bit. */
int pccm_set_colors_u8(pccm_ctx *ctx, int which, const unsigned char *rgb, int64_t n);

/* Reflectance of cloud `which`: one scalar per point (the laser return intensity of LiDAR content), n = the cloud's point count,
 * dtype PCCM_F32 or PCCM_F64.  Held as fp64 on the device with the values as given: nothing is normalised or divided.  Values
 * must be finite.  A new reflectance leaves searches, normals, colours, PointSSIM features, spacings and point-to-distribution
 * columns as they are; pending reductions and captured graphs go stale (they may read the column).  New points on the cloud
 * (pccm_set_cloud, pccm_ctx_reset) take its reflectance away; pccm_merge_duplicates carries it: PCCM_DUP_DROP keeps the
 * representative's value bit for bit, PCCM_DUP_AVERAGE gives s / (double)m with s = r[i_1], then s = s + r[i_k] in ascending row
 * order, every add rounded (the colour rule; m = 1 gives the value back bit for bit).
 * PCCM_E_STATE: the cloud is not set.  PCCM_E_ARG: n is not the cloud's point count; a non-finite value (the cloud then has no
 * reflectance). */
int pccm_set_reflectance(pccm_ctx *ctx, int which, const void *r, int64_t n, int dtype, int on_device);
/* The same from the 16-bit values LiDAR files hold (host memory; 40000 becomes 40000.0).  The library widens them to float on
 * the host -- exact: every 16-bit value is a float -- and they cross PCIe as four bytes per point through the float ingest; a
 * device-side widening of the two-byte values would need a kernel of its own, which this library does not have yet. */
int pccm_set_reflectance_u16(pccm_ctx *ctx, int which, const uint16_t *r, int64_t n);
/* the stored column: n doubles (PCCM_E_STATE when the cloud has no reflectance) */
int pccm_get_reflectance(pccm_ctx *ctx, int which, double *out);

/* Colour metrics of one direction on the device, metric.py:302-333 and :389-427.  Per row i of the
 * iterating cloud: own = T(rgb_own[i]), other = T(rgb_other[nn(i)]) (the gather of
 * get_left/right_neighbour_colors(), cloud_pair.py:120-124; T = transform_colors(), metric.py:261-290,
 * scheme 0 "rgb" | 1 "ycc" | 2 "yuv"), sq = (scale * (own - other))^2.
 *   sum_out[c] = np.add.reduce(sq, axis=0)[c]  -- bit for bit: the left-to-right row order NumPy uses for
 *                axis 0 (ColorMSE = sum / n, i.e. np.mean(diff**2, axis=0));
 *   max_out[c] = np.max(sq, axis=0)[c]          (ColorHausdorffDistance; scale = 255 for "rgb", metric.py:422-425).
 * `rows`: NULL = the neighbour rows of the context's own search of `dir` (which must cover the whole cloud);
 * otherwise `nrows` = n_iter host rows (sharded searches: the ranks' slices gathered by the caller). */
int pccm_color_reduce(pccm_ctx *ctx, int dir, int scheme, double scale, const int32_t *rows, int64_t nrows,
                      double sum_out[3], double max_out[3]);

/* The same rows materialised to the host, out[n_iter][3]: what = 0 own colours in the scheme,
 * 1 neighbour colours in the scheme, 2 scale * (own - other), 3 its square. */
int pccm_color_rows(pccm_ctx *ctx, int dir, int scheme, double scale, int what, const int32_t *rows, int64_t nrows,
                    double *out);

/* The frame search behind CloudPair.get_extent() (cloud_pair.py:111-112, Open3D's minimal oriented bounding box):
 * verts = the nv vertices of the convex hull of cloud A, tri = its nt triangles as vertex coordinates [nt][3][3]
 * (the hull itself is Qhull on the host, as in Open3D).  For every triangle the axis-aligned extents of the hull
 * vertices in the triangle's frame (x along its first edge, z along its normal) are evaluated on the device;
 * ext_out = the extents of the frame with the smallest volume (first one on ties), *vol_out its volume. */
int pccm_obb_frames(pccm_ctx *ctx, const double *verts, int64_t nv, const double *tri, int64_t nt, double ext_out[3], double *vol_out);

/* Thinning cloud `which` before the host's Qhull run (get_minimal_oriented_bounding_box, cloud_pair.py:111-112):
 * pccm_extreme_rows  rows_out[k] = row of (about) the farthest point of the cloud along dirs[k] (ndirs <= 1024, fp32);
 * pccm_rows_outside  the rows (unordered) of all points x with n.x + off > -margin for some plane (n, off) of
 *                    planes[nplanes][4] -- Qhull's convention: n.x + off <= 0 inside.  With the facets of the hull of
 *                    the extreme points as planes, every point NOT reported lies strictly inside the hull of other
 *                    points of the cloud and cannot be a vertex of the cloud's hull.  rows_out must hold n rows. */
int pccm_extreme_rows(pccm_ctx *ctx, int which, const float *dirs, int ndirs, int32_t *rows_out);
int pccm_rows_outside(pccm_ctx *ctx, int which, const double *planes, int nplanes, double margin, int32_t *rows_out, int64_t *count);

/* Utility behind pccm_color_reduce: out[c] = left-to-right fp64 sum of column c of three non-negative
 * host columns cols[3][n] -- what np.add.reduce(a, axis=0) returns for the (n, 3) array a = cols.T --
 * evaluated on the device without the dependent chain (csrc/pccm_color.hip). */
int pccm_seq_colsum(pccm_ctx *ctx, const double *cols, int64_t n, double out[3]);

/* Host-only helper (no GPU) of the PCD reader that stands in for o3d.io.read_point_cloud (handler.py:57):
 * liblzf decompression of a binary_compressed body.  *out_len = bytes written (<= out_cap). */
int pccm_lzf_decompress(const unsigned char *in, int64_t in_len, unsigned char *out, int64_t out_cap, int64_t *out_len);

/* Host-only helper (no GPU): rows of RGB in [n][3] -> the target scheme of transform_colors(),
 * metric.py:261-290 (scheme 1 = "ycc", 2 = "yuv"), bit-compatible with the reference's per-row np.matmul. */
int pccm_color_transform(const double *rgb, int64_t n, int scheme, double *out);

/* Forget the search structures derived from the clouds (the grid engine's cell-sorted copies,
 * the analogue of the KD-trees CloudPair.__init__ builds at cloud_pair.py:65), so that the next
 * pccm_nn() rebuilds them.  bench.py calls it every step: a step pays for its builds. */
int pccm_drop_caches(pccm_ctx *ctx);

/* hipGraph capture.  Between pccm_graph_begin() and pccm_graph_end() only pccm_drop_caches(),
 * pccm_nn(), pccm_reduce_prefetch[_many](), pccm_select_prefetch_many(), pccm_count_prefetch_many(), pccm_reduce_map_prefetch_many(), pccm_reduce_density_prefetch_many() and pccm_reduce_moment_prefetch_many() may be called; they are recorded on the
 * context's stream instead of executed.  The same sequence must have run once before (capture cannot allocate).
 * pccm_graph_end() instantiates the graph, runs it once and returns its id; pccm_graph_launch()
 * replays the whole sequence -- kernels and host-side bookkeeping -- with a single launch, after which
 * pccm_reduce()/pccm_select_many()/pccm_count_many()/pccm_reduce_map_total_many()/pccm_reduce_density_total_many()/pccm_reduce_moment_total_many()/pccm_match_counts()/pccm_nn_fetch() read the fresh results.  A graph goes stale (PCCM_E_STATE) when
 * clouds, normals, shard or any buffer it references change.  One report over resident clouds is
 * ~45 small launches, which an eager host cannot issue as fast as the GPU retires them. */
int pccm_graph_begin(pccm_ctx *ctx);
int pccm_graph_end(pccm_ctx *ctx, int *graph_id);
int pccm_graph_launch(pccm_ctx *ctx, int graph_id);
int pccm_graph_destroy(pccm_ctx *ctx, int graph_id);

/* Filed tails.  A capture may leave the tail launch of pccm_nn_pair() out: the brick search files the queries ring 1 did not settle
 * under their block of 4096 rows, and the reduction workgroup that owns those rows settles them (rings 2-3, the tail launch's own
 * search) before it reduces.  It does so only when the eager step in front of the capture, on the same resident clouds, handed no
 * query to the exact rescan, filled no block beyond the lists' capacity and reduced D1 + row-indexed D2 of every searched
 * direction in one batch behind the search (and searched every direction the capture searches); otherwise, and whenever anything but such a reduction reads the results first, the
 * graph holds the tail launch as ever.  Results are bit-identical either way.  pccm_set_tail_filing(ctx, 0), between
 * pccm_graph_begin() and the captured search, keeps the tail launch in that capture (on: the default of every capture);
 * PCCM_TAIL_FILED=0 in the environment keeps it always (A/B runs).
 * pccm_graph_tail_filed(): *filed = 1 when graph `graph_id` was captured without the tail launch. */
int pccm_set_tail_filing(pccm_ctx *ctx, int on);
int pccm_graph_tail_filed(pccm_ctx *ctx, int graph_id, int *filed);

/* Wait for everything queued on the context's stream. */
int pccm_sync(pccm_ctx *ctx);

/* HIP-event timing of kernel classes on the context's stream (for bench.py's roofline). */
int pccm_profile_enable(pccm_ctx *ctx, int on);
int pccm_profile_reset(pccm_ctx *ctx);
int pccm_profile_get(pccm_ctx *ctx, int kernel_class, double *ms_total, int64_t *launches);

/* Bookkeeping of the last pccm_nn() in `dir`: out[0] = queries sent to the exact fallback
 * rescan, out[1] = ref-axis splits of the brute-force scan / number of cells of the grid the
 * grid engine searched, out[2] = (query, ref) pairs evaluated by the brute-force scan (grid: 0).
 * `dir | PCCM_STATS_TAIL`: out[0] = queries the grid engine's ring-1 kernel left to the tail launch, out[1] = out[2] = 0.
 * `dir | PCCM_STATS_TIES`: see below. */
#define PCCM_STATS_TAIL 0x10
/* `dir | PCCM_STATS_TIES` (search under PCCM_TIES_MEAN): out[0] = queries whose tie set the cell walk could not settle (a ball over
 * more than 4096 cells, more than 16 ties, no tie met) and the exact scan of the whole searched cloud enumerated; out[1] = out[2] = 0. */
#define PCCM_STATS_TIES 0x20
int pccm_nn_stats(pccm_ctx *ctx, int dir, int64_t out[3]);

/* Which kernel variants served a call: the library picks them from the data (density, size ratio, fp32-exactness, integer
 * coordinates, the normals' precision, the shard) and from a few environment switches, never from the caller.  `which`:
 *   PCCM_DIR_LEFT / _RIGHT / _SELF  the last search of that direction (pccm_nn, pccm_nn_pair, or the repeat of a search that
 *                                   left its rows out), with the tie means and tie exposure made from it later;
 *   PCCM_PATH_REDUCE                the last batch of reductions (pccm_reduce_prefetch[_many] or a call that enqueued one).
 * buf receives the kernels that call enqueued, in launch order without repeats, separated by ';', each named as `nm -C` names
 * its host stub after "__device_stub__" -- "k_brick_query<false, 4, 2, 2176, false, 0, true>", "k_grid_tail<pccm::Rec32, false>",
 * "k_unit_lean<2, 1, 3>" -- NUL-terminated and cut to cap - 1 bytes; *len (may be NULL) = the full length.  Noted when the
 * kernels are enqueued (host bookkeeping only: no GPU work, no wait), so a captured call is described by its capture; graph
 * replays do not change it.  A launch the device decides to leave idle (a tail with no queries) is still listed.  A log holds
 * 64 distinct kernels; a call that enqueued more ends its list with the entry "..." (the path is incomplete). */
#define PCCM_PATH_REDUCE 3
int pccm_nn_path(pccm_ctx *ctx, int which, char *buf, int64_t cap, int64_t *len);

/* The uniform grid the last grid-engine search ran on: cell (i, j, k) spans org + (i, j, k) * h .. org + (i + 1, j + 1, k + 1) * h
 * per axis, dim cells per axis (voxel-brick searches: cells of 8 voxels).  Lets a caller place points exactly on cell faces.
 * PCCM_E_STATE before the first grid search. */
int pccm_grid_geometry(pccm_ctx *ctx, double org[3], double h[3], int32_t dim[3]);

/* What a grid build left behind, read back for inspection (diagnostics and tests; never part of a report).  Every build is one
 * counting sort of some rows by cell; the library notes on the host, where it starts the sort, what each of these structures
 * was last built as -- no GPU work, no wait:
 *   PCCM_BUILD_GRID0 / _GRID1                cloud 0 / 1 of the grid the last search built (the pair's grid, or the grid over one
 *                                            cloud alone that a k-nearest-neighbour search -- normal estimation -- builds for itself);
 *   PCCM_BUILD_SHARD_LEFT / _RIGHT / _SELF   the cell-sorted query rows of that direction's shard in the last search (whether they
 *                                            were sorted by the grid build's own launches or by a sort of their own);
 *   PCCM_BUILD_SP0 / _SP1                    cloud 0 / 1 in its spatial order (made by the first pccm_drop_caches behind a search).
 * pccm_build_plan fills plan[PCCM_BP_COUNT] (indices below) and geom = {org[3], h[3]}; pccm_build_fetch copies the structure to
 * the host: cell_start[ncells + 1] (relative to the structure's first record), rows[n] and xyz[n][3] (the records in stored
 * order: original row, and the stored coordinates widened to fp64 -- exact), occ[(ncells + 31) / 32] (the occupancy bitmap, when
 * PCCM_BP_HAS_OCC); a null pointer skips that part.  The shard structures and the spatial order's cell starts live in scratch
 * that any later build or occupancy measurement overwrites: PCCM_E_STATE for a structure that is no longer (or was never) there
 * -- a grid never built or dropped by pccm_drop_caches, a direction that was not sharded, a cloud without a spatial order -- and,
 * in pccm_build_fetch, for cell starts asked of a structure whose PCCM_BP_HAS_CS is 0.  Not allowed during graph capture; a
 * captured search is described by its capture, and every replay leaves the same structures. */
#define PCCM_BUILD_GRID0 0
#define PCCM_BUILD_GRID1 1
#define PCCM_BUILD_SHARD_LEFT 2
#define PCCM_BUILD_SHARD_RIGHT 3
#define PCCM_BUILD_SHARD_SELF 4
#define PCCM_BUILD_SP0 5
#define PCCM_BUILD_SP1 6
#define PCCM_BUILD_COUNT 7
#define PCCM_BP_REC32 0      /* records are 16 bytes {x, y, z as fp32, row}; 0: 32 bytes {x, y, z as fp64, row} */
#define PCCM_BP_NCELLS 1
#define PCCM_BP_N 2          /* records of the structure */
#define PCCM_BP_ROW0 3       /* ... which are rows [row0, row0 + n) of their cloud */
#define PCCM_BP_HAS_OCC 4    /* an occupancy bitmap was written beside the cell starts */
#define PCCM_BP_MORTON 5     /* cells are numbered along a Z-order curve (the spatial order), not x-fastest */
#define PCCM_BP_BITS 6       /* ... over 2^bits cells per axis */
#define PCCM_BP_DIM 7        /* [7..9]: cells per axis */
#define PCCM_BP_LG 10        /* the sort's plan: a bin is 2^lg consecutive cells, */
#define PCCM_BP_NBIN 11      /* bins per job, */
#define PCCM_BP_TILES 12     /* tiles of this structure's job */
#define PCCM_BP_TILE_ROWS 13 /* ... and rows per tile, */
#define PCCM_BP_SCAN 14      /* 1: hist matrix + look-back scan (PCCM_BUILD_SCAN=1), 0: bin cursors, */
#define PCCM_BP_SCAN_TILES 15 /* workgroups of the look-back scan (0 without it), */
#define PCCM_BP_READ_SP 16   /* the job read its cloud in spatial order instead of row order, */
#define PCCM_BP_NJOBS 17     /* jobs the sort's launches served, */
#define PCCM_BP_JOB 18       /* which of them made this structure, */
#define PCCM_BP_JOB_ROW0 19  /* [19..20]: first row of job 0 / 1, */
#define PCCM_BP_JOB_N 21     /* [21..22]: rows of job 0 / 1 */
#define PCCM_BP_HAS_CS 23    /* the structure's cell starts are still there to fetch */
#define PCCM_BP_COUNT 24
int pccm_build_plan(pccm_ctx *ctx, int which, int64_t plan[PCCM_BP_COUNT], double geom[6]);
int pccm_build_fetch(pccm_ctx *ctx, int which, uint32_t *cell_start, int32_t *rows, double *xyz, uint32_t *occ);

#ifdef __cplusplus
}
#endif
#endif /* PCCM_H */
