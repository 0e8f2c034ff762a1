// Exact k-NN searches on the grid engine's cell-sorted records, shared by normal estimation (pccm_normals.hip), the PointSSIM
// features (pccm_ssim.hip) and the point-to-distribution columns (pccm_p2d.hip).
//   - neighbours: exact k-NN, squared distance in fp64 ((dx*dx)+(dy*dy))+(dz*dz), ties to the smaller row.
// Three kernels make one chain.  A wave per point first (k_knn_cov_wave, below); the points it cannot settle go to one thread per
// point (k_knn_normals), which scans the cube [c-r, c+r]^3 ring by ring, keeping the k best (d2, row) in a sorted private list,
// until the k-th best is provably closer than anything outside the cube (knn_stop_bound, the 1-NN search's stop rule).  Points
// that are still open after kKnnMaxRing rings (isolated outliers) are finished by an exact block-per-point scan of the whole cloud
// (k_knn_normals_full).
//
// The sink (KnnSink) is either the normals -- the wave kernel leaves covariances, which k_normals_from_cov turns into normals, the
// other two write their normals themselves -- or neighbour lists (nbr_out, [n][k] int32): each kernel then writes the point's
// neighbours in ascending (d2, row) order and their count instead.
//
// The searches also run ACROSS the clouds (point-to-distribution): the queries are the points of one cloud (query_at), the
// candidates the cells of the other.  A query's cell comes from its coordinates through ncell_coord, which clamps, so a query may
// lie outside the searched cloud's grid.  The stop rule stays a valid lower bound: L only counts a face of the cube [c-r, c+r]^3
// that is not a face of the grid, and on every axis the query lies between the two faces of its cube or beyond the one that is the
// grid's (where no point of the searched cloud can be: the grid's boundary cells hold everything that clamps into them).  A point
// outside the cube is beyond a counted face, at least (face - q) - slack away along that axis, exactly as for a query inside the
// grid.
#include "pccm_knn.h"
#include "pccm_normals.h"

namespace pccm {

__device__ void normal_from_neighbours(const double *__restrict__ x64, double qx, double qy, double qz, const int *bi, int cnt,
                                       double *__restrict__ out)
{
    double n[3] = {0.0, 0.0, 1.0};
    if (cnt >= 3) {
        double a[6];
        neighbour_covariance(x64, qx, qy, qz, bi, cnt, a);
        smallest_eigenvector(a[0], a[1], a[2], a[3], a[4], a[5], n);
    }
    out[0] = n[0]; out[1] = n[1]; out[2] = n[2];
}

// the list sink: the neighbour rows (ascending (d2, row)) and their count
__device__ __forceinline__ void ssim_neighbours_out(const int *bi, int cnt, int k, int qrow, int32_t *__restrict__ nbr_out,
                                                    int32_t *__restrict__ cnt_out)
{
    for (int j = 0; j < cnt; ++j) nbr_out[(int64_t)qrow * k + j] = bi[j];
    cnt_out[qrow] = cnt;
}

// one thread per point (in cell-sorted order); rings 0..kKnnMaxRing
// `todo` / `todo_count`: positions (within this cloud's slice) the wave kernel handed on; the threads stride over them
// `qrecs` / `qx64`: where the queries are read (query_at); `recs`, `cell_start`, `x64`: the searched cloud
__global__ __launch_bounds__(256) void k_knn_normals(const GridRec *__restrict__ recs, const GridRec *__restrict__ qrecs,
                                                     const double *__restrict__ qx64, KnnGeom g,
                                                     const uint32_t *__restrict__ cell_start, const double *__restrict__ x64,
                                                     int k, double *__restrict__ nrm_out, const uint32_t *__restrict__ todo,
                                                     const uint32_t *__restrict__ todo_count, int32_t *__restrict__ open_list,
                                                     uint32_t *__restrict__ open_count, int32_t *__restrict__ nbr_out,
                                                     int32_t *__restrict__ cnt_out)
{
  const int64_t n = *todo_count;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < n; u += (int64_t)gridDim.x * 256) {
    const int64_t t = todo[u];
    double qx, qy, qz;
    int qrow;
    query_at(qrecs, qx64, t, qx, qy, qz, qrow);
    const int dimx = g.dim[0], dimy = g.dim[1], dimz = g.dim[2];
    const int cx = ncell_coord(qx, g.org[0], g.inv_h[0], dimx);
    const int cy = ncell_coord(qy, g.org[1], g.inv_h[1], dimy);
    const int cz = ncell_coord(qz, g.org[2], g.inv_h[2], dimz);
    double bd[kKnnMax];
    int bi[kKnnMax];
    int cnt = 0;
    bool done = false;
    for (int r = 0; r <= kKnnMaxRing && !done; ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, dimz - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, dimy - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, dimx - 1);
        for (int z = z0; z <= z1; ++z) {
            const bool zface = (z == cz - r) || (z == cz + r);
            for (int y = y0; y <= y1; ++y) {
                const uint32_t row = ((uint32_t)z * dimy + y) * dimx;
                const bool full = zface || y == cy - r || y == cy + r;
                for (int part = 0; part < (full ? 1 : 2); ++part) {
                    int xa, xb;
                    if (full) { xa = x0; xb = x1; }
                    else if (part == 0) { xa = xb = cx - r; if (xa < 0) continue; }
                    else { xa = xb = cx + r; if (xb > dimx - 1) continue; }
                    const uint32_t s = cell_start[row + xa], e = cell_start[row + xb + 1];
                    for (uint32_t p = s; p < e; ++p) {
                        const double4 a = *reinterpret_cast<const double4 *>(&recs[p]);
                        knn_insert(bd, bi, k, cnt, nd2(qx, qy, qz, a.x, a.y, a.z), (int)(__double_as_longlong(a.w) & 0xffffffffll));
                    }
                }
            }
        }
        // stop rule of the grid engine, applied to the k-th best
        const double L = knn_stop_bound(g, qx, qy, qz, cx, cy, cz, r);
        if (L == INFINITY) done = true;
        else if (cnt == k && L > 0.0 && bd[k - 1] < L * L * (1.0 - 0x1.0p-30)) done = true;
    }
    if (done && nbr_out) {
        ssim_neighbours_out(bi, cnt, k, qrow, nbr_out, cnt_out);
    } else if (done) {
        normal_from_neighbours(x64, qx, qy, qz, bi, cnt, nrm_out + 3 * (int64_t)qrow);
    } else {
        open_list[atomicAdd(open_count, 1u)] = qrow;
    }
  }
}

// ---- one wave per point -------------------------------------------------------------------------------
// The per-thread search above keeps its k best in a private sorted list: ~85 insertions of ~15 shifts each per
// point, all through scratch memory (12 ms per million points).  Here a wave takes one point: the lanes own the
// x-runs of the cube [c-r, c+r]^3 (r = 2, then 3), the candidates' distances go to LDS, the k-th smallest is
// found by a wave-wide quickselect (pivot = some staged distance inside the bracket, counted with ballots), ties at
// the k-th distance go to the smaller rows, and the covariance of the selected points is accumulated by all lanes
// and written out; k_normals_from_cov then solves the 3x3 eigenproblems one thread per point.  Same neighbour set
// as the per-thread search (exact k-NN, (d2, row) order); the sums are taken in a different order (a butterfly over the lanes
// instead of left to right), but one the neighbour set alone decides: the selected candidates are compacted to the front of the
// wave's LDS (ballot + prefix count), lane l < kk finds the rank of entry l among them in ascending (d2, row) order, and the
// neighbour of rank r is summed by lane r.  The order of the records inside a cell, which the grid build leaves to its atomics,
// does not reach the covariance: an estimate repeated on a rebuilt grid gives the same bits.
// Points the two cubes cannot settle, or with more than kWCap candidates, are passed on to k_knn_normals.
// With nbr_out (PointSSIM) lane l also writes the row of entry l at its rank: the kk selected rows in ascending (d2, row) order.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(256) void k_knn_cov_wave(const GridRec *__restrict__ recs, const GridRec *__restrict__ qrecs,
                                                      const double *__restrict__ qx64, int64_t n, KnnGeom g,
                                                      const uint32_t *__restrict__ cell_start, int k,
                                                      double *__restrict__ cov_out /*[n][6] by row*/, int32_t *__restrict__ cnt_out,
                                                      uint32_t *__restrict__ todo, uint32_t *__restrict__ todo_count,
                                                      int32_t *__restrict__ nbr_out /*[n][k] by row, or null*/)
{
    __shared__ double s_d[4][kWCap];
    __shared__ uint32_t s_p[4][kWCap];
    __shared__ uint32_t s_r[4][kKnnMax];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int dimx = g.dim[0], dimy = g.dim[1], dimz = g.dim[2];
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t t = (int64_t)blockIdx.x * 4 + w; t < n; t += nwaves) {
        double qx, qy, qz;                                                                  // wave-uniform
        int qrow;
        query_at(qrecs, qx64, t, qx, qy, qz, qrow);
        const int cx = ncell_coord(qx, g.org[0], g.inv_h[0], dimx);
        const int cy = ncell_coord(qy, g.org[1], g.inv_h[1], dimy);
        const int cz = ncell_coord(qz, g.org[2], g.inv_h[2], dimz);
        bool done = false, giveup = false;
        for (int r = 2; r <= 3 && !done && !giveup; ++r) {
            // the lanes own the (2r+1)^2 x-runs of the cube
            const int side = 2 * r + 1;
            uint32_t s = 0, len = 0;
            if (lane < side * side) {
                const int z = cz + lane / side - r, y = cy + lane % side - r;
                if (z >= 0 && z < dimz && y >= 0 && y < dimy) {
                    const uint32_t row = ((uint32_t)z * dimy + y) * dimx;
                    const int x0 = max(cx - r, 0), x1 = min(cx + r, dimx - 1);
                    s = cell_start[row + x0];
                    len = cell_start[row + x1 + 1] - s;
                }
            }
            const uint32_t inc = wave_incl_scan_u32(len, lane);
            const uint32_t T = __shfl(inc, 63);
            if (T > (uint32_t)kWCap) { giveup = true; break; }
            for (uint32_t u = 0; u < len; ++u) s_p[w][inc - len + u] = s + u;            // flatten the runs
            wave_lds_sync();
            double dmax = 0.0;
            for (uint32_t i = lane; i < T; i += 64) {
                const double4 a = *reinterpret_cast<const double4 *>(&recs[s_p[w][i]]);
                const double d = nd2(qx, qy, qz, a.x, a.y, a.z);
                s_d[w][i] = d;
                dmax = fmax(dmax, d);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, off));
            // stop rule of the grid engine for this cube: knn_stop_bound written out (through the call the compiler reads the whole
            // geometry ahead of the loop and the kernel takes a 98th VGPR)
            double L = INFINITY;
            {
                const double q[3] = {qx, qy, qz};
                const int c[3] = {cx, cy, cz};
                for (int a = 0; a < 3; ++a) {
                    if (c[a] - r > 0) L = fmin(L, (q[a] - (g.org[a] + (double)(c[a] - r) * g.h[a])) - g.slack[a]);
                    if (c[a] + r < g.dim[a] - 1) L = fmin(L, ((g.org[a] + (double)(c[a] + r + 1) * g.h[a]) - q[a]) - g.slack[a]);
                }
            }
            const bool whole = (L == INFINITY);                     // the cube covers the grid: these are all the points
            if (!whole && T < (uint32_t)k) continue;
            // k-th smallest distance tau by quickselect over the staged values; bracket: #(d <= lo) < kk <= #(d <= hi)
            const uint32_t kk = T < (uint32_t)k ? T : (uint32_t)k;
            double lo = -1.0, hi = dmax;
            for (;;) {
                double cand = 0.0;
                bool have = false;
                for (uint32_t i = lane; i < T && !have; i += 64) {
                    const double d = s_d[w][i];
                    if (d > lo && d < hi) { cand = d; have = true; }
                }
                const unsigned long long m = __ballot(have);
                if (!m) break;                                      // nothing strictly inside: tau = hi
                const double x = __shfl(cand, __ffsll((long long)m) - 1);
                uint32_t c = 0;
                for (uint32_t i = lane; i < T; i += 64) c += (s_d[w][i] <= x) ? 1u : 0u;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
                if (c >= kk) hi = x; else lo = x;
            }
            const double tau = hi;
            if (!whole && !(L > 0.0 && tau < L * L * (1.0 - 0x1.0p-30))) continue;        // try the next cube
            // ties at tau: the smaller rows win
            uint32_t below = 0, equal = 0;
            for (uint32_t i = lane; i < T; i += 64) {
                const double d = s_d[w][i];
                below += d < tau ? 1u : 0u;
                equal += d == tau ? 1u : 0u;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                below += __shfl_xor(below, off);
                equal += __shfl_xor(equal, off);
            }
            int row_cut = 0x7fffffff;                                // rows <= row_cut among the tied are taken
            if (below + equal > kk) {
                int last = -1;
                for (uint32_t need = kk - below; need > 0; --need) {                       // need-th smallest tied row
                    int best = 0x7fffffff;
                    for (uint32_t i = lane; i < T; i += 64)
                        if (s_d[w][i] == tau) {
                            const int row = recs[s_p[w][i]].idx;
                            if (row > last && row < best) best = row;
                        }
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off));
                    last = best;
                }
                row_cut = last;
            }
            // the kk selected candidates go to the front of the wave's LDS (in place: a selected entry only moves down), then to
            // the lane of their rank in ascending (d2, row) order: the sums below are then taken in an order that the neighbour
            // set alone decides -- the order of the records inside a cell (the grid build's atomics) does not reach the result
            uint32_t base = 0;
            for (uint32_t i0 = 0; i0 < T; i0 += 64) {
                const uint32_t i = i0 + lane;
                double d = 0.0;
                int row = 0;
                uint32_t rec = 0;
                bool sel = false;
                if (i < T) {
                    d = s_d[w][i];
                    if (d <= tau) {
                        rec = s_p[w][i];
                        row = recs[rec].idx;
                        sel = d < tau || row <= row_cut;
                    }
                }
                const unsigned long long m = __ballot(sel);
                wave_lds_sync();                                  // every lane has read its entry
                if (sel) {
                    const uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    s_d[w][pos] = d;
                    s_p[w][pos] = (uint32_t)row;
                    if (pos < (uint32_t)kKnnMax) s_r[w][pos] = rec;
                }
                base += (uint32_t)__popcll(m);
                wave_lds_sync();
            }
            const uint32_t nsel = base < kk ? base : kk;           // == kk (fewer only if distances are NaN: nothing unwritten is read)
            const bool own = (uint32_t)lane < nsel;                // lane l owns selected entry l
            int row = 0, rank = 0;
            uint32_t rec = 0;
            if (own) {
                const double d = s_d[w][lane];
                row = (int)s_p[w][lane];
                rec = s_r[w][lane];
                for (uint32_t j = 0; j < nsel; ++j) {
                    const double e = s_d[w][j];
                    const int r = (int)s_p[w][j];
                    rank += (e < d || (e == d && r < row)) ? 1 : 0;
                }
            }
            wave_lds_sync();                                      // every owner has read its record's position
            if (own) s_r[w][rank] = rec;
            wave_lds_sync();
            double dx = 0.0, dy = 0.0, dz = 0.0;                  // lane l: the neighbour of rank l (none: zeros)
            if (own) {
                const double4 a = *reinterpret_cast<const double4 *>(&recs[s_r[w][lane]]);
                dx = a.x - qx; dy = a.y - qy; dz = a.z - qz;
            }
            double m0 = wave_sum_f64(dx), m1 = wave_sum_f64(dy), m2 = wave_sum_f64(dz);
            const double s00 = wave_sum_f64(dx * dx), s01 = wave_sum_f64(dx * dy), s02 = wave_sum_f64(dx * dz);
            const double s11 = wave_sum_f64(dy * dy), s12 = wave_sum_f64(dy * dz), s22 = wave_sum_f64(dz * dz);
            if (lane == 0) {
                const double inv = 1.0 / (double)kk;
                m0 *= inv; m1 *= inv; m2 *= inv;
                double *o = cov_out + 6 * (int64_t)qrow;
                o[0] = s00 * inv - m0 * m0; o[1] = s01 * inv - m0 * m1; o[2] = s02 * inv - m0 * m2;
                o[3] = s11 * inv - m1 * m1; o[4] = s12 * inv - m1 * m2; o[5] = s22 * inv - m2 * m2;
                cnt_out[qrow] = (int)kk;
            }
            if (nbr_out && own) nbr_out[(int64_t)qrow * k + rank] = row;
            done = true;
        }
        if (!done && lane == 0) {
            cnt_out[qrow] = -1;                                       // k_knn_normals writes this normal itself
            todo[atomicAdd(todo_count, 1u)] = (uint32_t)t;
        }
        wave_lds_sync();                                              // LDS is reused by the next point
    }
}

// isolated points: exact k-NN by a full scan, one workgroup per point.  Every thread keeps the k best of its
// stride; the k global best are then extracted one by one with a workgroup-wide lexicographic minimum.
// (`qx64`: the queries' cloud -- the scanned cloud itself, or the other one for a search across the clouds)
__global__ __launch_bounds__(256) void k_knn_normals_full(const double *__restrict__ x64, const double *__restrict__ qx64, int64_t n, int k,
                                                          const int32_t *__restrict__ open_list,
                                                          const uint32_t *__restrict__ open_count,
                                                          double *__restrict__ nrm_out, int32_t *__restrict__ nbr_out,
                                                          int32_t *__restrict__ cnt_out)
{
    __shared__ double s_d[256];
    __shared__ int s_i[256];
    __shared__ int s_sel[kKnnMax];
    const int tid = threadIdx.x;
    const uint32_t count = *open_count;
    for (uint32_t f = blockIdx.x; f < count; f += gridDim.x) {
        const int qrow = open_list[f];
        const double qx = qx64[3 * (int64_t)qrow], qy = qx64[3 * (int64_t)qrow + 1], qz = qx64[3 * (int64_t)qrow + 2];
        double bd[kKnnMax];
        int bi[kKnnMax];
        int cnt = 0;
        for (int64_t j = tid; j < n; j += 256) knn_insert(bd, bi, k, cnt, nd2(qx, qy, qz, x64[3 * j], x64[3 * j + 1], x64[3 * j + 2]), (int)j);
        int head = 0, nsel = 0;
        const int want = n < k ? (int)n : k;
        for (int round = 0; round < want; ++round) {
            s_d[tid] = head < cnt ? bd[head] : INFINITY;
            s_i[tid] = head < cnt ? bi[head] : 0x7fffffff;
            __syncthreads();
            for (int off = 128; off > 0; off >>= 1) {
                if (tid < off) {
                    const double od = s_d[tid + off];
                    const int oi = s_i[tid + off];
                    if (od < s_d[tid] || (od == s_d[tid] && oi < s_i[tid])) { s_d[tid] = od; s_i[tid] = oi; }
                }
                __syncthreads();
            }
            const int win = s_i[0];
            if (head < cnt && bi[head] == win) ++head;      // rows are unique: exactly one thread owns the winner
            if (tid == 0) s_sel[nsel] = win;
            ++nsel;
            __syncthreads();
        }
        if (tid == 0 && nbr_out) ssim_neighbours_out(s_sel, nsel, k, qrow, nbr_out, cnt_out);
        else if (tid == 0) normal_from_neighbours(x64, qx, qy, qz, s_sel, nsel, nrm_out + 3 * (int64_t)qrow);
        __syncthreads();
    }
}

int knn_setup(pccm_ctx *ctx, int which, KnnGeom &g, const uint32_t *&cs, const GridRec *&crecs, const GridRec **qrecs)
{
    const Cloud &c = ctx->cloud[which];
    int rc;
    // GridRec (fp64) records of this cloud alone.  The pair's geometry follows the pair's larger cloud: fine for that cloud and for
    // one of similar size, hopeless for a much sparser one (a low rate of a codec: k = 30 neighbours then lie six rings out), which
    // gets cells of its own (grid_ensure_solo: a few histogram passes, cached with the cloud)
    const Cloud &other = ctx->cloud[1 - which];
    const bool solo = other.n > 2 * c.n;
    if (solo) {
        if ((rc = grid_ensure_solo(ctx, which))) return rc;
    } else if ((rc = grid_ensure(ctx, true, qrecs ? 3 : 1 << which))) return rc;
    const Grid &gr = ctx->grid;
    for (int a = 0; a < 3; ++a) {
        g.dim[a] = gr.dim[a];
        g.org[a] = gr.org[a];
        g.h[a] = gr.h[a];
        g.inv_h[a] = gr.inv_h[a];
        g.slack[a] = (fabs(gr.org[a]) + (gr.dim[a] + 2) * gr.h[a]) * 0x1.0p-48;
    }
    // cell_start holds positions relative to the cloud's first record
    cs = (const uint32_t *)gr.cell_start.p + (which ? gr.ncells + 1 : 0);
    crecs = (const GridRec *)gr.recs.p + (which ? gr.n[0] : 0);
    if (qrecs) *qrecs = solo ? nullptr : (const GridRec *)gr.recs.p + (which ? 0 : gr.n[0]);
    return PCCM_OK;
}

// scratch of the three searches: covariances + counts (ctx->val), points handed on (g_rank, g_cell_of) and their counters
int knn_scratch(pccm_ctx *ctx, int64_t n, double **cov, int32_t **cnt, uint32_t **open_count, uint32_t **todo_count)
{
    int rc;
    if ((rc = ensure(ctx, ctx->g_cell_of, (size_t)n * sizeof(uint32_t)))) return rc;   // reused: points left to the full scan
    if ((rc = ensure(ctx, ctx->g_rank, (size_t)n * sizeof(uint32_t)))) return rc;      // reused: points left to the per-thread search
    if ((rc = ensure(ctx, ctx->val, (size_t)n * (6 * sizeof(double) + sizeof(int32_t))))) return rc;   // covariances + counts
    if ((rc = ensure(ctx, ctx->g_blocksum, 256))) return rc;
    *open_count = (uint32_t *)ctx->g_blocksum.p;
    *todo_count = *open_count + 1;
    PCCM_HIP(hipMemsetAsync(*open_count, 0, 2 * sizeof(uint32_t), ctx->stream));
    *cov = (double *)ctx->val.p;
    *cnt = (int32_t *)(*cov + 6 * n);
    return PCCM_OK;
}

void launch_knn(pccm_ctx *ctx, const GridRec *crecs, const uint32_t *cs, const KnnGeom &g, const double *s64, int64_t ns,
                const GridRec *qrecs, const double *qx64, const double *q64, int64_t nq, int k, double *cov, int32_t *cnt,
                uint32_t *open_count, uint32_t *todo_count, KnnSink sink)
{
    int32_t *const lcnt = sink.nbr ? cnt : nullptr;        // (the lists' counts; a normal has none)
    const int64_t wblocks = (nq + 3) / 4;
    PCCM_LAUNCH(ctx, k_knn_cov_wave, dim3((unsigned)(wblocks < 16384 ? wblocks : 16384)), dim3(256), 0, ctx->stream,
                       crecs, qrecs, qx64, nq, g, cs, k, cov, cnt, (uint32_t *)ctx->g_rank.p, todo_count, sink.nbr);
    if (sink.nrm) launch_normals_from_cov(ctx, cov, cnt, nq, sink.nrm);
    PCCM_LAUNCH(ctx, k_knn_normals, dim3(2048), dim3(256), 0, ctx->stream, crecs, qrecs, qx64, g, cs,
                       s64, k, sink.nrm, (const uint32_t *)ctx->g_rank.p, (const uint32_t *)todo_count,
                       (int32_t *)ctx->g_cell_of.p, open_count, sink.nbr, lcnt);
    PCCM_LAUNCH(ctx, k_knn_normals_full, dim3(512), dim3(256), 0, ctx->stream, s64, q64, ns, k,
                       (const int32_t *)ctx->g_cell_of.p, (const uint32_t *)open_count, sink.nrm, sink.nbr, lcnt);
}

}  // namespace pccm
