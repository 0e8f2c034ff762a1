// Normal estimation on the GPU.
//
// Stands under `clouds[k].estimate_normals()` in CloudPair.__init__, open_pcc_metric/cloud_pair.py:61-64,
// i.e. Open3D 0.18 PointCloud::EstimateNormals with its defaults (KDTreeSearchParamKNN(knn = 30),
// fast_normal_computation): for every point, the covariance of its 30 nearest points of the same cloud
// (the point itself included) and the eigenvector of the smallest eigenvalue.  Open3D is not in the
// reference checkout, so this is a restatement of the published algorithm and is NOT parity-pinned (tests/test_gpu_normals.py holds
// every point to a high-precision reference within a tolerance that follows the conditioning of its own eigenproblem, per k, data
// family, slot, grid choice and stage of the search -- still not Open3D parity):
//   - neighbours: exact k-NN, squared distance in fp64 ((dx*dx)+(dy*dy))+(dz*dz), ties to the smaller row;
//   - covariance: E[d d^T] - E[d] E[d]^T with d = p - q (Open3D forms the same matrix from raw moments;
//     shifting by the query point only improves the conditioning);
//   - eigenvector: closed-form eigenvalues of the symmetric 3x3 (trigonometric form on the scaled matrix)
//     and the largest cross product of two rows of (C - lambda I), as in Open3D's FastEigen3x3;
//   - fewer than 3 points in the cloud, or a degenerate covariance: (0, 0, 1) (Open3D's default normal);
//   - sign: Open3D leaves it to the eigen-solver; here the component of largest magnitude is made positive.
//     D2 squares the projection (metric.py:179), so no metric depends on the sign.
// The neighbours come from the grid engine's cell-sorted records: one thread per point scans the cube
// [c-r, c+r]^3 ring by ring, keeping the k best (d2, row) in a sorted private list, until the k-th best is
// provably closer than anything outside the cube (same stop rule as the 1-NN search).  Points that are
// still open after kKnnMaxRing rings (isolated outliers) are finished by an exact block-per-point scan of
// the whole cloud.
//
// PointSSIM features (pccm_ssim_features, INTEGRATION.md "PointSSIM") reuse the same three searches: given a neighbour list
// (nbr_out, [n][k] int32), each of them writes the point's neighbours in ascending (d2, row) order and their count instead of a
// normal.  k_normals_from_cov then runs again: for the curvature of every point (mode 1) and for the features (mode 2), both from
// the neighbour lists -- the covariance behind a curvature is summed in neighbourhood order, not in the search's order (which
// follows the grid, and so the other cloud of the pair), so that a cloud's features do not depend on the pair it is in.
//
// Point-to-distribution (pccm_p2d_build, INTEGRATION.md "Point-to-distribution") runs the three searches ACROSS the clouds: the
// queries are the points of one cloud (query_at), the candidates the cells of the other.  A query's cell comes from its
// coordinates through ncell_coord, which clamps, so a query may lie outside the searched cloud's grid.  The stop rule stays a
// valid lower bound: L only counts a face of the cube [c-r, c+r]^3 that is not a face of the grid, and on every axis the query
// lies between the two faces of its cube or beyond the one that is the grid's (where no point of the searched cloud can be: the
// grid's boundary cells hold everything that clamps into them).  A point outside the cube is beyond a counted face, at least
// (face - q) - slack away along that axis, exactly as for a query inside the grid.  k_normals_from_cov (mode 3) then forms the
// Mahalanobis distance of every query to its neighbours' distribution from the neighbour lists.
#include "pccm_internal.h"

namespace pccm {

constexpr int kKnnMax = 64;        // largest supported k
constexpr int kKnnMaxRing = 6;

struct KnnGeom {
    int dim[3];
    double org[3], h[3], inv_h[3], slack[3];
};

__device__ __forceinline__ int ncell_coord(double v, double org, double inv_h, int dim)
{
    double t = floor(__dmul_rn(__dsub_rn(v, org), inv_h));
    t = t < 0.0 ? 0.0 : t;
    const double top = (double)(dim - 1);
    t = t > top ? top : t;
    return (int)t;
}

__device__ __forceinline__ double nd2(double qx, double qy, double qz, double rx, double ry, double rz)
{
    double dx = __dsub_rn(qx, rx), dy = __dsub_rn(qy, ry), dz = __dsub_rn(qz, rz);
    double d = __dmul_rn(dx, dx);
    d = __dadd_rn(d, __dmul_rn(dy, dy));
    d = __dadd_rn(d, __dmul_rn(dz, dz));
    return d;
}

// The query a search thread or wave works on: record t of `qrecs` (cell-sorted records: the searched cloud's own slice, or the
// other cloud's slice of the pair's grid), or -- qrecs null -- row t of `qx64` (a cloud that is not in the searched grid)
__device__ __forceinline__ void query_at(const GridRec *__restrict__ qrecs, const double *__restrict__ qx64, int64_t t, double &qx,
                                         double &qy, double &qz, int &qrow)
{
    if (qrecs) {
        const double4 qa = *reinterpret_cast<const double4 *>(&qrecs[t]);
        qx = qa.x; qy = qa.y; qz = qa.z;
        qrow = (int)(__double_as_longlong(qa.w) & 0xffffffffll);
    } else {
        qx = qx64[3 * t]; qy = qx64[3 * t + 1]; qz = qx64[3 * t + 2];
        qrow = (int)t;
    }
}

// sorted insertion of (d, row) into the k best kept in ascending (d, row) order
__device__ __forceinline__ void knn_insert(double *bd, int *bi, int k, int &cnt, double d, int row)
{
    if (cnt == k && !(d < bd[k - 1] || (d == bd[k - 1] && row < bi[k - 1]))) return;
    int p = cnt < k ? cnt : k - 1;
    while (p > 0 && (d < bd[p - 1] || (d == bd[p - 1] && row < bi[p - 1]))) {
        bd[p] = bd[p - 1];
        bi[p] = bi[p - 1];
        --p;
    }
    bd[p] = d;
    bi[p] = row;
    if (cnt < k) ++cnt;
}

// smallest eigenvalue of the symmetric matrix [a00 a01 a02; a01 a11 a12; a02 a12 a22] (closed form, trigonometric)
__device__ __forceinline__ double smallest_eigenvalue(double a00, double a01, double a02, double a11, double a12, double a22)
{
    const double norm = a01 * a01 + a02 * a02 + a12 * a12;
    if (!(norm > 0.0)) return fmin(a00, fmin(a11, a22));
    const double q = (a00 + a11 + a22) / 3.0;
    const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
    const double p = sqrt((b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * norm) / 6.0);
    const double c00 = b11 * b22 - a12 * a12, c01 = a01 * b22 - a12 * a02, c02 = a01 * a12 - b11 * a02;
    const double det = (b00 * c00 - a01 * c01 + a02 * c02) / (p * p * p);
    const double half = fmin(fmax(0.5 * det, -1.0), 1.0);
    const double angle = acos(half) / 3.0;
    return q + 2.0 * p * cos(angle + 2.0943951023931953);          // smallest root: + 2*pi/3
}

// eigenvector of the smallest eigenvalue of the symmetric matrix [a00 a01 a02; a01 a11 a12; a02 a12 a22]
__device__ void smallest_eigenvector(double a00, double a01, double a02, double a11, double a12, double a22, double n[3])
{
    n[0] = 0.0; n[1] = 0.0; n[2] = 1.0;
    double mx = fmax(fmax(fabs(a00), fabs(a11)), fmax(fabs(a22), fmax(fabs(a01), fmax(fabs(a02), fabs(a12)))));
    if (!(mx > 0.0)) return;
    const double s = 1.0 / mx;
    a00 *= s; a01 *= s; a02 *= s; a11 *= s; a12 *= s; a22 *= s;
    const double lam = smallest_eigenvalue(a00, a01, a02, a11, a12, a22);
    // rows of (A - lam I); the eigenvector is orthogonal to all of them: take the best-conditioned cross product
    const double r0[3] = {a00 - lam, a01, a02}, r1[3] = {a01, a11 - lam, a12}, r2[3] = {a02, a12, a22 - lam};
    double c[3][3];
    c[0][0] = r0[1] * r1[2] - r0[2] * r1[1]; c[0][1] = r0[2] * r1[0] - r0[0] * r1[2]; c[0][2] = r0[0] * r1[1] - r0[1] * r1[0];
    c[1][0] = r0[1] * r2[2] - r0[2] * r2[1]; c[1][1] = r0[2] * r2[0] - r0[0] * r2[2]; c[1][2] = r0[0] * r2[1] - r0[1] * r2[0];
    c[2][0] = r1[1] * r2[2] - r1[2] * r2[1]; c[2][1] = r1[2] * r2[0] - r1[0] * r2[2]; c[2][2] = r1[0] * r2[1] - r1[1] * r2[0];
    int best = 0;
    double bl = -1.0;
    for (int k = 0; k < 3; ++k) {
        const double l = c[k][0] * c[k][0] + c[k][1] * c[k][1] + c[k][2] * c[k][2];
        if (l > bl) { bl = l; best = k; }
    }
    if (!(bl > 1.0e-280)) return;                           // (numerically) isotropic or rank-0 spread
    const double inv = 1.0 / sqrt(bl);
    double v0 = c[best][0] * inv, v1 = c[best][1] * inv, v2 = c[best][2] * inv;
    const double m0 = fabs(v0), m1 = fabs(v1), m2 = fabs(v2);
    const double lead = (m0 >= m1 && m0 >= m2) ? v0 : (m1 >= m2 ? v1 : v2);
    if (lead < 0.0) { v0 = -v0; v1 = -v1; v2 = -v2; }
    n[0] = v0; n[1] = v1; n[2] = v2;
}

__device__ void normal_from_neighbours(const double *__restrict__ x64, double qx, double qy, double qz, const int *bi, int cnt,
                                       double *__restrict__ out)
{
    double n[3] = {0.0, 0.0, 1.0};
    if (cnt >= 3) {
        double m0 = 0, m1 = 0, m2 = 0, s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0;
        for (int k = 0; k < cnt; ++k) {
            const double *p = x64 + 3 * (int64_t)bi[k];
            const double dx = p[0] - qx, dy = p[1] - qy, dz = p[2] - qz;
            m0 += dx; m1 += dy; m2 += dz;
            s00 += dx * dx; s01 += dx * dy; s02 += dx * dz; s11 += dy * dy; s12 += dy * dz; s22 += dz * dz;
        }
        const double inv = 1.0 / (double)cnt;
        m0 *= inv; m1 *= inv; m2 *= inv;
        smallest_eigenvector(s00 * inv - m0 * m0, s01 * inv - m0 * m1, s02 * inv - m0 * m2, s11 * inv - m1 * m1,
                             s12 * inv - m1 * m2, s22 * inv - m2 * m2, n);
    }
    out[0] = n[0]; out[1] = n[1]; out[2] = n[2];
}

// PointSSIM: the neighbour rows (ascending (d2, row)) and their count
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
        double L = INFINITY;
        const double q[3] = {qx, qy, qz};
        const int c[3] = {cx, cy, cz};
        for (int a = 0; a < 3; ++a) {
            if (c[a] - r > 0) L = fmin(L, (q[a] - (g.org[a] + (double)(c[a] - r) * g.h[a])) - g.slack[a]);
            if (c[a] + r < g.dim[a] - 1) L = fmin(L, ((g.org[a] + (double)(c[a] + r + 1) * g.h[a]) - q[a]) - g.slack[a]);
        }
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
constexpr int kWCap = 512;

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
            uint32_t inc = len;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t o = __shfl_up(inc, off);
                if (lane >= off) inc += o;
            }
            const uint32_t T = __shfl(inc, 63);
            if (T > (uint32_t)kWCap) { giveup = true; break; }
            for (uint32_t u = 0; u < len; ++u) s_p[w][inc - len + u] = s + u;            // flatten the runs
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            double dmax = 0.0;
            for (uint32_t i = lane; i < T; i += 64) {
                const double4 a = *reinterpret_cast<const double4 *>(&recs[s_p[w][i]]);
                const double d = nd2(qx, qy, qz, a.x, a.y, a.z);
                s_d[w][i] = d;
                dmax = fmax(dmax, d);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, off));
            // stop rule of the grid engine for this cube
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
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");        // LDS is reused by the next point
        __builtin_amdgcn_wave_barrier();
    }
}

// One Jacobi rotation of the symmetric 3x3 in the plane (p, q): app, aqq the two diagonal entries, apq the entry it annihilates,
// arp, arq the two entries of the third row (Rutishauser's update: the diagonal moves by t * apq)
__device__ __forceinline__ void jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // (theta^2 = inf: t = 0)
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double h = t * apq;
    app -= h;
    aqq += h;
    apq = 0.0;
    const double g = arp;
    arp = c * g - s * arq;
    arq = s * g + c * arq;
}

// smallest eigenvalue of the symmetric matrix [a00 a01 a02; a01 a11 a12; a02 a12 a22], SCALED so that its largest entry is 1, by
// cyclic Jacobi sweeps: the absolute error is a few ulps of the matrix norm whatever the spectrum -- also where the two smallest
// eigenvalues meet (collinear neighbourhoods), where the closed form's acos keeps only half the digits.  The sweeps end when the
// off-diagonal entries are below 2^-54 (each moves an eigenvalue by no more than itself); convergence is quadratic, 3 to 5 sweeps.
__device__ __forceinline__ double smallest_eigenvalue_jacobi(double a00, double a01, double a02, double a11, double a12, double a22)
{
    for (int sweep = 0; sweep < 8; ++sweep) {
        if ((fabs(a01) + fabs(a02)) + fabs(a12) <= 0x1.0p-54) break;
        jacobi_rotate(a00, a11, a01, a02, a12);
        jacobi_rotate(a00, a22, a02, a01, a12);
        jacobi_rotate(a11, a22, a12, a01, a02);
    }
    return fmin(a00, fmin(a11, a22));
}

// PointSSIM curvature of point p: lambda_min / trace of the covariance normal_from_neighbours forms (E[d d^T] - E[d] E[d]^T,
// d = q - p), summed in neighbourhood order; scale-free (taken on the matrix scaled as for the normal), 0 when the trace is 0.
// lambda_min comes from Jacobi sweeps, not from smallest_eigenvalue: c is perfectly conditioned, the closed form is not.
__device__ __forceinline__ double curvature_of(const double *__restrict__ x64, int64_t p, const int32_t *__restrict__ row, int cnt)
{
    const double qx = x64[3 * p], qy = x64[3 * p + 1], qz = x64[3 * p + 2];
    double m0 = 0, m1 = 0, m2 = 0, s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0;
    for (int j = 0; j < cnt; ++j) {
        const double *q = x64 + 3 * (int64_t)row[j];
        const double dx = q[0] - qx, dy = q[1] - qy, dz = q[2] - qz;
        m0 += dx; m1 += dy; m2 += dz;
        s00 += dx * dx; s01 += dx * dy; s02 += dx * dz; s11 += dy * dy; s12 += dy * dz; s22 += dz * dz;
    }
    const double inv = 1.0 / (double)cnt;
    m0 *= inv; m1 *= inv; m2 *= inv;
    const double a[6] = {s00 * inv - m0 * m0, s01 * inv - m0 * m1, s02 * inv - m0 * m2,
                         s11 * inv - m1 * m1, s12 * inv - m1 * m2, s22 * inv - m2 * m2};
    double mx = fmax(fmax(fabs(a[0]), fabs(a[3])), fmax(fabs(a[5]), fmax(fabs(a[1]), fmax(fabs(a[2]), fabs(a[4])))));
    if (!(mx > 0.0)) return 0.0;
    const double s = 1.0 / mx;
    const double a00 = a[0] * s, a01 = a[1] * s, a02 = a[2] * s, a11 = a[3] * s, a12 = a[4] * s, a22 = a[5] * s;
    const double tr = (a00 + a11) + a22;
    if (tr == 0.0) return 0.0;
    return smallest_eigenvalue_jacobi(a00, a01, a02, a11, a12, a22) / tr;
}

// PointSSIM value of neighbour j of row p for attribute a (0 geometry, 1 normal, 2 curvature, 3 colour; include/pccm.h)
__device__ __forceinline__ double ssim_value(int a, int64_t p, int64_t q, const double *__restrict__ x64, const double *__restrict__ nrm64,
                                             const double *__restrict__ curv, const double *__restrict__ rgb64)
{
    if (a == 0) return __dsqrt_rn(nd2(x64[3 * p], x64[3 * p + 1], x64[3 * p + 2], x64[3 * q], x64[3 * q + 1], x64[3 * q + 2]));
    if (a == 1) return angular_similarity(nrm64 + 3 * p, nrm64 + 3 * q);
    if (a == 2) return curv[q];
    // luma: row 0 of the "ycc" matrix as pccm_color.hip's to_scheme (and transform_colors) evaluates it
    const double *c = rgb64 + 3 * q;
    return fma(0.0722, c[2], fma(0.2126, c[0], __dmul_rn(0.7152, c[1])));
}

// Point-to-distribution value of query i (include/pccm.h, pccm_p2d_build): the Mahalanobis distance from the query p to the
// distribution of its cnt neighbours `row` (rows of x64, ascending (d2, row)).  Moments of e_j = q_j - p summed left to right in
// neighbourhood order, population covariance, a ridge of 2^-10 of the trace on the diagonal, the quadratic form by cofactors.
// Every operation is rounded separately, in the order INTEGRATION.md writes it: a NumPy restatement gives the same bits.
__device__ __forceinline__ double p2d_value(const double *__restrict__ x64, const double *__restrict__ q64, int64_t i,
                                            const int32_t *__restrict__ row, int cnt)
{
    const double px = q64[3 * i], py = q64[3 * i + 1], pz = q64[3 * i + 2];
    double s0 = 0, s1 = 0, s2 = 0, s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0;
    for (int j = 0; j < cnt; ++j) {
        const double *q = x64 + 3 * (int64_t)row[j];
        const double e0 = __dsub_rn(q[0], px), e1 = __dsub_rn(q[1], py), e2 = __dsub_rn(q[2], pz);
        s0 = __dadd_rn(s0, e0); s1 = __dadd_rn(s1, e1); s2 = __dadd_rn(s2, e2);
        s00 = __dadd_rn(s00, __dmul_rn(e0, e0)); s01 = __dadd_rn(s01, __dmul_rn(e0, e1)); s02 = __dadd_rn(s02, __dmul_rn(e0, e2));
        s11 = __dadd_rn(s11, __dmul_rn(e1, e1)); s12 = __dadd_rn(s12, __dmul_rn(e1, e2)); s22 = __dadd_rn(s22, __dmul_rn(e2, e2));
    }
    const double kk = (double)cnt;
    const double m0 = __ddiv_rn(s0, kk), m1 = __ddiv_rn(s1, kk), m2 = __ddiv_rn(s2, kk);
    const double C00 = __dsub_rn(__ddiv_rn(s00, kk), __dmul_rn(m0, m0)), c01 = __dsub_rn(__ddiv_rn(s01, kk), __dmul_rn(m0, m1));
    const double c02 = __dsub_rn(__ddiv_rn(s02, kk), __dmul_rn(m0, m2)), C11 = __dsub_rn(__ddiv_rn(s11, kk), __dmul_rn(m1, m1));
    const double c12 = __dsub_rn(__ddiv_rn(s12, kk), __dmul_rn(m1, m2)), C22 = __dsub_rn(__ddiv_rn(s22, kk), __dmul_rn(m2, m2));
    const double t = __dadd_rn(__dadd_rn(C00, C11), C22);
    const double lam = __dmul_rn(t, 0x1.0p-10);
    const double c00 = __dadd_rn(C00, lam), c11 = __dadd_rn(C11, lam), c22 = __dadd_rn(C22, lam);
    const double f00 = __dsub_rn(__dmul_rn(c11, c22), __dmul_rn(c12, c12)), f01 = __dsub_rn(__dmul_rn(c02, c12), __dmul_rn(c01, c22));
    const double f02 = __dsub_rn(__dmul_rn(c01, c12), __dmul_rn(c02, c11)), f11 = __dsub_rn(__dmul_rn(c00, c22), __dmul_rn(c02, c02));
    const double f12 = __dsub_rn(__dmul_rn(c01, c02), __dmul_rn(c00, c12)), f22 = __dsub_rn(__dmul_rn(c00, c11), __dmul_rn(c01, c01));
    const double det = __dadd_rn(__dadd_rn(__dmul_rn(c00, f00), __dmul_rn(c01, f01)), __dmul_rn(c02, f02));
    if (!(t > 0.0) || !(det > 0.0)) return (m0 == 0.0 && m1 == 0.0 && m2 == 0.0) ? 0.0 : INFINITY;
    const double v0 = __dadd_rn(__dadd_rn(__dmul_rn(f00, m0), __dmul_rn(f01, m1)), __dmul_rn(f02, m2));
    const double v1 = __dadd_rn(__dadd_rn(__dmul_rn(f01, m0), __dmul_rn(f11, m1)), __dmul_rn(f12, m2));
    const double v2 = __dadd_rn(__dadd_rn(__dmul_rn(f02, m0), __dmul_rn(f12, m1)), __dmul_rn(f22, m2));
    const double quad = __dadd_rn(__dadd_rn(__dmul_rn(m0, v0), __dmul_rn(m1, v1)), __dmul_rn(m2, v2));
    const double r = __ddiv_rn(quad, det);
    return __dsqrt_rn(r > 0.0 ? r : 0.0);
}

// luma (ssim_value, a == 3) of row r of a cloud's colours: from the packed bytes `c8` (r | g << 8 | b << 16) when the cloud has them
// -- 4 bytes per gathered row instead of 24; k / 255.0 is the very double rgb64 holds, so the bits agree -- or from rgb64
__device__ __forceinline__ double p2d_luma(const uint32_t *__restrict__ c8, const double *__restrict__ rgb64, int64_t r)
{
    double c0, c1, c2;
    if (c8) {
        const uint32_t w = c8[r];
        c0 = __ddiv_rn((double)(w & 0xffu), 255.0);
        c1 = __ddiv_rn((double)((w >> 8) & 0xffu), 255.0);
        c2 = __ddiv_rn((double)((w >> 16) & 0xffu), 255.0);
    } else {
        const double *c = rgb64 + 3 * r;
        c0 = c[0]; c1 = c[1]; c2 = c[2];
    }
    return fma(0.0722, c2, fma(0.2126, c0, __dmul_rn(0.7152, c1)));
}

// Colour point-to-distribution value M_Y of query i (include/pccm.h, pccm_p2d_build_attrs): the distance of the query's luma to
// the luma distribution of its cnt neighbours `row` (rows of the searched cloud, ascending (d2, row)), in standard deviations.
// Moments of e_j = y(q_j) - y(p) summed left to right; the variance is clamped at 0 (it rounds below it where the neighbourhood's
// luma is flat) and ridged by 2^-20.  Every operation is rounded separately, in the order INTEGRATION.md writes it.
__device__ __forceinline__ double p2d_color_value(const uint32_t *__restrict__ s8, const double *__restrict__ srgb64,
                                                  const uint32_t *__restrict__ q8, const double *__restrict__ qrgb64, int64_t i,
                                                  const int32_t *__restrict__ row, int cnt)
{
    const double yp = p2d_luma(q8, qrgb64, i);
    double s1 = 0, s2 = 0;
    for (int j = 0; j < cnt; ++j) {
        const double e = __dsub_rn(p2d_luma(s8, srgb64, row[j]), yp);
        s1 = __dadd_rn(s1, e);
        s2 = __dadd_rn(s2, __dmul_rn(e, e));
    }
    const double kk = (double)cnt;
    const double m = __ddiv_rn(s1, kk);
    const double V = __dsub_rn(__ddiv_rn(s2, kk), __dmul_rn(m, m));
    const double v = __dadd_rn(V < 0.0 ? 0.0 : V, 0x1.0p-20);
    return __ddiv_rn(fabs(m), __dsqrt_rn(v));
}

// mode 0: normals from the covariances (the per-thread kernels write their own: cnt < 0)
// mode 1 (PointSSIM): curvature of every point -> curv[n], from the neighbour lists nbr[n][k] (cnt[i] entries)
// mode 2 (PointSSIM): the features of the attributes in `attrs` -> feat[a][n], from the neighbour lists nbr[n][k] (cnt[i] entries):
//   m values v_j over N_k(p), mu = (sum v_j) / m, F = (sum (v_j - mu)^2) / (m - 1), F = 0 for m < 2; left-to-right sums, every
//   operation separately rounded.  Geometry and normal skip q_0 (the point itself).  The values are formed twice (two passes)
//   instead of being kept: up to 64 of them per thread would live in scratch memory.
// mode 3 (point-to-distribution): p2d_value of every query i (row i of q64) -> nrm_out[n], from its neighbour list nbr[n][k] of rows
//   of x64 (cnt[i] entries)
// mode 4 (point-to-distribution, colour and joint): p2d_color_value M_Y of every query i -> nrm_out[n] and the joint value
//   sqrt(M_G * M_G + M_Y * M_Y) -> curv[n], M_G = cov[i] (the column mode 3 wrote), from the same neighbour list; the searched
//   cloud's colours are s8 (packed bytes) or else rgb64, the queries' q8 or else q64 (here the queries' COLOUR rows)
__global__ __launch_bounds__(256) void k_normals_from_cov(const double *__restrict__ cov, const int32_t *__restrict__ cnt, int64_t n,
                                                          double *__restrict__ nrm_out, int mode, const int32_t *__restrict__ nbr, int k,
                                                          const double *__restrict__ x64, const double *__restrict__ nrm64,
                                                          const double *__restrict__ rgb64, double *__restrict__ curv,
                                                          double *__restrict__ feat, int attrs, const double *__restrict__ q64,
                                                          const uint32_t *__restrict__ s8, const uint32_t *__restrict__ q8)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (mode == 4) {
        const double my = p2d_color_value(s8, rgb64, q8, q64, i, nbr + i * k, cnt[i]);
        const double mg = cov[i];
        nrm_out[i] = my;
        curv[i] = __dsqrt_rn(__dadd_rn(__dmul_rn(mg, mg), __dmul_rn(my, my)));
        return;
    }
    if (mode == 3) {
        nrm_out[i] = p2d_value(x64, q64, i, nbr + i * k, cnt[i]);
        return;
    }
    if (mode == 1) {
        curv[i] = curvature_of(x64, i, nbr + i * k, cnt[i]);
        return;
    }
    if (mode == 2) {
        const int32_t *row = nbr + i * k;
        const int c = cnt[i];
        for (int a = 0; a < 4; ++a) {
            if (!(attrs & (1 << a))) continue;
            const int j0 = (a <= 1) ? 1 : 0;
            const int m = c - j0;
            double f = 0.0;
            if (m >= 2) {
                double sum = 0.0;
                for (int j = j0; j < c; ++j) sum = __dadd_rn(sum, ssim_value(a, i, row[j], x64, nrm64, curv, rgb64));
                const double mu = __ddiv_rn(sum, (double)m);
                double sq = 0.0;
                for (int j = j0; j < c; ++j) {
                    const double e = __dsub_rn(ssim_value(a, i, row[j], x64, nrm64, curv, rgb64), mu);
                    sq = __dadd_rn(sq, __dmul_rn(e, e));
                }
                f = __ddiv_rn(sq, (double)(m - 1));
            }
            feat[(int64_t)a * n + i] = f;
        }
        return;
    }
    const int c = cnt[i];
    if (c < 0) return;                                               // settled by the per-thread kernel
    double nn[3] = {0.0, 0.0, 1.0};
    const double *a = cov + 6 * i;
    if (c >= 3) smallest_eigenvector(a[0], a[1], a[2], a[3], a[4], a[5], nn);
    nrm_out[3 * i] = nn[0];
    nrm_out[3 * i + 1] = nn[1];
    nrm_out[3 * i + 2] = nn[2];
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

// the grid the k-NN searches of cloud `which` run on, its cell starts and records (shared by estimate_normals, ssim_features and
// the point-to-distribution search).  `qrecs` (the search across the clouds): the OTHER cloud's cell-sorted records when both
// clouds sit in the pair's grid -- queries taken in that order walk the same cells wave after wave -- or null when `which` has
// cells of its own, which only sort `which`
static int knn_setup(pccm_ctx *ctx, int which, KnnGeom &g, const uint32_t *&cs, const GridRec *&crecs, const GridRec **qrecs = nullptr)
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
static int knn_scratch(pccm_ctx *ctx, int64_t n, double **cov, int32_t **cnt, uint32_t **open_count, uint32_t **todo_count)
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

// the three searches in neighbour-list mode: for each of the nq queries (qrecs / qx64: query_at; q64: their cloud's rows, which
// the full scan reads) its k nearest points of the searched cloud (crecs, cs, s64, ns points) -> nbr[nq][k], cnt[nq] by query row
static void launch_knn_lists(pccm_ctx *ctx, const GridRec *crecs, const uint32_t *cs, const KnnGeom &g, const double *s64, int64_t ns,
                             const GridRec *qrecs, const double *qx64, const double *q64, int64_t nq, int k, double *cov, int32_t *cnt,
                             uint32_t *open_count, uint32_t *todo_count, int32_t *nbr)
{
    const int64_t wblocks = (nq + 3) / 4;
    PCCM_LAUNCH(ctx, k_knn_cov_wave, dim3((unsigned)(wblocks < 16384 ? wblocks : 16384)), dim3(256), 0, ctx->stream,
                       crecs, qrecs, qx64, nq, g, cs, k, cov, cnt, (uint32_t *)ctx->g_rank.p, todo_count, nbr);
    PCCM_LAUNCH(ctx, k_knn_normals, dim3(2048), dim3(256), 0, ctx->stream, crecs, qrecs, qx64, g, cs,
                       s64, k, (double *)nullptr, (const uint32_t *)ctx->g_rank.p, (const uint32_t *)todo_count,
                       (int32_t *)ctx->g_cell_of.p, open_count, nbr, cnt);
    PCCM_LAUNCH(ctx, k_knn_normals_full, dim3(512), dim3(256), 0, ctx->stream, s64, q64, ns, k,
                       (const int32_t *)ctx->g_cell_of.p, (const uint32_t *)open_count, (double *)nullptr, nbr, cnt);
}

int estimate_normals(pccm_ctx *ctx, int which, int k)
{
    Cloud &c = ctx->cloud[which];
    if (c.n <= 0) return fail(PCCM_E_STATE, "cloud %d is not set", which);
    if (k < 3 || k > kKnnMax) return fail(PCCM_E_ARG, "k must be in 3..%d", kKnnMax);
    int rc;
    KnnGeom g;
    const uint32_t *cs;
    const GridRec *crecs;
    if ((rc = knn_setup(ctx, which, g, cs, crecs))) return rc;
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    if ((rc = grow((void **)&c.nrm64, c.cap_nrm, (size_t)c.n * 3 * sizeof(double)))) return rc;
    c.n_nrm = c.n;
    c.nrm_exact32 = false;
    c.nrm_deferred = false;
    c.nrm_host = nullptr;
    c.ssim_attrs &= ~PCCM_SSIM_NORMAL;
    for (int d = 0; d < 3; ++d) ctx->nn_gen[d]++;      // pending D2 reductions would use stale normals
    ctx->epoch++;
    double *cov;
    int32_t *cnt;
    uint32_t *open_count, *todo_count;
    if ((rc = knn_scratch(ctx, c.n, &cov, &cnt, &open_count, &todo_count))) return rc;
    const int64_t wblocks = (c.n + 3) / 4;
    PCCM_LAUNCH(ctx, k_knn_cov_wave, dim3((unsigned)(wblocks < 16384 ? wblocks : 16384)), dim3(256), 0, ctx->stream,
                       crecs, crecs, (const double *)nullptr, c.n, g, cs, k, cov, cnt, (uint32_t *)ctx->g_rank.p, todo_count,
                       (int32_t *)nullptr);
    PCCM_LAUNCH(ctx, k_normals_from_cov, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)cov,
                       (const int32_t *)cnt, c.n, c.nrm64, 0, (const int32_t *)nullptr, k, (const double *)nullptr,
                       (const double *)nullptr, (const double *)nullptr, (double *)nullptr, (double *)nullptr, 0,
                       (const double *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr);
    PCCM_LAUNCH(ctx, k_knn_normals, dim3(2048), dim3(256), 0, ctx->stream, crecs, crecs, (const double *)nullptr, g, cs,
                       (const double *)c.xyz64, k, c.nrm64, (const uint32_t *)ctx->g_rank.p, (const uint32_t *)todo_count,
                       (int32_t *)ctx->g_cell_of.p, open_count, (int32_t *)nullptr, (int32_t *)nullptr);
    PCCM_LAUNCH(ctx, k_knn_normals_full, dim3(512), dim3(256), 0, ctx->stream, (const double *)c.xyz64, (const double *)c.xyz64,
                       c.n, k, (const int32_t *)ctx->g_cell_of.p, (const uint32_t *)open_count, c.nrm64, (int32_t *)nullptr,
                       (int32_t *)nullptr);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

// PointSSIM features of cloud `which` (pccm_ssim_features has checked k, the mask and the inputs it needs).  The same three
// searches as estimate_normals, in neighbour-list mode (every point's k rows in (d2, row) order and their count), then
// k_normals_from_cov for the curvatures and for the features.  Neighbour lists and curvatures are scratch: 4 k + 8 bytes per point.
int ssim_features(pccm_ctx *ctx, int which, int k, int attrs, int *built)
{
    Cloud &c = ctx->cloud[which];
    if (built) *built = 0;
    if (c.ssim_k == k && (c.ssim_attrs & attrs) == attrs) return PCCM_OK;
    if (ctx->capturing) {
        ctx->capture_failed = true;
        return fail(PCCM_E_STATE, "PointSSIM features are built before graph capture");
    }
    if (c.ssim_k == k) attrs |= c.ssim_attrs;         // (what is there is made again with the rest: one pass)
    int rc;
    KnnGeom g;
    const uint32_t *cs;
    const GridRec *crecs;
    if ((rc = knn_setup(ctx, which, g, cs, crecs))) return rc;
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    const double *ssim_before = c.ssim64;
    if ((rc = grow((void **)&c.ssim64, c.cap_ssim, (size_t)c.n * 4 * sizeof(double)))) return rc;
    c.ssim_attrs = 0;
    for (int d = 0; d < 3; ++d) ctx->nn_gen[d]++;      // pending PointSSIM reductions would use stale features
    if (c.ssim64 != ssim_before) ctx->epoch++;          // (graphs that read the old columns are stale)
    double *cov;
    int32_t *cnt;
    uint32_t *open_count, *todo_count;
    if ((rc = knn_scratch(ctx, c.n, &cov, &cnt, &open_count, &todo_count))) return rc;
    const size_t nbr_words = ((size_t)c.n * k + 1) & ~(size_t)1;          // (the curvatures behind them stay 8-byte aligned)
    if ((rc = ensure(ctx, ctx->ssim_scratch, nbr_words * sizeof(int32_t) + (size_t)c.n * sizeof(double)))) return rc;
    int32_t *nbr = (int32_t *)ctx->ssim_scratch.p;
    double *curv = (double *)(nbr + nbr_words);
    const dim3 pgrid((unsigned)((c.n + 255) / 256));
    launch_knn_lists(ctx, crecs, cs, g, c.xyz64, c.n, crecs, nullptr, c.xyz64, c.n, k, cov, cnt, open_count, todo_count, nbr);
    if (attrs & PCCM_SSIM_CURVATURE)
        PCCM_LAUNCH(ctx, k_normals_from_cov, pgrid, dim3(256), 0, ctx->stream, (const double *)nullptr, (const int32_t *)cnt, c.n,
                           (double *)nullptr, 1, (const int32_t *)nbr, k, (const double *)c.xyz64, (const double *)nullptr,
                           (const double *)nullptr, curv, (double *)nullptr, 0, (const double *)nullptr, (const uint32_t *)nullptr,
                           (const uint32_t *)nullptr);
    // one launch per attribute: at 1M points and k = 12 the four attributes take 2.25 ms in one launch, 1.99 ms in four
    for (int a = 0; a < 4; ++a)
        if (attrs & (1 << a))
            PCCM_LAUNCH(ctx, k_normals_from_cov, pgrid, dim3(256), 0, ctx->stream, (const double *)nullptr, (const int32_t *)cnt, c.n,
                               (double *)nullptr, 2, (const int32_t *)nbr, k, (const double *)c.xyz64,
                               (const double *)((attrs & PCCM_SSIM_NORMAL) ? c.nrm64 : nullptr),
                               (const double *)((attrs & PCCM_SSIM_COLOR) ? c.rgb64 : nullptr), curv, c.ssim64, 1 << a,
                               (const double *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr);
    PCCM_HIP(hipGetLastError());
    c.ssim_k = k;
    c.ssim_attrs = attrs;
    if (built) *built = 1;
    return PCCM_OK;
}

// Point-to-distribution: the k nearest points of the OTHER cloud for every point of cloud `dir` (direction dir: cloud dir's points
// are the queries), as neighbour lists nbr[n][k] / cnt[n] in ctx->ssim_scratch / ctx->val.  The grid is the one knn_setup picks for
// the searched cloud; the chain wave -> per-thread -> full scan is the same-cloud searches', and so is the exactness.
static int p2d_search(pccm_ctx *ctx, int dir, int k, int32_t **nbr_out, int32_t **cnt_out)
{
    const Cloud &a = ctx->cloud[dir], &b = ctx->cloud[1 - dir];
    int rc;
    KnnGeom g;
    const uint32_t *cs;
    const GridRec *crecs, *qrecs;
    if ((rc = knn_setup(ctx, 1 - dir, g, cs, crecs, &qrecs))) return rc;
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    double *cov;
    int32_t *cnt;
    uint32_t *open_count, *todo_count;
    if ((rc = knn_scratch(ctx, a.n, &cov, &cnt, &open_count, &todo_count))) return rc;
    if ((rc = ensure(ctx, ctx->ssim_scratch, (size_t)a.n * k * sizeof(int32_t)))) return rc;
    int32_t *nbr = (int32_t *)ctx->ssim_scratch.p;
    launch_knn_lists(ctx, crecs, cs, g, b.xyz64, b.n, qrecs, a.xyz64, a.xyz64, a.n, k, cov, cnt, open_count, todo_count, nbr);
    PCCM_HIP(hipGetLastError());
    *nbr_out = nbr;
    *cnt_out = cnt;
    return PCCM_OK;
}

// pccm_p2d_build_attrs has checked k, attrs, the clouds (and their colours) and the context's state.  One k-NN search per
// direction serves every column that is missing: the geometry column (mode 3) and, with PCCM_P2D_COLOR, the colour and joint columns
// (mode 4, which reads the geometry column back) are formed from the same neighbour lists while they are in HBM.
int p2d_build(pccm_ctx *ctx, int k, int attrs, int *built)
{
    if (built) *built = 0;
    const bool geometry = ctx->p2d_k != k;                                  // (a new k drops the colour columns too)
    const bool color = (attrs & PCCM_P2D_COLOR) && (geometry || !ctx->p2d_color);
    if (!geometry && !color) return PCCM_OK;
    if (ctx->capturing) {
        ctx->capture_failed = true;
        return fail(PCCM_E_STATE, "point-to-distribution columns are built before graph capture");
    }
    int rc;
    if (geometry) {
        ctx->p2d_k = 0;
        ctx->p2d_color = false;
    }
    for (int d = 0; d < 2; ++d) ctx->nn_gen[d]++;       // pending point-to-distribution reductions would read stale columns
    for (int d = 0; d < 2; ++d) {
        const Cloud &a = ctx->cloud[d], &b = ctx->cloud[1 - d];
        PCCM_HIP(hipStreamSynchronize(ctx->stream));
        double **cols[3] = {&ctx->p2d64[d], &ctx->p2d_cj64[d][0], &ctx->p2d_cj64[d][1]};
        size_t *caps[3] = {&ctx->cap_p2d[d], &ctx->cap_p2d_cj[d][0], &ctx->cap_p2d_cj[d][1]};
        for (int c = 0; c < 3; ++c) {
            if (!(c == 0 ? geometry : color)) continue;
            const double *before = *cols[c];
            if ((rc = grow((void **)cols[c], *caps[c], (size_t)a.n * sizeof(double)))) return rc;
            if (*cols[c] != before) ctx->epoch++;           // (graphs that read the old column are stale)
        }
        int32_t *nbr, *cnt;
        if ((rc = p2d_search(ctx, d, k, &nbr, &cnt))) return rc;
        const dim3 pgrid((unsigned)((a.n + 255) / 256));
        if (geometry)
            PCCM_LAUNCH(ctx, k_normals_from_cov, pgrid, dim3(256), 0, ctx->stream, (const double *)nullptr,
                               (const int32_t *)cnt, a.n, ctx->p2d64[d], 3, (const int32_t *)nbr, k, (const double *)b.xyz64,
                               (const double *)nullptr, (const double *)nullptr, (double *)nullptr, (double *)nullptr, 0,
                               (const double *)a.xyz64, (const uint32_t *)nullptr, (const uint32_t *)nullptr);
        if (color)
            PCCM_LAUNCH(ctx, k_normals_from_cov, pgrid, dim3(256), 0, ctx->stream, (const double *)ctx->p2d64[d],
                               (const int32_t *)cnt, a.n, ctx->p2d_cj64[d][0], 4, (const int32_t *)nbr, k, (const double *)nullptr,
                               (const double *)nullptr, (const double *)b.rgb64, ctx->p2d_cj64[d][1], (double *)nullptr, 0,
                               (const double *)a.rgb64, (const uint32_t *)(b.rgb8_valid ? b.rgb8 : nullptr),
                               (const uint32_t *)(a.rgb8_valid ? a.rgb8 : nullptr));
        PCCM_HIP(hipGetLastError());
    }
    ctx->p2d_k = k;
    if (color) ctx->p2d_color = true;
    if (built) *built = 1;
    return PCCM_OK;
}

// the neighbour lists of direction dir, in HBM until the next k-NN search (a search of its own: the build keeps no lists)
int p2d_neighbours(pccm_ctx *ctx, int dir, int k, const int32_t **nbr_out, const int32_t **cnt_out)
{
    const Cloud &a = ctx->cloud[dir];
    int rc;
    if ((rc = ensure(ctx, ctx->ssim_scratch, (size_t)a.n * k * sizeof(int32_t)))) return rc;
    PCCM_HIP(hipMemsetAsync(ctx->ssim_scratch.p, 0xff, (size_t)a.n * k * sizeof(int32_t), ctx->stream));   // unused entries: -1
    int32_t *nbr, *cnt;
    if ((rc = p2d_search(ctx, dir, k, &nbr, &cnt))) return rc;
    *nbr_out = nbr;
    *cnt_out = cnt;
    return PCCM_OK;
}

}  // namespace pccm
