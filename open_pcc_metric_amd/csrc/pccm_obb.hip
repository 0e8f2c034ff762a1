// Minimal oriented bounding box: the search over hull-face frames on the device.
//
// Stands under CloudPair.get_extent(), open_pcc_metric/cloud_pair.py:111-112
// (get_minimal_oriented_bounding_box().extent; Open3D 0.18: Qhull convex hull, then for every hull triangle
// the axis-aligned box of the hull vertices in the triangle's frame -- x along its first edge, z along its
// normal -- keeping the smallest volume).  The hull itself is Qhull on the host (as in Open3D); what is left
// is H hull vertices x T hull triangles of projections, which is seconds of NumPy for a rounded shape
// (H ~ 5e4, T ~ 1e5) and milliseconds here.  fp64 throughout.  Not parity-pinned (Open3D is not in the
// reference checkout); the three kernels of this file are held, per tile, workgroup and edge, to the exact references of
// tests/extent_reference.py (tests/test_gpu_extent_kernels.py; DESIGN.md, "Minimal OBB").
//
// k_obb_frames: one thread per triangle, the hull vertices streamed through LDS in tiles (every tile is read
// once per workgroup and broadcast to its 256 frames).  18 fp64 operations per (vertex, triangle) pair.
#include "pccm_internal.h"

namespace pccm {

constexpr int kObbTile = 1024;      // hull vertices per LDS tile (24 KB)

__global__ __launch_bounds__(256) void k_obb_frames(const double *__restrict__ verts, int64_t nv, const double *__restrict__ tri,
                                                    int64_t nt, double *__restrict__ ext_out /*[nt][3]*/, double *__restrict__ vol_out)
{
    __shared__ double s_v[kObbTile * 3];
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = t < nt;
    double a[3] = {0, 0, 0}, f[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (live) {
        const double *p = tri + 9 * t;
        double u[3], v[3], w[3];
        for (int k = 0; k < 3; ++k) { a[k] = p[k]; u[k] = p[3 + k] - p[k]; v[k] = p[6 + k] - p[k]; }
        w[0] = u[1] * v[2] - u[2] * v[1]; w[1] = u[2] * v[0] - u[0] * v[2]; w[2] = u[0] * v[1] - u[1] * v[0];
        v[0] = w[1] * u[2] - w[2] * u[1]; v[1] = w[2] * u[0] - w[0] * u[2]; v[2] = w[0] * u[1] - w[1] * u[0];
        const double *row[3] = {u, v, w};
        for (int r = 0; r < 3; ++r) {
            const double l = sqrt(row[r][0] * row[r][0] + row[r][1] * row[r][1] + row[r][2] * row[r][2]);
            for (int k = 0; k < 3; ++k) f[r][k] = row[r][k] / l;       // a degenerate triangle gives NaN: its volume is discarded
        }
    }
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t base = 0; base < nv; base += kObbTile) {
        const int64_t m = nv - base < kObbTile ? nv - base : kObbTile;
        __syncthreads();
        for (int64_t i = threadIdx.x; i < 3 * m; i += 256) s_v[i] = verts[3 * base + i];
        __syncthreads();
        for (int64_t j = 0; j < m; ++j) {
            const double dx = s_v[3 * j] - a[0], dy = s_v[3 * j + 1] - a[1], dz = s_v[3 * j + 2] - a[2];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double l = f[r][0] * dx + f[r][1] * dy + f[r][2] * dz;
                lo[r] = fmin(lo[r], l);        // fmin/fmax drop a NaN operand: a NaN frame leaves +-inf, hence an infinite volume
                hi[r] = fmax(hi[r], l);
            }
        }
    }
    if (live) {
        double e[3], vol = 1.0;
        bool ok = true;
        for (int r = 0; r < 3; ++r) {
            e[r] = hi[r] - lo[r];
            ok = ok && e[r] >= 0.0 && e[r] < INFINITY;      // a NaN row saw no vertex: hi - lo = -inf
            ext_out[3 * t + r] = e[r];
            vol *= e[r];
        }
        vol_out[t] = (ok && vol < INFINITY) ? vol : INFINITY;
    }
}

int launch_obb_frames(pccm_ctx *ctx, const double *verts, int64_t nv, const double *tri, int64_t nt, double *ext_out, double *vol_out)
{
    ProfScope ps(ctx, PCCM_K_POINT);
    PCCM_LAUNCH(ctx, k_obb_frames, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, ctx->stream, verts, nv, tri, nt, ext_out, vol_out);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

}  // namespace pccm

// ---- thinning the cloud before Qhull -----------------------------------------------------------------------
// Qhull's time goes into the N input points, almost all of which lie deep inside the hull.  Two kernels let the
// host hand it only points that can still be hull vertices -- exactly, not approximately:
//   k_extreme_rows    for K directions the row of (about) the farthest point: these K points span an inner polytope;
//   k_outside_planes  the rows of all points that are not strictly inside that polytope (its facets come back from
//                     a tiny Qhull run on the K points).  A point strictly inside the hull of other points of the
//                     cloud is not a vertex of the cloud's hull, so dropping it does not change the hull.
// Which K points are picked does not matter for correctness (any subset of the cloud gives a valid inner polytope),
// so the extremes are chosen in fp32.
namespace pccm {

constexpr int kMaxDirs = 1024;

// Lanes own directions (16 each: 1024 per wave), waves own slices of the cloud: a point's coordinates are the same for
// every lane (one broadcast load), so the running maxima stay in registers and nothing is reduced across lanes; a wave
// meets the other waves only at the end, with one conditional atomicMax per direction.
constexpr int kDirsPerLane = kMaxDirs / 64;

__global__ __launch_bounds__(256) void k_extreme_rows(const double *__restrict__ x64, int64_t n, const float *__restrict__ dirs, int ndirs,
                                                      unsigned long long *__restrict__ best /*[ndirs]: (ordered dot << 32) | row*/)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (int64_t)gridDim.x * 4;
    float dx[kDirsPerLane], dy[kDirsPerLane], dz[kDirsPerLane];
    unsigned long long mine[kDirsPerLane];
#pragma unroll
    for (int j = 0; j < kDirsPerLane; ++j) {
        const int k = lane + 64 * j;
        dx[j] = k < ndirs ? dirs[3 * k] : 0.f;
        dy[j] = k < ndirs ? dirs[3 * k + 1] : 0.f;
        dz[j] = k < ndirs ? dirs[3 * k + 2] : 0.f;
        mine[j] = 0ull;
    }
    const int64_t per = (n + nwaves - 1) / nwaves;
    const int64_t i0 = wave * per, i1 = (i0 + per < n) ? i0 + per : n;
    for (int64_t i = i0; i < i1; ++i) {                                            // wave-uniform: broadcast loads
        const float x = (float)x64[3 * i], y = (float)x64[3 * i + 1], z = (float)x64[3 * i + 2];
#pragma unroll
        for (int j = 0; j < kDirsPerLane; ++j) {
            const float d = dx[j] * x + dy[j] * y + dz[j] * z;
            uint32_t b = __float_as_uint(d);
            b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);                          // order-preserving key
            const unsigned long long key = ((unsigned long long)b << 32) | (unsigned long long)(uint32_t)i;
            mine[j] = key > mine[j] ? key : mine[j];
        }
    }
#pragma unroll
    for (int j = 0; j < kDirsPerLane; ++j) {
        const int k = lane + 64 * j;
        if (k < ndirs && mine[j] > __hip_atomic_load(&best[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&best[k], mine[j]);
    }
}

__global__ __launch_bounds__(256) void k_outside_planes(const double *__restrict__ x64, int64_t n, const double *__restrict__ planes,
                                                        int nplanes, double margin, int32_t *__restrict__ rows_out,
                                                        unsigned int *__restrict__ count)
{
    __shared__ double s_pl[512 * 4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    const double x = live ? x64[3 * i] : 0.0, y = live ? x64[3 * i + 1] : 0.0, z = live ? x64[3 * i + 2] : 0.0;
    bool outside = false;
    for (int base = 0; base < nplanes; base += 512) {
        const int m = nplanes - base < 512 ? nplanes - base : 512;
        __syncthreads();
        for (int k = threadIdx.x; k < 4 * m; k += 256) s_pl[k] = planes[4 * base + k];
        __syncthreads();
        if (!outside)
            for (int k = 0; k < m; ++k)
                if (s_pl[4 * k] * x + s_pl[4 * k + 1] * y + s_pl[4 * k + 2] * z + s_pl[4 * k + 3] > -margin) {   // Qhull: n.x + off <= 0 inside
                    outside = true;
                    break;
                }
    }
    if (live && outside) rows_out[atomicAdd(count, 1u)] = (int32_t)i;
}

int launch_extreme_rows(pccm_ctx *ctx, const double *x64, int64_t n, const float *dirs, int ndirs, unsigned long long *best)
{
    ProfScope ps(ctx, PCCM_K_POINT);
    const int64_t blocks = (n + 255) / 256;
    PCCM_LAUNCH(ctx, k_extreme_rows, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, ctx->stream, x64, n, dirs, ndirs, best);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

int launch_outside_planes(pccm_ctx *ctx, const double *x64, int64_t n, const double *planes, int nplanes, double margin,
                          int32_t *rows_out, unsigned int *count)
{
    ProfScope ps(ctx, PCCM_K_POINT);
    PCCM_LAUNCH(ctx, k_outside_planes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, x64, n, planes, nplanes, margin,
                       rows_out, count);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

}  // namespace pccm
