// Per-thread ring search for VOXELISED content on gfx950: both clouds integer-valued (every PCC test sequence: 8i,
// Owlii, MVUB -- BASELINE.json configs[4]), surfaces rather than volumes, exact distance ties the rule.
//
// Stands under get_neighbour_cloud(), open_pcc_metric/cloud_pair.py:10-42, like every other search kernel here; it
// replaces k_grid_query<Rec32> (pccm_grid.hip: fp64 evaluation of every candidate, window after window) for pairs where
//   * fp32 arithmetic is EXACT: coordinates are integers below 2^22, a candidate within kMaxRing cells differs by less than
//     2^11 per axis (the host checks the cell edge), so dx, dx*dx and the sum of three squares are integers below 2^24 --
//     the fp32 value IS the reference's fp64 ((dx*dx)+(dy*dy))+(dz*dz); no certification, no second look;
//   * ties are decided in the same breath: (d2 bits, row) packed into one 64-bit key, smallest key wins = smallest row among
//     the nearest (the library's rule, include/pccm.h);
//   * most cells are empty (a surface fills ~6 % of its grid): the searched cloud's OCCUPANCY BITMAP (one bit per cell, written
//     by k_bin_sort next to the cell starts; 1.7 MB at 13 M cells: L2-resident) is asked first, and cell starts / records are
//     fetched only for windows that hold something -- a third of ring 1 on a surface;
//   * every dependent step of ring 1 is issued for all nine x-runs at once -- bitmap words, then the cell starts of the windows
//     that hold something, then the candidates eight at a time out of the concatenation of the windows: six memory round trips
//     per query where window-by-window took fifteen.
// Bound: memory latency of dependent gathers (bitmap word -> cell starts -> records), hidden by occupancy and batching.
// Measured and dropped (round 3): a sparse cell index instead of the dense cell starts (occupancy words with ranks + starts of
// the occupied cells only: 7 MB where the dense arrays take 108) -- its build is not write-bound but bound by the per-cell LDS
// work of the counting sort, which stays (build 92 us against 75, search 171 against 159 on the 0.8M surrogate).
#include "pccm_grid.h"

namespace pccm {

__device__ __forceinline__ unsigned long long lat_key(float d, int row)
{
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned int)row;      // d >= 0: float order == bit order
}

// cells [c0, c1] (inclusive, c1 - c0 < 32) of a bitmap: any bit set?
__device__ __forceinline__ bool any_occupied(const uint32_t *__restrict__ occ, uint32_t c0, uint32_t c1)
{
    const uint32_t w0 = c0 >> 5, w1 = c1 >> 5;
    const uint32_t lo = occ[w0] >> (c0 & 31u);
    if (w0 == w1) return (lo & (0xffffffffu >> (31u - (c1 - c0)))) != 0u;
    return lo != 0u || (occ[w1] & (0xffffffffu >> (31u - (c1 & 31u)))) != 0u;
}

template <bool SELF>
__device__ __forceinline__ void lat_scan(const float4 *__restrict__ recs, uint32_t s, uint32_t e, float qx, float qy, float qz, int qrow,
                                         unsigned long long &best)
{
    for (uint32_t p = s; p < e; p += 4u) {
        float4 a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = recs[(p + j < e) ? p + j : e - 1u];     // (re-evaluating a record is harmless: min is idempotent)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float dx = qx - a[j].x, dy = qy - a[j].y, dz = qz - a[j].z;
            const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));   // exact: integers below 2^24
            unsigned long long k = lat_key(d, __float_as_int(a[j].w));
            if (SELF) k = (__float_as_int(a[j].w) == qrow) ? ~0ull : k;
            best = k < best ? k : best;
        }
    }
}

constexpr int kLatBatch = 8;     // candidates in flight per lane (95 VGPRs: five waves per SIMD; 4 at eight waves and 12 at four
                                 // waves measured 191 and 170 us against 159)

template <bool SELF>
__global__ __launch_bounds__(256, 5) void k_lattice_query(QueryJobs jobs, GridGeom g)
{
    const int dimx = g.dim[0], dimy = g.dim[1], dimz = g.dim[2];
    for (int jb = 0; jb < jobs.njobs; ++jb) {
        const QueryJob &J = jobs.j[jb];
        const float4 *__restrict__ qrecs = reinterpret_cast<const float4 *>(J.qrecs);
        const float4 *__restrict__ srecs = reinterpret_cast<const float4 *>(J.srecs);
        const uint32_t *__restrict__ cs = J.cs;
        const uint32_t *__restrict__ occ = J.occ;
        const int64_t nq = J.nq;
        for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < nq; t += (int64_t)gridDim.x * 256) {
            const float4 q = qrecs[t];
            const int qrow = __float_as_int(q.w);
            const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
            const int cx = cell_coord(qx, g.org[0], g.inv_h[0], dimx);
            const int cy = cell_coord(qy, g.org[1], g.inv_h[1], dimy);
            const int cz = cell_coord(qz, g.org[2], g.inv_h[2], dimz);
            unsigned long long best = ~0ull;
            bool done = false;
            {
                // ---- ring 1, batched ------------------------------------------------------------------------------------
                const int x0 = max(cx - 1, 0), x1 = min(cx + 1, dimx - 1);
                uint32_t wlo[9], whi[9], rowv[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const int z = cz + k / 3 - 1, y = cy + k % 3 - 1;
                    const bool in = z >= 0 && z < dimz && y >= 0 && y < dimy;
                    rowv[k] = in ? ((uint32_t)z * dimy + y) * dimx : 0xffffffffu;
                    const uint32_t c0 = in ? rowv[k] + x0 : 0u, c1 = in ? rowv[k] + x1 : 0u;
                    wlo[k] = occ[c0 >> 5];
                    whi[k] = occ[c1 >> 5];
                }
                uint32_t ws[9], we[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const uint32_t c0 = rowv[k] + x0, c1 = rowv[k] + x1;
                    const uint32_t lo = wlo[k] >> (c0 & 31u);
                    const bool same = (c0 >> 5) == (c1 >> 5);
                    const bool any = rowv[k] != 0xffffffffu &&
                                     (same ? (lo & (0xffffffffu >> (31u - (c1 - c0)))) != 0u
                                           : (lo != 0u || (whi[k] & (0xffffffffu >> (31u - (c1 & 31u)))) != 0u));
                    ws[k] = 0u;
                    we[k] = 0u;
                    if (any) {
                        ws[k] = cs[c0];
                        we[k] = cs[c1 + 1u];
                    }
                }
                // place of every window in the concatenation of the nine
                uint32_t pre[10];
                pre[0] = 0u;
#pragma unroll
                for (int k = 0; k < 9; ++k) pre[k + 1] = pre[k] + (we[k] - ws[k]);
                const uint32_t T = pre[9];
                for (uint32_t i0 = 0; i0 < T; i0 += (uint32_t)kLatBatch) {
                    float4 a[kLatBatch];
#pragma unroll
                    for (int u = 0; u < kLatBatch; ++u) {
                        const uint32_t i = (i0 + u < T) ? i0 + u : T - 1u;       // (re-evaluating a record is harmless: min is idempotent)
                        uint32_t delta = ws[0];
#pragma unroll
                        for (int k = 1; k < 9; ++k) delta = (i >= pre[k]) ? ws[k] - pre[k] : delta;
                        a[u] = srecs[i + delta];
                    }
#pragma unroll
                    for (int u = 0; u < kLatBatch; ++u) {
                        const float dx = q.x - a[u].x, dy = q.y - a[u].y, dz = q.z - a[u].z;
                        const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));   // exact: integers below 2^24
                        unsigned long long kk = lat_key(d, __float_as_int(a[u].w));
                        if (SELF) kk = (__float_as_int(a[u].w) == qrow) ? ~0ull : kk;
                        best = kk < best ? kk : best;
                    }
                }
                const double bd1 = best == ~0ull ? INFINITY : (double)__uint_as_float((uint32_t)(best >> 32));
                done = settled_by(face_bound(g, qx, qy, qz, cx, cy, cz, 1), bd1);
            }
            for (int r = 2; r <= kMaxRing && !done; ++r) {           // (a few per cent of the queries get here)
                const int z0 = max(cz - r, 0), z1 = min(cz + r, dimz - 1);
                const int y0 = max(cy - r, 0), y1 = min(cy + r, dimy - 1);
                const int x0 = max(cx - r, 0), x1 = min(cx + r, dimx - 1);
                for (int z = z0; z <= z1; ++z) {
                    const bool zface = z == cz - r || z == cz + r;
                    for (int y = y0; y <= y1; ++y) {
                        const uint32_t row = ((uint32_t)z * dimy + y) * dimx;
                        if (zface || y == cy - r || y == cy + r) {          // the shell's faces whole
                            if (any_occupied(occ, row + x0, row + x1))
                                lat_scan<SELF>(srecs, cs[row + x0], cs[row + x1 + 1], q.x, q.y, q.z, qrow, best);
                        } else {                                             // interior of the shell: only the two end cells
                            if (cx - r >= 0 && any_occupied(occ, row + cx - r, row + cx - r))
                                lat_scan<SELF>(srecs, cs[row + cx - r], cs[row + cx - r + 1], q.x, q.y, q.z, qrow, best);
                            if (cx + r <= dimx - 1 && any_occupied(occ, row + cx + r, row + cx + r))
                                lat_scan<SELF>(srecs, cs[row + cx + r], cs[row + cx + r + 1], q.x, q.y, q.z, qrow, best);
                        }
                    }
                }
                const double bd = best == ~0ull ? INFINITY : (double)__uint_as_float((uint32_t)(best >> 32));
                done = settled_by(face_bound(g, qx, qy, qz, cx, cy, cz, r), bd);
            }
            const double bd = best == ~0ull ? INFINITY : (double)__uint_as_float((uint32_t)(best >> 32));
            if (done) {
                int idx = (int)(uint32_t)best;
                double d2 = bd;
                if (best == ~0ull) { idx = -1; d2 = 0.0; }      // SELF on a one-point cloud (the host handles it earlier)
                emit_result_lookup(J.out, J.s64, qrow, qx, qy, qz, idx, d2);
            } else {
                // still open after kMaxRing rings: exact rescan of the whole cloud (k2b_fallback), as thread_search does
                const double tq = (bd == INFINITY) ? 1.0e18 : sqrt(bd) * (1.0 + 0x1.0p-20) + J.slack32;
                const double thr = tq * tq * (1.0 + 0x1.0p-30) + 1.0e-36;
                float tf = thr > 3.0e38 ? 3.0e38f : (float)thr;
                tf = __uint_as_float(__float_as_uint(tf) + 1u);
                const uint32_t pos = atomicAdd(&J.counters[0], 1u);
                J.flagged[pos] = qrow - (int)J.row_base;
                J.flag_thr[pos] = tf;
            }
        }
    }
}

int launch_lattice_query(pccm_ctx *ctx, const QueryJobs &jobs, const GridGeom &g, bool self)
{
    int64_t nqmax = 0;
    for (int k = 0; k < jobs.njobs; ++k) nqmax = jobs.j[k].nq > nqmax ? jobs.j[k].nq : nqmax;
    dim3 grid((unsigned)((nqmax + 255) / 256));
    if (self) PCCM_LAUNCH(ctx, (k_lattice_query<true>), grid, dim3(256), 0, ctx->stream, jobs, g);
    else PCCM_LAUNCH(ctx, (k_lattice_query<false>), grid, dim3(256), 0, ctx->stream, jobs, g);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

}  // namespace pccm
