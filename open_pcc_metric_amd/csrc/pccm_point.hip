// Ingest, the per-point column kernel (K3) and the NumPy-ordered leaf reduction (K5).
#include "pccm_internal.h"
#include "pccm_reduce_shape.h"
#include "pccm_tail_wave.h"

namespace pccm {

// ------------------------------------------------------------------------------------------
// Ingest: packed [n][3] f32/f64 rows -> float4 scan copy (padded) + fp64 copy, and three
// statistics: [0] max |coordinate| (as fp64 bits; non-negative doubles order like uint64), [1] number
// of coordinates that do not survive fp64 -> fp32 -> fp64, [2] number of non-finite coordinates,
// [3..5] / [6..8] order keys of the bounding box minimum / maximum per axis (for the grid engine),
// [9] number of coordinates that are not integers (voxelised content has none).
// ------------------------------------------------------------------------------------------
// monotonic map double -> uint64 (so that atomicMin/atomicMax order like the doubles do)
__device__ __forceinline__ unsigned long long order_key(double v)
{
    unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

template <typename T>
__global__ __launch_bounds__(256) void k_ingest_points(const T *__restrict__ src, int64_t n, int64_t n_pad,
                                                       float *__restrict__ x32, double *__restrict__ x64, float4 *__restrict__ x32r,
                                                       unsigned long long *__restrict__ stats, const IngestMove mv)
{
    __shared__ unsigned long long s_mx[4], s_lo[4][3], s_hi[4][3];
    __shared__ int s_cnt[4][3];
    unsigned long long mx = 0;
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};   // bounding box keys
    int inexact = 0, bad = 0, frac = 0;
    // grid-stride: one workgroup per CU, so that the ten statistics cost a few hundred atomics on the same ten
    // addresses (same-address atomics and the loads that peek at them serialise: 2048 workgroups took 111 us for a
    // million points, 256 take 38) instead of one set per wave
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_pad; i += (int64_t)gridDim.x * 256) {
        if (i < n) {
            double v[3];
            float f[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) v[a] = (double)src[3 * i + a];
            if (mv.on) {                                   // (a kernel argument: an ingest that moves nothing pays one scalar branch per row)
                const double x = v[0], y = v[1], z = v[2];
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    v[a] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(mv.m[4 * a], x), __dmul_rn(mv.m[4 * a + 1], y)), __dmul_rn(mv.m[4 * a + 2], z)),
                                     mv.m[4 * a + 3]);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                f[a] = (float)v[a];
                inexact += ((double)f[a] != v[a]) ? 1 : 0;
                frac += (floor(v[a]) != v[a]) ? 1 : 0;
                bad += isfinite(v[a]) ? 0 : 1;
                unsigned long long b = (unsigned long long)__double_as_longlong(fabs(v[a]));
                mx = b > mx ? b : mx;
                x64[3 * i + a] = v[a];
                const unsigned long long key = order_key(v[a]);
                lo[a] = key < lo[a] ? key : lo[a];
                hi[a] = key > hi[a] ? key : hi[a];
            }
            float *qd = x32 + (i >> 2) * 12 + (i & 3);
            qd[0] = f[0];
            qd[4] = f[1];
            qd[8] = f[2];
            x32r[i] = make_float4(f[0], f[1], f[2], 0.f);
        } else {
            float *qd = x32 + (i >> 2) * 12 + (i & 3);
            qd[0] = qd[4] = qd[8] = kPadCoord;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx;
        inexact += __shfl_xor(inexact, off);
        bad += __shfl_xor(bad, off);
        frac += __shfl_xor(frac, off);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            unsigned long long l = __shfl_xor(lo[a], off), h = __shfl_xor(hi[a], off);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_mx[w] = mx;
        s_cnt[w][0] = inexact; s_cnt[w][1] = bad; s_cnt[w][2] = frac;
        for (int a = 0; a < 3; ++a) { s_lo[w][a] = lo[a]; s_hi[w][a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            mx = s_mx[k] > mx ? s_mx[k] : mx;
            inexact += s_cnt[k][0]; bad += s_cnt[k][1]; frac += s_cnt[k][2];
            for (int a = 0; a < 3; ++a) {
                lo[a] = s_lo[k][a] < lo[a] ? s_lo[k][a] : lo[a];
                hi[a] = s_hi[k][a] > hi[a] ? s_hi[k][a] : hi[a];
            }
        }
        // the host reads stats[1], [2] and [9] as flags and the rest as extrema, so an atomic is only issued when it
        // would change the word: after the first few workgroups almost none are (same-address atomics serialise)
        auto peek = [&](int k) { return __hip_atomic_load(&stats[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
        if (mx > peek(0)) atomicMax(&stats[0], mx);
        if (inexact && !peek(1)) atomicAdd(&stats[1], (unsigned long long)inexact);
        if (bad && !peek(2)) atomicAdd(&stats[2], (unsigned long long)bad);
        if (frac && !peek(9)) atomicAdd(&stats[9], (unsigned long long)frac);
        for (int a = 0; a < 3; ++a) {
            if (lo[a] < peek(3 + a)) atomicMin(&stats[3 + a], lo[a]);
            if (hi[a] > peek(6 + a)) atomicMax(&stats[6 + a], hi[a]);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_ingest_normals(const T *__restrict__ src, int64_t n3,
                                                        double *__restrict__ out, float *__restrict__ out32,
                                                        unsigned long long *__restrict__ stats, const IngestMove mv)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int bad = 0, inexact = 0;
    if (i < n3) {
        double v;
        if (mv.on) {                                       // component a of A n for the row this component belongs to
            const int64_t r = i / 3;
            const int a = (int)(i - 3 * r);
            const double nx = (double)src[3 * r], ny = (double)src[3 * r + 1], nz = (double)src[3 * r + 2];
            const double m0 = a == 0 ? mv.m[0] : (a == 1 ? mv.m[4] : mv.m[8]);
            const double m1 = a == 0 ? mv.m[1] : (a == 1 ? mv.m[5] : mv.m[9]);
            const double m2 = a == 0 ? mv.m[2] : (a == 1 ? mv.m[6] : mv.m[10]);
            v = __dadd_rn(__dadd_rn(__dmul_rn(m0, nx), __dmul_rn(m1, ny)), __dmul_rn(m2, nz));
        } else {
            v = (double)src[i];
        }
        out[i] = v;
        const float f = (float)v;
        if (out32) out32[(i / 3) * 4 + (i % 3)] = f;      // stats[1] says whether this copy may stand for `out`
        bad = isfinite(v) ? 0 : 1;
        inexact = ((double)f == v) ? 0 : 1;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicAdd(&stats[2], 1ull);
    if (__ballot(inexact) && (threadIdx.x & 63) == 0) atomicAdd(&stats[1], 1ull);
}

int launch_ingest_points(pccm_ctx *ctx, const void *src, int dtype, int64_t n, int64_t n_pad, float4 *x32,
                         double *x64, float4 *x32r, unsigned long long *stats, const IngestMove *move)
{
    const IngestMove mv = move ? *move : IngestMove();
    ProfScope ps(ctx, PCCM_K_INGEST);
    const int64_t blocks = (n_pad + 255) / 256;
    dim3 grid((unsigned)(blocks < 256 ? blocks : 256));
    if (dtype == PCCM_F32)
        PCCM_LAUNCH(ctx, (k_ingest_points<float>), grid, dim3(256), 0, ctx->stream, (const float *)src, n, n_pad, (float *)x32, x64, x32r, stats, mv);
    else
        PCCM_LAUNCH(ctx, (k_ingest_points<double>), grid, dim3(256), 0, ctx->stream, (const double *)src, n, n_pad, (float *)x32, x64, x32r, stats, mv);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

int launch_ingest_normals(pccm_ctx *ctx, const void *src, int dtype, int64_t n, double *out, float *out32, unsigned long long *stats,
                          const IngestMove *move)
{
    const IngestMove mv = move ? *move : IngestMove();
    ProfScope ps(ctx, PCCM_K_INGEST);
    const int64_t n3 = 3 * n;
    dim3 grid((unsigned)((n3 + 255) / 256));
    if (dtype == PCCM_F32)
        PCCM_LAUNCH(ctx, (k_ingest_normals<float>), grid, dim3(256), 0, ctx->stream, (const float *)src, n3, out, out32, stats, mv);
    else
        PCCM_LAUNCH(ctx, (k_ingest_normals<double>), grid, dim3(256), 0, ctx->stream, (const double *)src, n3, out, out32, stats, mv);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

// Reflectance: [n] scalars of f32 or f64 -> the fp64 column, values as given.  The widening copy of the normals' ingest over n
// values instead of 3 n (no fp32 copy): stats[2] counts the waves that met a non-finite value.
int launch_ingest_reflectance(pccm_ctx *ctx, const void *src, int dtype, int64_t n, double *out, unsigned long long *stats)
{
    ProfScope ps(ctx, PCCM_K_INGEST);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (dtype == PCCM_F32)
        PCCM_LAUNCH(ctx, (k_ingest_normals<float>), grid, block, 0, ctx->stream, (const float *)src, n, out, (float *)nullptr, stats, IngestMove());
    else
        PCCM_LAUNCH(ctx, (k_ingest_normals<double>), grid, block, 0, ctx->stream, (const double *)src, n, out, (float *)nullptr, stats, IngestMove());
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

// ------------------------------------------------------------------------------------------
// K3 (k_point_jobs): every per-point column that is formed from a search result -- the reductions' and selections' batches
// (up to four columns per launch) and the getters (pccm_point_metric, pccm_error_vectors: one job) alike.
// point_row is one row of one job: gather the matched point, error vector e = iter[i] - search[nn(i)] (cloud_pair.py:90-100),
// projection on the other cloud's normal (metric.py:146-153) and its square (metric.py:179).
// The dot product is the FMA chain fma(e2,n2, fma(e1,n1, e0*n0)) that np.dot (OpenBLAS ddot)
// evaluates on FMA-capable hosts; see oracle/pccm_oracle.c for how that was pinned.
// HBM/gather bound: 24 (q) + 4 (idx) + 24 (r, gathered) + 24 (normal) + 8 (out) bytes per row.
// PCCM_METRIC_D1: the error vector itself, val as [ns][3] rows (pccm_error_vectors; the D1 column needs no point pass).
// PCCM_METRIC_ANGULAR (the pick's column): the own normal inrm[gi] against the matched row's nrm[j] -- 24 + 4 (or 16) + 24 + 8 bytes.
// PCCM_METRIC_SSIM_*: inrm / nrm are the two clouds' feature columns, the own feature against the matched row's -- 8 + 4 (or 16) + 8 + 8.
// PCCM_METRIC_REFLECTANCE: inrm / nrm are the two clouds' reflectance columns, the same traffic.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void point_row(const PointJob &J, int64_t i)
{
    const int64_t gi = J.q_begin + i;
    if (J.metric == PCCM_METRIC_ANGULAR) {
        const int64_t j = J.recs ? (int64_t)__float_as_int(J.recs[i].w) : (int64_t)J.idx[i];
        J.val[i] = angular_similarity(J.inrm + 3 * gi, J.nrm + 3 * j);
        return;
    }
    if (is_ssim_metric(J.metric)) {
        const int64_t j = J.recs ? (int64_t)__float_as_int(J.recs[i].w) : (int64_t)J.idx[i];
        J.val[i] = ssim_similarity(J.inrm[gi], J.nrm[j]);
        return;
    }
    if (J.metric == PCCM_METRIC_REFLECTANCE) {
        const int64_t j = J.recs ? (int64_t)__float_as_int(J.recs[i].w) : (int64_t)J.idx[i];
        J.val[i] = reflectance_error(J.inrm[gi], J.nrm[j]);
        return;
    }
    const int64_t j = J.idx[i];
    const double *r = J.c64 ? J.c64 + 3 * i : J.r64 + 3 * j;     // PCCM_TIES_MEAN: the virtual neighbour of row i
    const double ex = __dsub_rn(J.q64[3 * gi], r[0]);
    const double ey = __dsub_rn(J.q64[3 * gi + 1], r[1]);
    const double ez = __dsub_rn(J.q64[3 * gi + 2], r[2]);
    if (J.metric == PCCM_METRIC_D1) {
        J.val[3 * i] = ex;
        J.val[3 * i + 1] = ey;
        J.val[3 * i + 2] = ez;
        return;
    }
    const double *nv = (J.normal_mode == PCCM_NORMAL_ROW) ? J.nrm + 3 * gi : J.cn64 ? J.cn64 + 3 * i : J.nrm + 3 * j;
    double p = __dmul_rn(ex, nv[0]);
    p = __fma_rn(ey, nv[1], p);
    p = __fma_rn(ez, nv[2], p);
    J.val[i] = (J.metric == PCCM_METRIC_PROJ) ? p : __dmul_rn(p, p);
}

// ------------------------------------------------------------------------------------------
// K5 (k_unit_jobs below): per 128-row leaf, eight lanes accumulate rows k, k+8, k+16, ... in order and
// the eight accumulators are combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) -- exactly NumPy's
// pairwise-sum leaf, so that np.sum's tree can be finished bit for bit (pccm_finish_sum / pccm_reduce_total).
// ------------------------------------------------------------------------------------------
// ---- batched forms: several columns per launch, results written straight into pinned host memory ------
// A report needs up to four columns (D1/D2 x left/right).  One k_point_jobs launch evaluates all D2 (and the pick's
// PCCM_METRIC_ANGULAR) columns, one k_unit_jobs launch reduces all columns and stores the per-unit sums/min/max and the raw
// tail values directly into the slots' pinned host buffers (device-visible), so there is no copy node
// and no extra launch per column.
__global__ __launch_bounds__(256) void k_point_jobs(PointJobs jobs)
{
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i0 >= jobs.off[jobs.njobs]) return;
    int jb = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (k < jobs.njobs && i0 >= jobs.off[k]) jb = k;
    point_row(jobs.j[jb], i0 - jobs.off[jb]);
}

int launch_point_jobs(pccm_ctx *ctx, const PointJobs &jobs)
{
    const int64_t total = jobs.off[jobs.njobs];
    if (total <= 0) return PCCM_OK;
    ProfScope ps(ctx, PCCM_K_POINT);
    PCCM_LAUNCH(ctx, k_point_jobs, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, jobs);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

// One job = one per-point array and up to TWO columns reduced from it in the same pass: a plain column (stride 1),
// or fields of the grid engine's 32-byte result records (stride 4 doubles: [0] squared distance, [1] signed
// projection) -- the D1 and D2 columns of a direction then cost one read of its records, 16 of every 32 bytes used.
struct UnitView {               // the fields of a job the inner loop needs, in registers (wave-uniform)
    const double *val;
    int stride, off0, off1, sq0, sq1;
    int map0, map1;             // UnitCol::map / cap / alpha of the two columns
    double cap0, cap1;
    double alpha0, alpha1;
    const int32_t *rows;        // UnitJob::rows / cnt / cnt_rows (PCCM_MAP_DENSITY)
    const uint32_t *cnt;
    int64_t cnt_rows;
    int defer;                  // UnitJob::defer
    int64_t nrm_rows;           // UnitJob::nrm_rows
    const double *nrm64;
    const float4 *nrm32;
    const float4 *q32;
    int64_t row0;
};

// The two fields of a result record of layout 1 (the matched record {rx, ry, rz, row}, NNOut::layout) for row `row` of the
// iterating cloud: squared distance -- nanoflann's accumulation order, as every search kernel evaluates it (gdist64, pccm_grid.h)
// -- and err . normal[row] -- the FMA chain of emit_result / K3; bit for bit what the searches would have stored.
// defer 4 / 5: the normal of the MATCHED row (--normal-index neighbour; the record carries the row), a gather where 1 / 2 stream;
// nrm_rows bounds it (a row outside the searched cloud cannot be in a record the searches wrote: clamped all the same).
__device__ __forceinline__ void matched_fields(const float4 rec, const float4 *__restrict__ q32, int defer, const double *__restrict__ nrm64,
                                               const float4 *__restrict__ nrm32, int64_t row, bool want_proj, double &d2, double &proj,
                                               int64_t nrm_rows = 0)
{
    const float4 q = q32[row];
    const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
    const double ex = __dsub_rn(qx, (double)rec.x), ey = __dsub_rn(qy, (double)rec.y), ez = __dsub_rn(qz, (double)rec.z);
    d2 = __dadd_rn(__dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)), __dmul_rn(ez, ez));
    proj = 0.0;
    if (want_proj && defer != 3) {
        double n0, n1, n2;
        int64_t nr = row;
        if (defer >= 4) {
            nr = (int64_t)__float_as_int(rec.w);
            nr = nr < 0 ? 0 : (nr >= nrm_rows ? nrm_rows - 1 : nr);
        }
        if (defer == 1 || defer == 4) {
            const float4 t = nrm32[nr];
            n0 = (double)t.x; n1 = (double)t.y; n2 = (double)t.z;
        } else {
            n0 = nrm64[3 * nr]; n1 = nrm64[3 * nr + 1]; n2 = nrm64[3 * nr + 2];
        }
        proj = __dmul_rn(ex, n0);
        proj = __fma_rn(ey, n1, proj);
        proj = __fma_rn(ez, n2, proj);
    }
}

__device__ __forceinline__ UnitView unit_view(const UnitJob &J)
{
    UnitView w;
    w.val = J.val;
    w.stride = J.stride;
    w.off0 = J.c[0].off; w.off1 = J.c[1].off;
    w.sq0 = J.c[0].square; w.sq1 = J.c[1].square;
    w.map0 = J.c[0].map; w.map1 = J.c[1].map;
    w.cap0 = J.c[0].cap; w.cap1 = J.c[1].cap;
    w.alpha0 = J.c[0].alpha; w.alpha1 = J.c[1].alpha;
    w.rows = J.rows; w.cnt = J.cnt; w.cnt_rows = J.cnt_rows;
    w.defer = J.defer; w.nrm64 = J.nrm64; w.nrm32 = J.nrm32; w.q32 = J.q32; w.row0 = J.row0; w.nrm_rows = J.nrm_rows;
    return w;
}

__device__ __forceinline__ void unit_load(const UnitView &J, int64_t i, double v[2])      // the load alone (callers batch them)
{
    if (J.stride >= 2 && J.defer) {
        matched_fields(reinterpret_cast<const float4 *>(J.val)[i], J.q32, J.defer, J.nrm64, J.nrm32, J.row0 + i, true, v[0], v[1], J.nrm_rows);
    } else if (J.stride >= 2) {
        const double2 t = *reinterpret_cast<const double2 *>(&J.val[i * J.stride]);
        v[0] = t.x;
        v[1] = t.y;
    } else {
        v[0] = v[1] = J.val[i];
    }
}

// PCCM_MAP_DENSITY: the density-aware Chamfer term of s (the distance, or its square) for a row whose matched row m rows share --
// 1 - exp(-alpha s) / m, every operation but the fp64 exp correctly rounded and in this order (include/pccm.h)
__device__ __forceinline__ double unit_density(double alpha, double s, uint32_t m)
{
    const double e = exp(__dmul_rn(-alpha, s));
    return __dsub_rn(1.0, __ddiv_rn(e, (double)m));
}

// f(value) of a mapped column: the clamp is np.minimum(value, cap) for the NaN-free columns the map is defined on, the root
// the correctly rounded one (np.sqrt), the density term the one above (m: the row's match count), in this order
__device__ __forceinline__ double unit_map(int map, double cap, double alpha, double v, uint32_t m)
{
    if (map & PCCM_MAP_CLAMP) v = (v < cap) ? v : cap;
    if (map & PCCM_MAP_ROOT) v = __dsqrt_rn(v);
    if (map & PCCM_MAP_DENSITY) v = unit_density(alpha, v, m);
    return v;
}

// a density job (wave-uniform), and the match count its row i gathers: through the matched row, read where the search left it
__device__ __forceinline__ bool unit_dense(const UnitView &J) { return ((J.map0 | J.map1) & PCCM_MAP_DENSITY) != 0; }
__device__ __forceinline__ int32_t unit_row(const UnitView &J, int64_t i) { return matched_row(J.rows, J.val, J.stride, i); }
__device__ __forceinline__ uint32_t unit_count_of(const UnitView &J, int32_t row)
{
    // (a row outside the searched cloud cannot be in a result the searches wrote: clamped all the same, as matched_fields does)
    const int64_t r = row < 0 ? 0 : ((int64_t)row >= J.cnt_rows ? J.cnt_rows - 1 : (int64_t)row);
    return J.cnt[r];
}

// fields -> the job's columns (m: the row's match count, read by a density map alone)
__device__ __forceinline__ void unit_pick(const UnitView &J, double v[2], uint32_t m = 1u)
{
    if (J.stride >= 2) {
        const double x = v[0], y = v[1];
        v[0] = J.off0 ? y : x;
        v[1] = J.off1 ? y : x;
    }
    if (J.sq0) v[0] = __dmul_rn(v[0], v[0]);
    if (J.sq1) v[1] = __dmul_rn(v[1], v[1]);
    // the map mode (UnitCol::map): np.sum(f(column)) without the column.  Behind one wave-uniform branch on both columns' maps,
    // so that a job without one -- every job but pccm_reduce_map_*'s and pccm_reduce_density_*'s -- passes with a single scalar test
    // per value
    if (J.map0 | J.map1) {
        v[0] = unit_map(J.map0, J.cap0, J.alpha0, v[0], m);
        v[1] = unit_map(J.map1, J.cap1, J.alpha1, v[1], m);
    }
}


// PCCM_MAP_MOMENT (include/pccm.h; MomentCols below): the term of kind map >> 8 for row i, whose D1 value is d2 and whose matched row is `row`: the components it needs -- at most one of either
// cloud -- are read from the stored fp64 rows, taken relative to the pivot, multiplied where the kind says so, and kept or
// replaced by 0.0 by the IEEE comparison d2 <= cap.  The kind is a kernel argument: the branches are scalar.  The clouds' rows and
// the pivot are read from the job (U, kernel-argument memory) where they are used, not carried in the view: ten more scalar
// registers live across the sixteen loads of a plain leaf made the kernel spill.
__device__ __forceinline__ double unit_moment_term(const UnitView &J, const UnitJob &U, int map, double cap, double d2, int64_t i, int32_t row)
{
    const int kind = map >> 8;
    double t = d2;
    if (kind < 15) {
        const int a = kind < 3 ? kind : (kind < 6 ? -1 : (kind - 6) / 3);
        const int b = kind < 3 ? -1 : (kind < 6 ? kind - 3 : (kind - 6) % 3);
        double u = 0.0, v = 0.0;
        if (a >= 0) u = __dsub_rn(U.mom_it[3 * (J.row0 + i) + a], a == 0 ? U.pivot[0] : (a == 1 ? U.pivot[1] : U.pivot[2]));
        if (b >= 0) {
            // (a row outside the searched cloud cannot be in a result the searches wrote: clamped all the same)
            const int64_t r = row < 0 ? 0 : ((int64_t)row >= J.cnt_rows ? J.cnt_rows - 1 : (int64_t)row);
            v = __dsub_rn(U.mom_se[3 * r + b], b == 0 ? U.pivot[0] : (b == 1 ? U.pivot[1] : U.pivot[2]));
        }
        t = a < 0 ? v : (b < 0 ? u : __dmul_rn(u, v));
    }
    return d2 <= cap ? t : 0.0;
}
__device__ __forceinline__ void unit_moment_pick(const UnitView &J, const UnitJob &U, double v[2], int64_t i, int32_t row)
{
    unit_pick(J, v);                                       // (both columns: the D1 value; unit_map passes a moment map through)
    v[0] = unit_moment_term(J, U, J.map0, J.cap0, v[0], i, row);
    v[1] = unit_moment_term(J, U, J.map1, J.cap1, v[1], i, row);
}


// ---- selection mode (UnitSelect, pccm_internal.h) ---------------------------------------------------------------------------
// The k-th smallest value of a job's column 0.  Keys: order_key of the value -- every value a report ranks is a square or a
// sum of squares (non-negative, never -0.0, never NaN), for which the plain bit pattern would order too; the sign-flip keeps the
// mode right for a column that does hold negative values.  Counts are 32 bits wide: the host refuses columns of 2^32 rows or more.
__device__ __forceinline__ int sel_shift(int p) { return p >= kSelPasses - 1 ? 0 : 64 - kSelBits * (p + 1); }

__device__ __forceinline__ double sel_value(unsigned long long key)         // inverse of order_key
{
    const unsigned long long b = (key >> 63) ? (key ^ 0x8000000000000000ull) : ~key;
    return __longlong_as_double((long long)b);
}

// What pass p (1..kSelPasses; kSelPasses: the resolve launch) matches and ranks by, for the m <= kSelPerCol selections s0.. of
// one job: from what pass p - 1 matched by (SelState; {0, k} for pass 0) and its counts -- the bin that holds the k-th row
// extends the prefix, the rows in the bins below it leave the rank.  Selections whose prefixes were equal in pass p - 1 shared
// one histogram, the first one's.  Every workgroup computes the same numbers; 256 threads, 8 bins each.
__device__ __forceinline__ void sel_derive(const UnitSelect &S, int p, int s0, int m, uint32_t *wsum, SelState *cur)
{
    unsigned long long ppre[kSelPerCol], pk[kSelPerCol];
#pragma unroll
    for (int r = 0; r < kSelPerCol; ++r) {
        ppre[r] = 0;
        pk[r] = 0;
        if (r < m) {
            if (p == 1) pk[r] = S.k[s0 + r];
            else { const SelState st = S.state[(p - 1) * kSelMax + s0 + r]; ppre[r] = st.prefix; pk[r] = st.k; }
        }
    }
    const int t = threadIdx.x, w = t >> 6;
#pragma unroll
    for (int r = 0; r < kSelPerCol; ++r) {
        if (r >= m) break;                                      // (uniform)
        int lead = r;
#pragma unroll
        for (int r2 = r - 1; r2 >= 0; --r2)
            if (ppre[r2] == ppre[r]) lead = r2;
        const uint32_t *h = S.hist + ((size_t)(p - 1) * kSelMax + s0 + lead) * kSelBins + 8 * t;
        const uint4 a = *reinterpret_cast<const uint4 *>(h), b = *reinterpret_cast<const uint4 *>(h + 4);
        const uint32_t c[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t tsum = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) tsum += c[j];
        uint32_t incl = tsum;                                   // (sums stay below 2^32: they count rows of one column)
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off);
            if ((t & 63) >= off) incl += o;
        }
        if ((t & 63) == 63) wsum[w] = incl;
        if (t == 0) cur[r] = SelState{ppre[r], pk[r]};          // (never kept: some bin holds the k-th row)
        __syncthreads();
        unsigned long long run = incl - tsum;
        for (int j = 0; j < w; ++j) run += wsum[j];
        const unsigned long long kk = pk[r];
        if (run < kk && kk <= run + tsum) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (run < kk && kk <= run + c[j])
                    cur[r] = SelState{ppre[r] | ((unsigned long long)(8 * t + j) << sel_shift(p - 1)), kk - run};
                run += c[j];
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void unit_select(const UnitJobs &jobs, unsigned char *smem)
{
    const UnitSelect &S = jobs.sel;
    uint32_t *lh = reinterpret_cast<uint32_t *>(smem);                                  // [kSelPerCol][kSelBins]
    SelState *cur = reinterpret_cast<SelState *>(smem + (size_t)kSelPerCol * kSelBins * sizeof(uint32_t));     // [kSelPerCol]
    uint32_t *wsum = reinterpret_cast<uint32_t *>(cur + kSelPerCol);                    // [4]
    const int p = S.pass - 1;
    const int t = threadIdx.x;
    if (p >= kSelPasses) {                                      // resolve: one workgroup, job after job
        for (int jb = 0; jb < jobs.njobs; ++jb) {
            const int s0 = S.sfirst[jb], m = S.sfirst[jb + 1] - s0;
            sel_derive(S, kSelPasses, s0, m, wsum, cur);
            for (int r = 0; r < m; ++r)
                if (t == r) *S.out[s0 + r] = sel_value(cur[r].prefix);     // after the last pass the prefix is the whole key
            __syncthreads();
        }
        return;
    }
    int jb = 0;
#pragma unroll
    for (int k = 1; k < 8; ++k)
        if (k < jobs.njobs && (int)blockIdx.x >= S.boff[k]) jb = k;
    jb = __builtin_amdgcn_readfirstlane(jb);
    const int s0 = S.sfirst[jb], m = S.sfirst[jb + 1] - s0;
    const int blk = (int)blockIdx.x - S.boff[jb], nblk = S.boff[jb + 1] - S.boff[jb];
    unsigned long long cpre[kSelPerCol];
    bool own[kSelPerCol];                                       // the selection has a histogram of its own in this pass
    if (p > 0) sel_derive(S, p, s0, m, wsum, cur);
#pragma unroll
    for (int r = 0; r < kSelPerCol; ++r) {
        cpre[r] = (p > 0 && r < m) ? cur[r].prefix : 0ull;
        own[r] = r < m;
#pragma unroll
        for (int r2 = 0; r2 < r; ++r2)
            if (cpre[r2] == cpre[r]) own[r] = false;
    }
    if (p > 0 && blk == 0 && t < m) S.state[p * kSelMax + s0 + t] = cur[t];
    for (int b = t; b < m * kSelBins; b += 256) lh[b] = 0u;
    __syncthreads();
    const UnitView V = unit_view(jobs.j[jb]);
    const int64_t ns = jobs.j[jb].ns;
    const int sh = sel_shift(p), above = p > 0 ? sel_shift(p - 1) : 0;
    const unsigned mask = p == kSelPasses - 1 ? (1u << (64 - kSelBits * (kSelPasses - 1))) - 1u : (unsigned)kSelBins - 1u;
    auto count = [&](double v) {
        const unsigned long long key = order_key(v);
        const unsigned bin = (unsigned)(key >> sh) & mask;
#pragma unroll
        for (int r = 0; r < kSelPerCol; ++r)
            if (own[r] && (p == 0 || ((key ^ cpre[r]) >> above) == 0ull)) atomicAdd(&lh[r * kSelBins + bin], 1u);
    };
    const int64_t step = (int64_t)nblk * 256;
    int64_t i = (int64_t)blk * 256 + t;
    for (; i + 3 * step < ns; i += 4 * step) {                  // four independent loads in flight
        double v[4][2];
#pragma unroll
        for (int j = 0; j < 4; ++j) unit_load(V, i + j * step, v[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unit_pick(V, v[j]);
            count(v[j][0]);
        }
    }
    for (; i < ns; i += step) {
        double v[2];
        unit_load(V, i, v);
        unit_pick(V, v);
        count(v[0]);
    }
    __syncthreads();
    // integer adds commute: the global counts do not depend on the order the workgroups arrive in
#pragma unroll
    for (int r = 0; r < kSelPerCol; ++r) {
        if (!own[r]) continue;
        uint32_t *g = S.hist + ((size_t)p * kSelMax + s0 + r) * kSelBins;
        for (int b = t; b < kSelBins; b += 256) {
            const uint32_t c = lh[r * kSelBins + b];
            if (c) atomicAdd(&g[b], c);
        }
    }
}

// ---- count mode (UnitSelect::pass kSelCountPass / kSelStorePass, pccm_internal.h) -------------------------------------------
// The inverse query of the selection: how many rows of a job's column 0 are <= x, for the m <= kSelPerCol thresholds s0.. of the
// job (UnitSelect::k holds their bit patterns).  The comparison is the IEEE one on the values unit_load / unit_pick form, not one
// of order keys: 0.0 <= -0.0 holds, a NaN row is counted by no threshold.  One streaming pass laid out as a histogram pass is
// (UnitSelect::boff); a counter per threshold in registers, combined across the wave by shuffles, across the workgroup through
// 64 bytes of the selection's LDS, and added to the zeroed device counters (the first kSelMax words of UnitSelect::hist) with one
// atomic per threshold and workgroup.  The store launch, one workgroup behind it, widens the counters into the slots' host words.
__device__ __forceinline__ void unit_count(const UnitJobs &jobs, unsigned char *smem)
{
    const UnitSelect &S = jobs.sel;
    const int t = threadIdx.x;
    if (S.pass == kSelStorePass) {
        for (int s = 0; s < S.nsel; ++s)
            if (t == s) *reinterpret_cast<unsigned long long *>(S.out[s]) = (unsigned long long)S.hist[s];
        return;
    }
    uint32_t *wc = reinterpret_cast<uint32_t *>(smem);         // [4 waves][kSelPerCol]
    int jb = 0;
#pragma unroll
    for (int k = 1; k < 8; ++k)
        if (k < jobs.njobs && (int)blockIdx.x >= S.boff[k]) jb = k;
    jb = __builtin_amdgcn_readfirstlane(jb);
    const int s0 = S.sfirst[jb], m = S.sfirst[jb + 1] - s0;
    const int blk = (int)blockIdx.x - S.boff[jb], nblk = S.boff[jb + 1] - S.boff[jb];
    double x[kSelPerCol];
    uint32_t c[kSelPerCol];
#pragma unroll
    for (int r = 0; r < kSelPerCol; ++r) {
        x[r] = __longlong_as_double((long long)S.k[s0 + (r < m ? r : 0)]);
        c[r] = 0u;
    }
    const UnitView V = unit_view(jobs.j[jb]);
    const int64_t ns = jobs.j[jb].ns;
    const int64_t step = (int64_t)nblk * 256;
    int64_t i = (int64_t)blk * 256 + t;
    for (; i + 3 * step < ns; i += 4 * step) {                  // four independent loads in flight
        double v[4][2];
#pragma unroll
        for (int j = 0; j < 4; ++j) unit_load(V, i + j * step, v[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unit_pick(V, v[j]);
#pragma unroll
            for (int r = 0; r < kSelPerCol; ++r) c[r] += v[j][0] <= x[r] ? 1u : 0u;
        }
    }
    for (; i < ns; i += step) {
        double v[2];
        unit_load(V, i, v);
        unit_pick(V, v);
#pragma unroll
        for (int r = 0; r < kSelPerCol; ++r) c[r] += v[0] <= x[r] ? 1u : 0u;
    }
#pragma unroll
    for (int r = 0; r < kSelPerCol; ++r) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c[r] += __shfl_xor(c[r], off);
        if ((t & 63) == 0) wc[(t >> 6) * kSelPerCol + r] = c[r];
    }
    __syncthreads();
    // integer adds commute: the global counts do not depend on the order the workgroups arrive in
    if (t < m) atomicAdd(&S.hist[s0 + t], wc[t] + wc[kSelPerCol + t] + wc[2 * kSelPerCol + t] + wc[3 * kSelPerCol + t]);
}

// ---- the leaf reduction, written once (UnitCols / LeanCols: what a record is; k_unit_jobs / k_unit_lean: who runs it) ----------
// A policy type says how a job's records become column values and nothing else: NC, the columns the kernel carries (compile
// time: loops over columns with constant bounds keep r / mn / mx in registers -- DESIGN.md, "k_unit_jobs compiled for gfx950");
// live(c): column c is reduced and stored; leaf(base, k, v): the values of rows base + k + 8 j of a full leaf, the sixteen
// loads of lane k issued together; one(i, v): the values of row i; min / max: what orders the extrema.
__device__ __forceinline__ double dmin_raw(double a, double b)       // operands are finite: no canonicalisation needed
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double dmax_raw(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// The layout read from the job at run time: every shape, two columns carried whether the job has one or two.  fmin / fmax: a
// signed projection column holds -0.0 beside 0.0, which the raw instructions do not order.
struct UnitCols {
    static constexpr int NC = 2;
    const UnitView V;
    const int ncols;
    __device__ __forceinline__ explicit UnitCols(const UnitJob &J) : V(unit_view(J)), ncols(J.ncols) {}
    __device__ __forceinline__ bool live(int c) const { return c < ncols; }
    static constexpr bool rowwise() { return false; }
    static __device__ __forceinline__ double min(double a, double b) { return fmin(a, b); }
    static __device__ __forceinline__ double max(double a, double b) { return fmax(a, b); }
    __device__ __forceinline__ void one(int64_t i, double v[2]) const
    {
        unit_load(V, i, v);
        unit_pick(V, v, unit_dense(V) ? unit_count_of(V, unit_row(V, i)) : 1u);
    }
    __device__ __forceinline__ void leaf(int64_t base, int k, double v[kLeaf / 8][2]) const
    {
        __builtin_assume((base & (kLeaf - 1)) == 0 && k >= 0 && k < 8);       // (see LeanCols::leaf)
        // sixteen independent loads first; the layout test sits outside the loop so that they are issued together
        if (V.stride >= 2 && V.defer) {
#pragma unroll
            for (int j = 0; j < kLeaf / 8; ++j) unit_load(V, base + 8 * j + k, v[j]);
        } else if (V.stride >= 2) {
#pragma unroll
            for (int j = 0; j < kLeaf / 8; ++j) {
                const double2 t = *reinterpret_cast<const double2 *>(&V.val[(base + 8 * j + k) * V.stride]);
                v[j][0] = t.x;
                v[j][1] = t.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kLeaf / 8; ++j) v[j][0] = v[j][1] = V.val[base + 8 * j + k];
        }
        if (unit_dense(V)) {
            // the density map: the sixteen rows come with (or beside) the sixteen records above, then the sixteen gathers of
            // their counts go out together -- no gather waits on its own record alone
            int32_t row[kLeaf / 8];
            uint32_t m[kLeaf / 8];
#pragma unroll
            for (int j = 0; j < kLeaf / 8; ++j) row[j] = unit_row(V, base + 8 * j + k);
#pragma unroll
            for (int j = 0; j < kLeaf / 8; ++j) m[j] = unit_count_of(V, row[j]);
#pragma unroll
            for (int j = 0; j < kLeaf / 8; ++j) unit_pick(V, v[j], m[j]);
            return;
        }
#pragma unroll
        for (int j = 0; j < kLeaf / 8; ++j) unit_pick(V, v[j]);
    }
};

// The alignment moments (PCCM_MAP_MOMENT; a launch's jobs are all moment jobs or none is): UnitCols' records, read the same way,
// and the moment term in the map's place.  A policy and a branch of its own in k_unit_jobs, so that the registers the term needs
// -- the two clouds' rows, the pivot, two kinds -- are live in that branch alone: carried through UnitCols they made the other
// jobs' sixteen-load leaf spill.  Row-wise: every row gathers up to four doubles of the two clouds, so a full leaf is formed one
// row at a time by unit_leaves' sequential path (leaf() is never called).  fmin / fmax: a term can be -0.0.
struct MomentCols {
    static constexpr int NC = 2;
    const UnitView V;
    const UnitJob &U;              // (the term's operands are read from the job itself: unit_moment_term)
    const int ncols;
    __device__ __forceinline__ explicit MomentCols(const UnitJob &J) : V(unit_view(J)), U(J), ncols(J.ncols) {}
    __device__ __forceinline__ bool live(int c) const { return c < ncols; }
    static constexpr bool rowwise() { return true; }
    static __device__ __forceinline__ double min(double a, double b) { return fmin(a, b); }
    static __device__ __forceinline__ double max(double a, double b) { return fmax(a, b); }
    __device__ __forceinline__ void one(int64_t i, double v[2]) const
    {
        unit_load(V, i, v);
        unit_moment_pick(V, U, v, i, unit_row(V, i));
    }
    __device__ __forceinline__ void leaf(int64_t, int, double[kLeaf / 8][2]) const {}
};

// The jobs' shape fixed at compile time (every report's jobs share one shape; ReduceShape, pccm_reduce_shape.h): record stride
// and which field feeds which column are template arguments, so the sixteen loads of a lane are one base address + immediate
// offsets and no value passes through a select.  CFG 0: two columns {field 0, field 1 squared} (D1 + D2 of a direction in
// one pass over its result records), 1: field 0, 2: field 1 squared.  A signed projection column (field 1 as it is) has no
// such kernel: its minimum and maximum need fmin / fmax (-0.0 beside 0.0), so it goes to the general kernel.  (That kernel
// spends most of its 20 us at 1M + 1M points on per-value selects, 64-bit index products and dependent scalar loads; a kernel
// of this shape streams the same 32 MB in 7 us: scripts/micro/reduce_gap.hip.)
template <int STRIDE, int CFG, int DEFER>          // DEFER: UnitJob::defer of every job (records of layout 1; STRIDE 2)
struct LeanCols {
    static constexpr int NC = CFG == 0 ? 2 : 1;
    const double *__restrict__ val, *__restrict__ nrm64;
    const float4 *__restrict__ nrm32, *__restrict__ q32;
    const int64_t row0, nrm_rows;
    __device__ __forceinline__ explicit LeanCols(const UnitJob &J)
        : val(J.val), nrm64(J.nrm64), nrm32(J.nrm32), q32(J.q32), row0(J.row0), nrm_rows(J.nrm_rows) {}
    __device__ __forceinline__ bool live(int) const { return true; }
    static constexpr bool rowwise() { return false; }
    static __device__ __forceinline__ double min(double a, double b) { return dmin_raw(a, b); }
    static __device__ __forceinline__ double max(double a, double b) { return dmax_raw(a, b); }
    __device__ __forceinline__ void one(int64_t i, double out[NC]) const { at(val + i * STRIDE, i, out); }
    __device__ __forceinline__ void at(const double *p, int64_t i, double out[NC]) const       // p: record i
    {
        double x, y = 0.0;
        if (DEFER) {
            matched_fields(*reinterpret_cast<const float4 *>(p), q32, DEFER, nrm64, nrm32, row0 + i, CFG != 1, x, y, nrm_rows);
        } else if (STRIDE >= 2) {
            const double2 q = *reinterpret_cast<const double2 *>(p);
            x = q.x; y = q.y;
        } else {
            x = *p;
        }
        if (CFG == 0) { out[0] = x; out[1] = __dmul_rn(y, y); }
        else out[0] = CFG == 1 ? x : __dmul_rn(y, y);
    }
    __device__ __forceinline__ void leaf(int64_t base, int k, double v[kLeaf / 8][NC]) const
    {
        // What the kernel knows of a leaf's first row and the lane's place in it, said here because this function is optimised
        // before it is inlined: the row indices then stay base | k | 8 j, as they were when the loop stood in the kernel.  Folded
        // into row0 + first they cost the kernels with fp64 normals 10 to 18 VGPRs (<2, 2, 2>: three waves per SIMD for four)
        __builtin_assume((base & (kLeaf - 1)) == 0 && k >= 0 && k < 8);
        const int64_t first = base + k;
        const double *p = val + first * STRIDE;            // one base address + immediate offsets
#pragma unroll
        for (int j = 0; j < kLeaf / 8; ++j) at(p + (int64_t)j * 8 * STRIDE, first + 8 * j, v[j]);
    }
};

// the job position `pos` falls into, for prefix sums `off` of the jobs' extents
__device__ __forceinline__ int unit_job_at(const int64_t (&off)[9], int njobs, int64_t pos)
{
    int jb = 0;
#pragma unroll
    for (int k = 1; k < 8; ++k)
        if (k < njobs && pos >= off[k]) jb = k;
    return jb;
}

// The leaves of job jb this workgroup owns (lane t of the launch; 8 lanes per leaf, 32 leaves per workgroup): per-leaf and
// per-workgroup sums, minima and maxima.  The order of the additions is NumPy's (K5 above).
template <class P>
__device__ __forceinline__ void unit_leaves(const UnitJobs &jobs, int jb, int64_t t)
{
    constexpr int NC = P::NC;
    __shared__ double ls[NC][32], lmn[NC][32], lmx[NC][32];
    const UnitJob &J = jobs.j[jb];
    const P cols(J);
    const int64_t ns = J.ns, nunits = J.nunits;
    const int64_t lane = t - jobs.uoff[jb], u = lane >> 3;
    const int k = threadIdx.x & 7, grp = threadIdx.x >> 3;
    const int64_t base = u * kLeaf;
    const bool live = u < nunits;
    const int64_t cnt = !live ? 0 : ((ns - base < kLeaf) ? ns - base : kLeaf);
    double r[NC], mn[NC], mx[NC];
    if (cnt == kLeaf && !P::rowwise()) {
        double v[kLeaf / 8][NC];
        cols.leaf(base, k, v);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            r[c] = v[0][c];
            mn[c] = mx[c] = v[0][c];
#pragma unroll
            for (int j = 1; j < kLeaf / 8; ++j) {
                r[c] = __dadd_rn(r[c], v[j][c]);
                mn[c] = P::min(mn[c], v[j][c]);
                mx[c] = P::max(mx[c], v[j][c]);
            }
        }
    } else {
#pragma unroll
        // (a row-wise job's full leaves come here too: from -0.0, the identity of the addition, its lane adds the same sixteen
        // values in the same order as the unrolled path, which starts from the first of them)
        for (int c = 0; c < NC; ++c) { r[c] = P::rowwise() ? -0.0 : 0.0; mn[c] = INFINITY; mx[c] = -INFINITY; }
        for (int64_t e = k; e < cnt; e += 8) {
            double w[NC];
            cols.one(base + e, w);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                r[c] = __dadd_rn(r[c], w[c]);
                mn[c] = P::min(mn[c], w[c]);
                mx[c] = P::max(mx[c], w[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
            r[c] = __dadd_rn(r[c], __shfl_xor(r[c], off));
            mn[c] = P::min(mn[c], __shfl_xor(mn[c], off));
            mx[c] = P::max(mx[c], __shfl_xor(mx[c], off));
        }
    }
    if (k == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {                     // (constant bounds: r / mn / mx stay in registers)
            double *ou = cols.live(c) ? J.c[c].out_units : nullptr;
            if (live && ou) {                              // per-leaf results: the sharded exchange needs them
                ou[u] = r[c];
                ou[nunits + u] = mn[c];
                ou[2 * nunits + u] = mx[c];
            }
            ls[c][grp] = r[c];
            lmn[c][grp] = mn[c];
            lmx[c][grp] = mx[c];
        }
    }
    __syncthreads();
    if (threadIdx.x < 32 * NC) {
        // this block's 32 leaves = one half of an 8192-row NumPy chunk when the shard starts on a chunk
        // boundary: finish NumPy's pairwise tree for the half here (adjacent pairs, five levels), so the
        // host only adds 2 numbers per chunk instead of walking 64 leaves.  Lanes 0..31: column 0, 32..63: column 1.
        const int c = threadIdx.x >> 5, l = threadIdx.x & 31;
        double s = ls[c][l], a = lmn[c][l], b = lmx[c][l];
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {
            s = __dadd_rn(s, __shfl_xor(s, off));
            a = P::min(a, __shfl_xor(a, off));
            b = P::max(b, __shfl_xor(b, off));
        }
        if (l == 0 && cols.live(c)) {
            const int64_t blk = lane >> 8;
            double *ob = J.c[c].out_blocks;
            ob[blk] = s;
            ob[J.nblocks + blk] = a;
            ob[2 * J.nblocks + blk] = b;
        }
    }
}

// raw values of the last, partial 8192-row chunk (NumPy sums them with its own tree on the host); c0: lane behind the leaves' lanes
template <class P>
__device__ __forceinline__ void unit_tail(const UnitJobs &jobs, int64_t c0)
{
    if (c0 >= jobs.toff[jobs.njobs]) return;
    const int jb = unit_job_at(jobs.toff, jobs.njobs, c0);
    const UnitJob &J = jobs.j[jb];
    const P cols(J);
    const int64_t e = c0 - jobs.toff[jb];
    double v[P::NC];
    cols.one(J.tail_first + e, v);
#pragma unroll
    for (int c = 0; c < P::NC; ++c)
        if (cols.live(c)) J.c[c].out_tail[e] = v[c];
}

__global__ __launch_bounds__(256) void k_unit_jobs(UnitJobs jobs)
{
    __shared__ __attribute__((aligned(16))) unsigned char sel_smem[kSelLds];      // selection and count launches only
    if (jobs.sel.pass) {                                   // block-uniform (a kernel argument)
        if (jobs.sel.pass >= kSelCountPass) unit_count(jobs, sel_smem);
        else unit_select(jobs, sel_smem);
        return;
    }
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t unit_threads = jobs.uoff[jobs.njobs];
    if (jobs.j[0].c[0].map & PCCM_MAP_MOMENT) {            // launch-uniform (a kernel argument): pccm_reduce_moment_*'s launches
        if (t < unit_threads) unit_leaves<MomentCols>(jobs, __builtin_amdgcn_readfirstlane(unit_job_at(jobs.uoff, jobs.njobs, t)), t);
        else unit_tail<MomentCols>(jobs, t - unit_threads);
        return;
    }
    if (t < unit_threads)                                  // block-uniform: jobs start at multiples of 256 lanes
        // (the job index is block-uniform by construction: readfirstlane makes the job's fields scalar loads)
        unit_leaves<UnitCols>(jobs, __builtin_amdgcn_readfirstlane(unit_job_at(jobs.uoff, jobs.njobs, t)), t);
    else
        unit_tail<UnitCols>(jobs, t - unit_threads);
}

// The settling head of k_unit_lean (filed tails, pccm_tail_wave.h): jobs over matched records whose direction's search left the tail
// launch out.  A workgroup owns 4096 consecutive rows of its job; the queries ring 1 did not settle among them lie filed under that
// block, a handful at most.  The workgroup reads its block's count (uniform: a scalar load), wave w settles entries w, w + 4, ...
// with the tail kernel's own search (wave_settle) and stores their matched records, and only then runs the unchanged leaf
// reduction over records that are all there.  The workgroups that copy the raw rows of the column's last, partial chunk
// (unit_tail) read rows of blocks that leaf workgroups own: they settle the entries of the (at most two per job) blocks their
// rows lie in for themselves -- the same stores, bit for bit.  So every workgroup reads only records that the search kernel
// wrote before the launch or that its own waves wrote: the hand-over is between waves of one workgroup (drained stores, then the
// barrier, whose workgroup-scope release / acquire is all one CU's L1 needs), nothing is waited for, nothing is polled, and no
// agent-scope fence writes an L2 back (k_grid_tail's notes: 57 against 12 us with one per workgroup).  A query three rings do not
// settle has no exact rescan behind it here (the capture rule saw none on these clouds): it raises the device error word.
// -> whether the block held entries (block-uniform)
__device__ __forceinline__ bool settle_block(const TailSettle &ts, const TailSettleDir &D, int64_t blk)
{
    uint32_t n = D.cnt[blk];                               // block-uniform: a scalar load
    if (!n) return false;
    n = n < (uint32_t)kTailBlockCap ? n : (uint32_t)kTailBlockCap;      // (a longer list raised the error word when it was filed)
    const int lane = threadIdx.x & 63;
    for (uint32_t e = threadIdx.x >> 6; e < n; e += 4) {
        const float4 q = D.list[blk * kTailBlockCap + e];  // wave-uniform
        P3 qa;
        qa.x = (double)q.x; qa.y = (double)q.y; qa.z = (double)q.z;
        qa.row = __float_as_int(q.w);
        BestAt b;
        const bool done = wave_settle<Rec32, false>(ts.g, D.cs, D.srecs, qa, lane, b);
        if (lane == 0) {
            if (done && b.idx != 0x7fffffff) D.out[qa.row] = make_float4((float)b.x, (float)b.y, (float)b.z, __int_as_float(b.idx));
            else if (ts.err) atomicOr(ts.err, kErrTailFiled);
        }
    }
    return true;
}

// The shapes that settle: those whose kernel loses no occupancy to the search's registers (VGPRs without -> with the settling head,
// waves per SIMD): <2, 0, 1> 102 -> 117, 4 -> 4 (D1 + D2 of a direction in one pass, fp32-exact normals: what a report reduces);
// <2, 0, 2> 112 -> 126 and <2, 2, 2> 118 -> 127, 4 -> 4 (fp64 normals).  The single-column shapes would fall from 6 waves to 4
// (<2, 1, *> 74 -> 113) or 3 (<2, 2, 1> 78 -> 134): a batch of those keeps the tail launch.
constexpr bool lean_settles(int stride, int cfg, int defer)
{
    return stride == 2 && ((cfg == 0 && (defer == 1 || defer == 2)) || (cfg == 2 && defer == 2));
}

template <int STRIDE, int CFG, int DEFER = 0>
__global__ __launch_bounds__(256) void k_unit_lean(UnitJobs jobs, TailSettle ts)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, t0 = (int64_t)blockIdx.x * 256;
    const int64_t unit_threads = jobs.uoff[jobs.njobs];
    const bool leaves = t0 < unit_threads;                 // block-uniform: jobs start at multiples of 256 lanes
    const int jb = leaves ? unit_job_at(jobs.uoff, jobs.njobs, t0) : 0;
    if constexpr (lean_settles(STRIDE, CFG, DEFER)) {
        if (ts.on) {                                       // (a kernel argument: launches that settle nothing pay one scalar branch)
            bool stored = false;
            if (leaves) {
                const int entry = jobs.j[jb].settle - 1;
                if (entry >= 0) stored = settle_block(ts, ts.d[entry], (t0 - jobs.uoff[jb]) >> 8);      // 256 lanes = 32 leaves = 4096 rows
            } else {
                const int64_t c0 = t0 - unit_threads, c1 = c0 + 255;           // this workgroup's raw rows, counted over all jobs
                for (int k = 0; k < jobs.njobs; ++k) {
                    const UnitJob &J = jobs.j[k];
                    const int64_t lo = c0 > jobs.toff[k] ? c0 : jobs.toff[k], hi = c1 < jobs.toff[k + 1] - 1 ? c1 : jobs.toff[k + 1] - 1;
                    if (lo > hi || !J.settle) continue;
                    const int64_t r_lo = J.tail_first + (lo - jobs.toff[k]), r_hi = J.tail_first + (hi - jobs.toff[k]);
                    for (int64_t blk = r_lo >> kTailBlockShift; blk <= r_hi >> kTailBlockShift; ++blk)
                        stored = settle_block(ts, ts.d[J.settle - 1], blk) || stored;
                }
            }
            if (stored) {                                  // block-uniform
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
        }
    }
    if (leaves) unit_leaves<LeanCols<STRIDE, CFG, DEFER>>(jobs, jb, t);
    else unit_tail<LeanCols<STRIDE, CFG, DEFER>>(jobs, t - unit_threads);
}

// A batch's completion, published to the host: one wave launched behind the batch's last reduction kernel on the same stream
// bumps the context's completion counter (pccm_ctx::done).  The stream starts it once that kernel has ended, i.e. once every store
// of the batch has left its workgroup; the outputs live in host-coherent memory, so no XCD's L2 holds any of them, and the
// system-scope release covers whatever else this wave's L2 holds.  The inline wait stays in asm: the compiler may drop the
// s_waitcnt behind buffer_wbl2 when it thinks the counter empty (MI355X_MICROARCH.md).  This wave costs ~4 us of GPU time at
// the end of the batch.  Publishing from k_unit_lean itself was measured too: every workgroup drained its stores, and the last
// one to arrive bumped the counter.  That made the kernel 3.6 us longer at 1M + 1M points for the same step time (DESIGN.md
// section 4).
__global__ __launch_bounds__(64) void k_publish(unsigned long long *done)
{
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");                                    // system scope
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(done, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// the kernel of every shape pccm_reduce_shape.h lists, row for row: adding a shape is a row there and a row here
struct LeanKernel {
    ReduceShape shape;
    void (*stub)(UnitJobs, TailSettle);
};
template <int STRIDE, int CFG, int DEFER>
constexpr LeanKernel lean() { return {{STRIDE, CFG, DEFER}, k_unit_lean<STRIDE, CFG, DEFER>}; }
static constexpr LeanKernel kLeanKernels[] = {
    lean<1, 1, 0>(),
    lean<2, 0, 0>(),
    lean<2, 1, 0>(),
    lean<2, 2, 0>(),
    lean<4, 0, 0>(),
    lean<4, 1, 0>(),
    lean<4, 2, 0>(),
    lean<2, 0, 1>(),      // matched records, fp32-exact normals
    lean<2, 1, 1>(),
    lean<2, 2, 1>(),
    lean<2, 0, 2>(),      // ... fp64 normals
    lean<2, 1, 2>(),
    lean<2, 2, 2>(),
    lean<2, 1, 3>(),      // ... no normals: distances only
    lean<2, 0, 4>(),      // ... the matched row's normal, fp32-exact
    lean<2, 2, 4>(),
    lean<2, 0, 5>(),      // ... fp64
    lean<2, 2, 5>(),
};
constexpr bool lean_rows_match()
{
    if (sizeof(kLeanKernels) / sizeof(kLeanKernels[0]) != (size_t)kLeanCount) return false;
    for (int i = 0; i < kLeanCount; ++i)
        if (!(kLeanKernels[i].shape == kLeanShapes[i])) return false;
    return true;
}
static_assert(lean_rows_match(), "kLeanKernels and kLeanShapes (pccm_reduce_shape.h) must list the same shapes in the same order");

static bool shape_settles(const ReduceShape &s) { return lean_settles(s.stride, s.cfg, s.defer); }

// one launch for jobs of one shape (lean: row of kLeanShapes, or -1: the general kernel)
static void launch_unit_shape(pccm_ctx *ctx, const UnitJobs &jobs, int lean, const TailSettle *settle = nullptr)
{
    const int64_t total = jobs.uoff[jobs.njobs] + jobs.toff[jobs.njobs];
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    TailSettle ts{};                                       // (on = 0: nothing to settle)
    for (int k = 0; k < jobs.njobs && settle; ++k)
        if (jobs.j[k].settle) ts = *settle;
    if (lean >= 0) PCCM_LAUNCH_STUB(ctx, kLeanKernels[lean].stub, grid, block, 0, ctx->stream, jobs, ts);
    else PCCM_LAUNCH(ctx, k_unit_jobs, grid, block, 0, ctx->stream, jobs);      // signed projections (min / max of -0.0 and 0.0: fmin / fmax there), other shapes
}

int launch_unit_jobs(pccm_ctx *ctx, const UnitJobs &jobs_in, uint64_t *seq)
{
    *seq = 0;
    UnitJobs jobs = jobs_in;                  // (filed tails: the settle fields are set here)
    const int64_t total = jobs.uoff[jobs.njobs] + jobs.toff[jobs.njobs];
    if (total <= 0) return PCCM_OK;
    ProfScope ps(ctx, PCCM_K_REDUCE);
    static const bool general = [] { const char *e = getenv("PCCM_REDUCE_GENERAL"); return e && e[0] == '1'; }();   // A/B: always the general kernel
    int shape[8], nshapes = 0, first_of[8];
    bool all_lean = !general;
    for (int k = 0; k < jobs.njobs; ++k) {
        shape[k] = lean_index(reduce_shape(jobs.j[k]));       // row of kLeanShapes, or -1
        all_lean = all_lean && shape[k] >= 0;
        bool seen = false;
        for (int j = 0; j < nshapes; ++j) seen = seen || shape[first_of[j]] == shape[k];
        if (!seen) first_of[nshapes++] = k;
    }
    // Filed tails (pccm_tail_wave.h).  A direction whose search left its tail launch out is settled by this batch when every
    // job that reads the direction's records covers all of its rows and has a settling kernel: those jobs are marked, and the
    // direction's form no longer says filed.  A batch that reads such records any other way has the classic tail launch first.
    // An eager batch notes per direction whether it could have (pccm_ctx::TailFile::eager_ok / eager_bad): the capture behind it
    // files only what its reductions will settle.
    const TailSettle *settle = nullptr;
    bool classic = false;
    for (int d = 0; d < 2; ++d) {
        int entry = -1;
        const TailSettle *ts = filed_tails_settle(ctx, d, &entry);
        if (!ts && ctx->capturing) continue;
        NNResult &res = ctx->nn[d];
        if (!res.valid || !res.rec.p) continue;
        bool ok = all_lean;
        int readers = 0;
        for (int k = 0; k < jobs.njobs; ++k) {
            if (jobs.j[k].val != (const double *)res.rec.p) continue;
            ++readers;
            ok = ok && shape[k] >= 0 && shape_settles(kLeanShapes[shape[k]]) && jobs.j[k].row0 == 0 && jobs.j[k].ns == res.end - res.begin;
        }
        if (readers == 0) continue;            // (not this batch's direction: it stays filed)
        if (!ctx->capturing) (ok ? ctx->tail_file.eager_ok : ctx->tail_file.eager_bad) |= 1 << d;
        if (!ts) continue;
        if (!ok) { classic = true; continue; }
        for (int k = 0; k < jobs.njobs; ++k)
            if (jobs.j[k].val == (const double *)res.rec.p) jobs.j[k].settle = entry + 1;
        res.form.tails_filed = false;
        settle = ts;
    }
    if (classic) {
        const int rc = filed_tails_resolve(ctx);
        if (rc) return rc;
    }
    if (!all_lean) {                          // one shape nobody specialised: the general kernel takes the whole batch
        launch_unit_shape(ctx, jobs, -1);
    } else if (nshapes == 1) {
        launch_unit_shape(ctx, jobs, shape[0], settle);
    } else {
        // jobs of different shapes (the pair's two directions with the projection, the self search without): one specialised launch
        // per shape -- the general kernel costs more than a second launch (53 against 20 + 9 us on the 0.8M-point content pair)
        for (int g = 0; g < nshapes; ++g) {
            UnitJobs sub;
            sub.njobs = 0;
            sub.uoff[0] = sub.toff[0] = 0;
            for (int k = 0; k < jobs.njobs; ++k) {
                if (shape[k] != shape[first_of[g]]) continue;
                sub.j[sub.njobs] = jobs.j[k];
                sub.uoff[sub.njobs + 1] = sub.uoff[sub.njobs] + (jobs.uoff[k + 1] - jobs.uoff[k]);
                sub.toff[sub.njobs + 1] = sub.toff[sub.njobs] + (jobs.toff[k + 1] - jobs.toff[k]);
                sub.njobs++;
            }
            for (int k = sub.njobs; k < 8; ++k) {
                sub.j[k] = sub.j[0];
                sub.uoff[k + 1] = sub.uoff[sub.njobs];
                sub.toff[k + 1] = sub.toff[sub.njobs];
            }
            launch_unit_shape(ctx, sub, shape[first_of[g]], settle);
        }
    }
    return launch_publish(ctx, seq);
}

// the batch's completion, published behind its last launch.  The count the counter will reach is taken before the launch
// is issued, so that a launch that fails can only make a waiter fall back to the event, never wake it early.
int launch_publish(pccm_ctx *ctx, uint64_t *seq)
{
    *seq = ctx->capturing ? ++ctx->cap_batches : ++ctx->batches_issued;
    PCCM_LAUNCH(ctx, k_publish, dim3(1), dim3(64), 0, ctx->stream, (unsigned long long *)ctx->done);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

// the workgroups of a histogram or count pass, job after job (UnitSelect::boff); -> their number
static int select_grid(UnitJobs &jobs)
{
    int nb = 0;
    for (int k = 0; k < 8; ++k) {
        jobs.sel.boff[k] = nb;
        if (k < jobs.njobs) {                 // 4096 rows per workgroup, at most one workgroup per CU and job
            const int64_t want = (jobs.j[k].ns + 4095) / 4096;
            nb += (int)(want < 1 ? 1 : want > 256 ? 256 : want);
        }
    }
    jobs.sel.boff[8] = nb;
    return nb;
}

// The selections of jobs.sel: the histograms zeroed on the stream, one launch per radix pass (each reads the counts of the one
// before: the launch boundary is the only synchronisation), one workgroup that resolves the values into pinned host memory.
int launch_unit_select(pccm_ctx *ctx, UnitJobs &jobs)
{
    UnitSelect &S = jobs.sel;
    if (S.nsel <= 0) return PCCM_OK;
    ProfScope ps(ctx, PCCM_K_REDUCE);
    const int nb = select_grid(jobs);
    PCCM_HIP(hipMemsetAsync(S.hist, 0, (size_t)kSelPasses * kSelMax * kSelBins * sizeof(uint32_t), ctx->stream));
    for (int p = 0; p <= kSelPasses; ++p) {
        S.pass = p + 1;
        PCCM_LAUNCH(ctx, k_unit_jobs, dim3(p < kSelPasses ? (unsigned)nb : 1u), dim3(256), 0, ctx->stream, jobs);
    }
    S.pass = 0;
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

// The counts of jobs.sel: the counters (the first kSelMax words of the histograms) zeroed on the stream, one count launch, one
// workgroup that stores the counts into pinned host memory -- the launch boundary is the only synchronisation.
int launch_unit_count(pccm_ctx *ctx, UnitJobs &jobs)
{
    UnitSelect &S = jobs.sel;
    if (S.nsel <= 0) return PCCM_OK;
    ProfScope ps(ctx, PCCM_K_REDUCE);
    const int nb = select_grid(jobs);
    PCCM_HIP(hipMemsetAsync(S.hist, 0, (size_t)kSelMax * sizeof(uint32_t), ctx->stream));
    S.pass = kSelCountPass;
    PCCM_LAUNCH(ctx, k_unit_jobs, dim3((unsigned)nb), dim3(256), 0, ctx->stream, jobs);
    S.pass = kSelStorePass;
    PCCM_LAUNCH(ctx, k_unit_jobs, dim3(1), dim3(256), 0, ctx->stream, jobs);
    S.pass = 0;
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

// Result records -> plain columns (only when a consumer wants them: colour kernels, getters, pccm_nn_fetch).
__global__ __launch_bounds__(256) void k_unpack(const double *__restrict__ rec, int stride, int layout, const float4 *__restrict__ q32, int64_t row0,
                                                int64_t ns, int32_t *__restrict__ idx, double *__restrict__ d2)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ns) return;
    if (layout == 1) {                                     // the matched record: {rx, ry, rz, row}
        const float4 r = reinterpret_cast<const float4 *>(rec)[i];
        double x, y;
        matched_fields(r, q32, 3, nullptr, nullptr, row0 + i, false, x, y);
        if (idx) idx[i] = __float_as_int(r.w);
        d2[i] = x;
        return;
    }
    const double *r = rec + i * stride;
    if (stride == 4 && idx) idx[i] = (int32_t)(__double_as_longlong(r[2]) & 0xffffffffll);      // 16-byte records carry no row
    d2[i] = r[0];
}

int launch_unpack(pccm_ctx *ctx, const double *rec, int stride, int layout, const float4 *q32, int64_t row0, int64_t ns, int32_t *idx, double *d2)
{
    if (ns <= 0) return PCCM_OK;
    PCCM_LAUNCH(ctx, k_unpack, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, ctx->stream, rec, stride, layout, q32, row0, ns, idx, d2);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

}  // namespace pccm
