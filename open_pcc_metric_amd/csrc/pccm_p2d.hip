// Point-to-distribution (pccm_p2d_build, INTEGRATION.md "Point-to-distribution"): the k-NN searches of pccm_knn.hip ACROSS the
// clouds, in neighbour-list mode, then the Mahalanobis distance of every query to its neighbours' distribution (k_p2d_geometry)
// and, with PCCM_P2D_COLOR, the colour and joint columns (k_p2d_color), all from the neighbour lists.
#include "pccm_knn.h"
#include "pccm_stale.h"

namespace pccm {

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

// p2d_value of every query i (row i of q64) -> out[n], from its neighbour list nbr[n][k] of rows of x64 (cnt[i] entries)
__global__ __launch_bounds__(256) void k_p2d_geometry(const double *__restrict__ x64, const double *__restrict__ q64,
                                                      const int32_t *__restrict__ nbr, const int32_t *__restrict__ cnt, int k, int64_t n,
                                                      double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = p2d_value(x64, q64, i, nbr + i * k, cnt[i]);
}

// p2d_color_value M_Y of every query i -> color[n] and the joint value sqrt(M_G * M_G + M_Y * M_Y) -> joint[n], M_G = geometry[i]
// (the column k_p2d_geometry wrote), from the same neighbour list; the searched cloud's colours are s8 (packed bytes) or else
// srgb64, the queries' q8 or else qrgb64
__global__ __launch_bounds__(256) void k_p2d_color(const uint32_t *__restrict__ s8, const double *__restrict__ srgb64,
                                                   const uint32_t *__restrict__ q8, const double *__restrict__ qrgb64,
                                                   const double *__restrict__ geometry, const int32_t *__restrict__ nbr,
                                                   const int32_t *__restrict__ cnt, int k, int64_t n, double *__restrict__ color,
                                                   double *__restrict__ joint)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double my = p2d_color_value(s8, srgb64, q8, qrgb64, i, nbr + i * k, cnt[i]);
    const double mg = geometry[i];
    color[i] = my;
    joint[i] = __dsqrt_rn(__dadd_rn(__dmul_rn(mg, mg), __dmul_rn(my, my)));
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
    launch_knn(ctx, crecs, cs, g, b.xyz64, b.n, qrecs, a.xyz64, a.xyz64, a.n, k, cov, cnt, open_count, todo_count,
               KnnSink{nullptr, nbr});
    PCCM_HIP(hipGetLastError());
    *nbr_out = nbr;
    *cnt_out = cnt;
    return PCCM_OK;
}

// pccm_p2d_build_attrs has checked k, attrs, the clouds (and their colours) and the context's state.  One k-NN search per
// direction serves every column that is missing: the geometry column (k_p2d_geometry) and, with PCCM_P2D_COLOR, the colour and
// joint columns (k_p2d_color, which reads the geometry column back) are formed from the same neighbour lists while they are in HBM.
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
    column_rebuild(ctx, geometry ? Stored::kP2d : Stored::kP2dColor);
    for (int d = 0; d < 2; ++d) {
        const Cloud &a = ctx->cloud[d], &b = ctx->cloud[1 - d];
        PCCM_HIP(hipStreamSynchronize(ctx->stream));
        double **cols[3] = {&ctx->p2d64[d], &ctx->p2d_cj64[d][0], &ctx->p2d_cj64[d][1]};
        size_t *caps[3] = {&ctx->cap_p2d[d], &ctx->cap_p2d_cj[d][0], &ctx->cap_p2d_cj[d][1]};
        for (int c = 0; c < 3; ++c) {
            if (!(c == 0 ? geometry : color)) continue;
            const double *before = *cols[c];
            if ((rc = grow((void **)cols[c], *caps[c], (size_t)a.n * sizeof(double)))) return rc;
            if (*cols[c] != before) column_moved(ctx);
        }
        int32_t *nbr, *cnt;
        if ((rc = p2d_search(ctx, d, k, &nbr, &cnt))) return rc;
        const dim3 pgrid((unsigned)((a.n + 255) / 256));
        if (geometry)
            PCCM_LAUNCH(ctx, k_p2d_geometry, pgrid, dim3(256), 0, ctx->stream, (const double *)b.xyz64, (const double *)a.xyz64,
                               (const int32_t *)nbr, (const int32_t *)cnt, k, a.n, ctx->p2d64[d]);
        if (color)
            PCCM_LAUNCH(ctx, k_p2d_color, pgrid, dim3(256), 0, ctx->stream, (const uint32_t *)(b.rgb8_valid ? b.rgb8 : nullptr),
                               (const double *)b.rgb64, (const uint32_t *)(a.rgb8_valid ? a.rgb8 : nullptr), (const double *)a.rgb64,
                               (const double *)ctx->p2d64[d], (const int32_t *)nbr, (const int32_t *)cnt, k, a.n,
                               ctx->p2d_cj64[d][0], ctx->p2d_cj64[d][1]);
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
