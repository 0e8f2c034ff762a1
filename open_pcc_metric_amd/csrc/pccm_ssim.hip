// PointSSIM features (pccm_ssim_features, INTEGRATION.md "PointSSIM"): the k-NN searches of pccm_knn.hip in neighbour-list mode
// (every point's k rows in ascending (d2, row) order and their count), then the curvature of every point (k_ssim_curvature) and
// the features (k_ssim_features), both from the neighbour lists -- the covariance behind a curvature is summed in neighbourhood
// order, not in the search's order (which follows the grid, and so the other cloud of the pair), so that a cloud's features do not
// depend on the pair it is in.
#include "pccm_knn.h"
#include "pccm_normals.h"
#include "pccm_stale.h"

namespace pccm {

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
    double a[6];
    neighbour_covariance(x64, x64[3 * p], x64[3 * p + 1], x64[3 * p + 2], row, cnt, a);
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

// curvature of every point -> curv[n], from the neighbour lists nbr[n][k] (cnt[i] entries)
__global__ __launch_bounds__(256) void k_ssim_curvature(const double *__restrict__ x64, const int32_t *__restrict__ nbr,
                                                        const int32_t *__restrict__ cnt, int k, int64_t n, double *__restrict__ curv)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    curv[i] = curvature_of(x64, i, nbr + i * k, cnt[i]);
}

// the features of the attributes in `attrs` -> feat[a][n], from the neighbour lists nbr[n][k] (cnt[i] entries):
//   m values v_j over N_k(p), mu = (sum v_j) / m, F = (sum (v_j - mu)^2) / (m - 1), F = 0 for m < 2; left-to-right sums, every
//   operation separately rounded.  Geometry and normal skip q_0 (the point itself).  The values are formed twice (two passes)
//   instead of being kept: up to 64 of them per thread would live in scratch memory.
// kSsimSpacing in `attrs` (resolution_build; no PointSSIM attribute beside it): the point's spacing instead -- the MEAN of the
//   geometry values, r = (sum_{j >= 1} sqrt(d2(p, q_j))) / (c - 1) in one pass, 0 for c < 2 -- into feat[n] (include/pccm.h,
//   pccm_resolution_build).
constexpr int kSsimSpacing = 16;
__global__ __launch_bounds__(256) void k_ssim_features(const double *__restrict__ x64, const double *__restrict__ nrm64,
                                                       const double *__restrict__ rgb64, const double *__restrict__ curv,
                                                       const int32_t *__restrict__ nbr, const int32_t *__restrict__ cnt, int k, int64_t n,
                                                       int attrs, double *__restrict__ feat)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t *row = nbr + i * k;
    const int c = cnt[i];
    if (attrs & kSsimSpacing) {
        double r = 0.0;
        if (c >= 2) {
            double sum = 0.0;
            for (int j = 1; j < c; ++j) sum = __dadd_rn(sum, ssim_value(0, i, row[j], x64, nrm64, curv, rgb64));
            r = __ddiv_rn(sum, (double)(c - 1));
        }
        feat[i] = r;
        return;
    }
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
}

// PointSSIM features of cloud `which` (pccm_ssim_features has checked k, the mask and the inputs it needs).  The same three
// searches as estimate_normals, in neighbour-list mode (every point's k rows in (d2, row) order and their count), then
// k_ssim_curvature and k_ssim_features.  Neighbour lists and curvatures are scratch: 4 k + 8 bytes per point.
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
    column_rebuild(ctx, Stored::kSsim, which);
    if (c.ssim64 != ssim_before) column_moved(ctx);
    double *cov;
    int32_t *cnt;
    uint32_t *open_count, *todo_count;
    if ((rc = knn_scratch(ctx, c.n, &cov, &cnt, &open_count, &todo_count))) return rc;
    const size_t nbr_words = ((size_t)c.n * k + 1) & ~(size_t)1;          // (the curvatures behind them stay 8-byte aligned)
    if ((rc = ensure(ctx, ctx->ssim_scratch, nbr_words * sizeof(int32_t) + (size_t)c.n * sizeof(double)))) return rc;
    int32_t *nbr = (int32_t *)ctx->ssim_scratch.p;
    double *curv = (double *)(nbr + nbr_words);
    const dim3 pgrid((unsigned)((c.n + 255) / 256));
    launch_knn(ctx, crecs, cs, g, c.xyz64, c.n, crecs, nullptr, c.xyz64, c.n, k, cov, cnt, open_count, todo_count,
               KnnSink{nullptr, nbr});
    if (attrs & PCCM_SSIM_CURVATURE)
        PCCM_LAUNCH(ctx, k_ssim_curvature, pgrid, dim3(256), 0, ctx->stream, (const double *)c.xyz64, (const int32_t *)nbr,
                           (const int32_t *)cnt, k, c.n, curv);
    // one launch per attribute: at 1M points and k = 12 the four attributes take 2.25 ms in one launch, 1.99 ms in four
    for (int a = 0; a < 4; ++a)
        if (attrs & (1 << a))
            PCCM_LAUNCH(ctx, k_ssim_features, pgrid, dim3(256), 0, ctx->stream, (const double *)c.xyz64,
                               (const double *)((attrs & PCCM_SSIM_NORMAL) ? c.nrm64 : nullptr),
                               (const double *)((attrs & PCCM_SSIM_COLOR) ? c.rgb64 : nullptr), (const double *)curv,
                               (const int32_t *)nbr, (const int32_t *)cnt, k, c.n, 1 << a, c.ssim64);
    PCCM_HIP(hipGetLastError());
    c.ssim_k = k;
    c.ssim_attrs = attrs;
    if (built) *built = 1;
    return PCCM_OK;
}

// Point spacings of cloud `which` (pccm_resolution_build has checked K, the cloud and the shard).  The searches of ssim_features
// at k = K + 1 in neighbour-list mode, then k_ssim_features' spacing branch on the lists.  The lists are scratch: 4 (K + 1) bytes
// per point.
int resolution_build(pccm_ctx *ctx, int which, int K, int *built)
{
    Cloud &c = ctx->cloud[which];
    if (built) *built = 0;
    if (c.res_k == K) return PCCM_OK;
    if (ctx->capturing) {
        ctx->capture_failed = true;
        return fail(PCCM_E_STATE, "point spacings are built before graph capture");
    }
    const int k = K + 1;
    int rc;
    KnnGeom g;
    const uint32_t *cs;
    const GridRec *crecs;
    if ((rc = knn_setup(ctx, which, g, cs, crecs))) return rc;
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    const double *before = c.res64;
    if ((rc = grow((void **)&c.res64, c.cap_res, (size_t)c.n * sizeof(double)))) return rc;
    column_rebuild(ctx, Stored::kSpacing, which);
    if (c.res64 != before) column_moved(ctx);
    double *cov;
    int32_t *cnt;
    uint32_t *open_count, *todo_count;
    if ((rc = knn_scratch(ctx, c.n, &cov, &cnt, &open_count, &todo_count))) return rc;
    if ((rc = ensure(ctx, ctx->ssim_scratch, (size_t)c.n * k * sizeof(int32_t)))) return rc;
    int32_t *nbr = (int32_t *)ctx->ssim_scratch.p;
    launch_knn(ctx, crecs, cs, g, c.xyz64, c.n, crecs, nullptr, c.xyz64, c.n, k, cov, cnt, open_count, todo_count,
               KnnSink{nullptr, nbr});
    PCCM_LAUNCH(ctx, k_ssim_features, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)c.xyz64,
                       (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, (const int32_t *)nbr,
                       (const int32_t *)cnt, k, c.n, kSsimSpacing, c.res64);
    PCCM_HIP(hipGetLastError());
    c.res_k = K;
    if (built) *built = 1;
    return PCCM_OK;
}

}  // namespace pccm
