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
// The neighbours come from the shared k-NN searches (pccm_knn.hip); the eigen code is pccm_normals.h's.
#include "pccm_knn.h"
#include "pccm_normals.h"
#include "pccm_stale.h"

namespace pccm {

// normals from the covariances the wave search left (the per-thread kernels write their own: cnt < 0)
__global__ __launch_bounds__(256) void k_normals_from_cov(const double *__restrict__ cov, const int32_t *__restrict__ cnt, int64_t n,
                                                          double *__restrict__ nrm_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = cnt[i];
    if (c < 0) return;                                               // settled by the per-thread kernel
    double nn[3] = {0.0, 0.0, 1.0};
    const double *a = cov + 6 * i;
    if (c >= 3) smallest_eigenvector(a[0], a[1], a[2], a[3], a[4], a[5], nn);
    nrm_out[3 * i] = nn[0];
    nrm_out[3 * i + 1] = nn[1];
    nrm_out[3 * i + 2] = nn[2];
}

void launch_normals_from_cov(pccm_ctx *ctx, const double *cov, const int32_t *cnt, int64_t n, double *nrm)
{
    PCCM_LAUNCH(ctx, k_normals_from_cov, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, cov, cnt, n, nrm);
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
    normals_changed(ctx, which);
    c.n_nrm = c.n;
    double *cov;
    int32_t *cnt;
    uint32_t *open_count, *todo_count;
    if ((rc = knn_scratch(ctx, c.n, &cov, &cnt, &open_count, &todo_count))) return rc;
    launch_knn(ctx, crecs, cs, g, c.xyz64, c.n, crecs, nullptr, c.xyz64, c.n, k, cov, cnt, open_count, todo_count,
               KnnSink{c.nrm64, nullptr});
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

}  // namespace pccm
