// The k-NN searches that normal estimation, the PointSSIM features and the point-to-distribution columns share (pccm_knn.hip):
// what their kernels and the kernels that read their neighbour lists have in common, and the host side of the chain.
#pragma once
#include "pccm_internal.h"

namespace pccm {

constexpr int kKnnMax = 64;        // largest supported k
constexpr int kKnnMaxRing = 6;     // rings the per-thread search opens before it leaves a point to the full scan
constexpr int kWCap = 512;         // candidates a wave stages in LDS; a point with more goes to the per-thread search

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

// The stop rule of the grid engine for the cube [c-r, c+r]^3 around the query's cell: the distance L from the query to the nearest
// face of the cube that is not a face of the grid, less the slack; INFINITY when the cube covers the grid.  A search is settled
// when its k-th best squared distance is below L * L * (1 - 2^-30), L > 0.
__device__ __forceinline__ double knn_stop_bound(const KnnGeom &g, double qx, double qy, double qz, int cx, int cy, int cz, int r)
{
    double L = INFINITY;
    const double q[3] = {qx, qy, qz};
    const int c[3] = {cx, cy, cz};
    for (int a = 0; a < 3; ++a) {
        if (c[a] - r > 0) L = fmin(L, (q[a] - (g.org[a] + (double)(c[a] - r) * g.h[a])) - g.slack[a]);
        if (c[a] + r < g.dim[a] - 1) L = fmin(L, ((g.org[a] + (double)(c[a] + r + 1) * g.h[a]) - q[a]) - g.slack[a]);
    }
    return L;
}

// the grid the k-NN searches of cloud `which` run on, its cell starts and records (shared by estimate_normals, ssim_features and
// the point-to-distribution search).  `qrecs` (the search across the clouds): the OTHER cloud's cell-sorted records when both
// clouds sit in the pair's grid -- queries taken in that order walk the same cells wave after wave -- or null when `which` has
// cells of its own, which only sort `which`
int knn_setup(pccm_ctx *ctx, int which, KnnGeom &g, const uint32_t *&cs, const GridRec *&crecs, const GridRec **qrecs = nullptr);
// scratch of the three searches: covariances + counts (ctx->val), points handed on (g_rank, g_cell_of) and their counters
int knn_scratch(pccm_ctx *ctx, int64_t n, double **cov, int32_t **cnt, uint32_t **open_count, uint32_t **todo_count);

// Where a search's results go, by query row: the normals [nq][3] (the queries are then the searched cloud's own points), or the
// neighbour lists nbr[nq][k] in ascending (d2, row) order with their counts in the scratch's cnt[nq].  One of the two is null.
struct KnnSink {
    double *nrm;
    int32_t *nbr;
};
// the chain wave -> per-thread -> full scan on the stream: for each of the nq queries (qrecs / qx64: query_at; q64: their cloud's
// rows, which the full scan reads) its k nearest points of the searched cloud (crecs, cs, s64, ns points), into `sink`
void launch_knn(pccm_ctx *ctx, const GridRec *crecs, const uint32_t *cs, const KnnGeom &g, const double *s64, int64_t ns,
                const GridRec *qrecs, const double *qx64, const double *q64, int64_t nq, int k, double *cov, int32_t *cnt,
                uint32_t *open_count, uint32_t *todo_count, KnnSink sink);

}  // namespace pccm
