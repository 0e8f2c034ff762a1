// Normals from neighbourhoods: the covariance of a point's neighbours and the eigenvector of its smallest eigenvalue (device code
// shared by the searches that settle a normal themselves, pccm_knn.hip, and by k_normals_from_cov, pccm_normals.hip).
#pragma once
#include "pccm_internal.h"

namespace pccm {

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
__device__ inline void smallest_eigenvector(double a00, double a01, double a02, double a11, double a12, double a22, double n[3])
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

// covariance E[d d^T] - E[d] E[d]^T of d = x64[row[j]] - q over the cnt neighbours `row` (cnt >= 1), the raw moments summed left to
// right in the order of `row` -> a = {a00, a01, a02, a11, a12, a22}
__device__ __forceinline__ void neighbour_covariance(const double *__restrict__ x64, double qx, double qy, double qz, const int *row,
                                                     int cnt, double a[6])
{
    double m0 = 0, m1 = 0, m2 = 0, s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0;
    for (int k = 0; k < cnt; ++k) {
        const double *p = x64 + 3 * (int64_t)row[k];
        const double dx = p[0] - qx, dy = p[1] - qy, dz = p[2] - qz;
        m0 += dx; m1 += dy; m2 += dz;
        s00 += dx * dx; s01 += dx * dy; s02 += dx * dz; s11 += dy * dy; s12 += dy * dz; s22 += dz * dz;
    }
    const double inv = 1.0 / (double)cnt;
    m0 *= inv; m1 *= inv; m2 *= inv;
    a[0] = s00 * inv - m0 * m0; a[1] = s01 * inv - m0 * m1; a[2] = s02 * inv - m0 * m2;
    a[3] = s11 * inv - m1 * m1; a[4] = s12 * inv - m1 * m2; a[5] = s22 * inv - m2 * m2;
}

// k_normals_from_cov on the stream: the normals of the n points whose covariance the wave search left in cov[n][6] (cnt[i] >= 0)
void launch_normals_from_cov(pccm_ctx *ctx, const double *cov, const int32_t *cnt, int64_t n, double *nrm);

}  // namespace pccm
