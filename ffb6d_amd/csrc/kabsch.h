// ffb6d_amd/csrc/kabsch.h -- the reflection-corrected least-squares rotation of best_fit_transform
// (ffb6d/utils/pvn3d_eval_utils_kpls.py:28-61) from a 3x3 cross-covariance, in double, one thread per problem.
// Shared by the keypoint fit (csrc/pose.hip) and the ICP refinement (csrc/icp.hip): one body, the same bits in both.
//
// The singular vectors come from a cyclic one-sided (Hestenes) Jacobi on H itself, never from H^T H: forming H^T H squares the
// singular values, and once (s2 / s1)^2 nears 2^-53 the second and third right singular vectors mix freely (thin, planar and
// rod-like point sets).  The one-sided form is backward stable in H: the rotation it returns is that of some H + dH with
// |dH| ~ 2^-53 s1, i.e. within a few 2^-53 * cond of the exact one, cond = s1 / (s2 + d s3), d = sign det H
// (tests/test_rigid_fit_cpu.py holds it to ten times what LAPACK's float64 SVD itself reaches against extended precision).
#pragma once
#include <hip/hip_runtime.h>

namespace ffb6d {

// G = H V with mutually orthogonal columns, V orthogonal: g holds H on entry and U S on exit (columns in no particular order).
// A pair of columns is rotated while |g_p . g_q| > 1.5 * 2^-52 |g_p| |g_q|; the comparison is false for NaN and for a zero column,
// and the number of sweeps is bounded, so no input can spin.
__device__ inline void jacobi_svd3(double g[3][3], double v[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = i == j;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int k = 0; k < 3; ++k) {
                    alpha += g[k][p] * g[k][p];
                    beta += g[k][q] * g[k][q];
                    gamma += g[k][p] * g[k][q];
                }
                if (!(fabs(gamma) > 0x1.8p-52 * (sqrt(alpha) * sqrt(beta)))) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
                const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
                for (int k = 0; k < 3; ++k) {      // G <- G J
                    const double gkp = g[k][p], gkq = g[k][q];
                    g[k][p] = cs * gkp - sn * gkq;
                    g[k][q] = sn * gkp + cs * gkq;
                }
                for (int k = 0; k < 3; ++k) {      // V <- V J
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = cs * vkp - sn * vkq;
                    v[k][q] = sn * vkp + cs * vkq;
                }
            }
        if (!rotated) break;
    }
}

__device__ inline void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ inline double normalize3(double* a) {
    const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (n > 0) {
        a[0] /= n;
        a[1] /= n;
        a[2] /= n;
    }
    return n;
}

// any unit vector orthogonal to u
__device__ inline void any_orthogonal(const double* u, double* o) {
    const int k = fabs(u[0]) <= fabs(u[1]) ? (fabs(u[0]) <= fabs(u[2]) ? 0 : 2) : (fabs(u[1]) <= fabs(u[2]) ? 1 : 2);
    double e[3] = {0, 0, 0};
    e[k] = 1;
    cross3(u, e, o);
    normalize3(o);
}

// [R|t] (row-major double [3,4]) from H = sum (a_i - ca)(b_i - cb)^T and the two centroids: R minimises sum |R (a_i - ca) - (b_i - cb)|^2
// over the rotations, t = cb - R ca
__device__ inline void kabsch_from_covariance(const double H[3][3], const double ca[3], const double cb[3], double* out) {
    // H = U S V^T: one-sided Jacobi gives V and G = H V = U S; s_k = |g_k|, u_k = g_k / s_k
    double G[3][3], V[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) G[r][c] = H[r][c];
    jacobi_svd3(G, V);
    double n2[3];
    for (int c = 0; c < 3; ++c) n2[c] = G[0][c] * G[0][c] + G[1][c] * G[1][c] + G[2][c] * G[2][c];
    int order[3] = {0, 1, 2};
    for (int i = 0; i < 2; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (n2[order[j]] > n2[order[i]]) {
                const int tmp = order[i];
                order[i] = order[j];
                order[j] = tmp;
            }
    double v[3][3], u[3][3];                   // rows = singular vectors, largest first
    for (int k = 0; k < 3; ++k)
        for (int r = 0; r < 3; ++r) v[k][r] = V[r][order[k]];
    for (int k = 0; k < 2; ++k)
        for (int r = 0; r < 3; ++r) u[k][r] = G[r][order[k]];
    const double s1 = normalize3(u[0]);
    if (!(s1 > 0)) {                           // H = 0: any rotation is optimal, return the identity
        u[0][0] = v[0][0] = 1; u[0][1] = u[0][2] = v[0][1] = v[0][2] = 0;
        u[1][1] = v[1][1] = 1; u[1][0] = u[1][2] = v[1][0] = v[1][2] = 0;
    } else {
        // rank 1: the plane is free.  A second column below 2^-60 s1 is rounding residue of the rotations (they leave ~2^-53 s1)
        // and says nothing about u2; choosing u2 freely then costs at most 2 s2 <= 2^-59 s1 of the objective
        const double s2 = normalize3(u[1]);
        const double proj = u[1][0] * u[0][0] + u[1][1] * u[0][1] + u[1][2] * u[0][2];
        for (int r = 0; r < 3; ++r) u[1][r] -= proj * u[0][r];
        const double rest = normalize3(u[1]);
        if (!(s2 > 0x1p-60 * s1) || !(rest > 0.5)) any_orthogonal(u[0], u[1]);
    }
    // third pair by right-handedness on both sides == the reference's det(R) < 0 correction (:53-56):
    // R = V diag(1, 1, det(V U^T)) U^T does not depend on the sign choice of u3 / v3
    cross3(u[0], u[1], u[2]);
    cross3(v[0], v[1], v[2]);
    double R[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r][c] = v[0][r] * u[0][c] + v[1][r] * u[1][c] + v[2][r] * u[2][c];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[4 * r + c] = R[r][c];
        out[4 * r + 3] = cb[r] - (R[r][0] * ca[0] + R[r][1] * ca[1] + R[r][2] * ca[2]);
    }
}

}  // namespace ffb6d
