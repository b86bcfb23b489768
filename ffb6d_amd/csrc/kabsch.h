// ffb6d_amd/csrc/kabsch.h -- the reflection-corrected least-squares rotation of best_fit_transform
// (ffb6d/utils/pvn3d_eval_utils_kpls.py:28-61) from a 3x3 cross-covariance, in double, one thread per problem.
// Shared by the keypoint fit (csrc/pose.hip) and the ICP refinement (csrc/icp.hip): one body, the same bits in both.
#pragma once
#include <hip/hip_runtime.h>

namespace ffb6d {

__device__ inline void jacobi_eigen3(double a[3][3], double v[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = i == j;
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
        if (off < 1e-300) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (fabs(a[p][q]) < 1e-300) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
                for (int k = 0; k < 3; ++k) {      // A <- A J
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = cs * akp - sn * akq;
                    a[k][q] = sn * akp + cs * akq;
                }
                for (int k = 0; k < 3; ++k) {      // A <- J^T A
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = cs * apk - sn * aqk;
                    a[q][k] = sn * apk + cs * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = cs * vkp - sn * vkq;
                    v[k][q] = sn * vkp + cs * vkq;
                }
            }
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
    // H = U S V^T: eigenvectors of H^T H give V; u_k = H v_k / s_k
    double M[3][3], V[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) M[r][c] = H[0][r] * H[0][c] + H[1][r] * H[1][c] + H[2][r] * H[2][c];
    jacobi_eigen3(M, V);
    int order[3] = {0, 1, 2};
    for (int i = 0; i < 2; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (M[order[j]][order[j]] > M[order[i]][order[i]]) {
                const int tmp = order[i];
                order[i] = order[j];
                order[j] = tmp;
            }
    double v[3][3], u[3][3];                   // rows = singular vectors, largest first
    for (int k = 0; k < 3; ++k)
        for (int r = 0; r < 3; ++r) v[k][r] = V[r][order[k]];
    for (int k = 0; k < 2; ++k)
        for (int r = 0; r < 3; ++r) u[k][r] = H[r][0] * v[k][0] + H[r][1] * v[k][1] + H[r][2] * v[k][2];
    const double s1 = normalize3(u[0]);
    if (!(s1 > 0)) {                           // H = 0: any rotation is optimal, return the identity
        u[0][0] = v[0][0] = 1; u[0][1] = u[0][2] = v[0][1] = v[0][2] = 0;
        u[1][1] = v[1][1] = 1; u[1][0] = u[1][2] = v[1][0] = v[1][2] = 0;
    } else {
        const double proj = u[1][0] * u[0][0] + u[1][1] * u[0][1] + u[1][2] * u[0][2];
        for (int r = 0; r < 3; ++r) u[1][r] -= proj * u[0][r];
        const double s2 = normalize3(u[1]);
        if (!(s2 > 1e-12 * s1)) any_orthogonal(u[0], u[1]);   // rank 1: the plane is free
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
