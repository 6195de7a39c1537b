// Procrustes alignment of one [n][3] point cloud onto another (reference src/experiments/evaluation_utils.py
// calc_procrustes_transform(X = ground truth, Y = prediction)), float64, one sample per call: the numeric core of
// pose_eval.hip.  Plain C++: the same text compiles for the device and, without hipcc, for the host
// (tests/eval_host_main.cpp), so the arithmetic the kernel runs can be checked, and run under a sanitizer, on a CPU.
//
// Steps, in the reference's order:
//   muX, muY             column means                              X0 = X - muX, Y0 = Y - muY
//   normX, normY         Frobenius norms of X0, Y0                 X0 /= normX, Y0 /= normY
//   A = X0^T Y0          3 x 3
//   A = U diag(s) V^T    one-sided (Hestenes) Jacobi: columns of A V are rotated until they are orthogonal; their lengths are
//                        the singular values (sorted, largest first), U's first two columns their directions and
//                        u3 = u1 x u2 (so that a planar cloud, s3 = 0, needs no 0 / 0; s3 = (A v3) . u3 then carries a sign)
//   R = V U^T            if det(R) < 0 the LAST singular pair changes sign: v3 = -v3, s3 = -s3 (torch: V[:, -1] *= sign(det))
//   scale_ratio = sum s  scale = scale_ratio normX / normY         translation = muX - scale (muY R)
//   y_transform = normX scale_ratio (Y0 R) + muX
// Only R, sum s and what follows from them leave this file: they do not depend on the sign and order conventions of the
// decomposition wherever the alignment is unique (rank >= 2).  A collinear cloud (rank 1) gives NaN or an arbitrary
// rotation, as the problem itself does; the sweep count is bounded, so nothing can loop forever.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PECLR_HD __host__ __device__ inline
#else
#define PECLR_HD inline
#endif

// The loops over the joints and the sweeps stay loops: unrolled, the device compiler keeps a whole cloud in registers and spills.
#if defined(__clang__)
#define PECLR_LOOP _Pragma("unroll 1")
#else
#define PECLR_LOOP
#endif

#if defined(__clang__)
#pragma clang fp contract(off)  // products and sums round separately: host and device run the same roundings
#endif

namespace peclr {
namespace procrustes {

constexpr int kJoints = 21;
constexpr int kMaxSweeps = 30;  // a 3 x 3 matrix converges in 4 - 7 sweeps

struct Fit {
    double muX[3], muY[3];
    double normX, normY;
    double R[3][3];      // rot_mat: y_transform rows = Y0 rows times R
    double scale_ratio;  // sum of the (sign-fixed) singular values
    double scale;        // scale_ratio normX / normY
    double t[3];         // translation
};

PECLR_HD void centroid(const double (*P)[3], int n, double mu[3]) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    PECLR_LOOP
    for (int j = 0; j < n; ++j) s0 += P[j][0], s1 += P[j][1], s2 += P[j][2];
    mu[0] = s0 / n, mu[1] = s1 / n, mu[2] = s2 / n;
}

PECLR_HD double centred_norm(const double (*P)[3], int n, const double mu[3]) {
    double s = 0.0;
    PECLR_LOOP
    for (int j = 0; j < n; ++j) {
        const double a = P[j][0] - mu[0], b = P[j][1] - mu[1], c = P[j][2] - mu[2];
        s += a * a;
        s += b * b;
        s += c * c;
    }
    return sqrt(s);
}

// A[i][k] = sum_j X0[j][i] Y0[j][k] of the centred, unit-norm clouds
PECLR_HD void covariance(const double (*X)[3], const double muX[3], double normX, const double (*Y)[3], const double muY[3],
                         double normY, int n, double A[3][3]) {
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a10 = 0.0, a11 = 0.0, a12 = 0.0, a20 = 0.0, a21 = 0.0, a22 = 0.0;
    PECLR_LOOP
    for (int j = 0; j < n; ++j) {
        const double x0 = (X[j][0] - muX[0]) / normX, x1 = (X[j][1] - muX[1]) / normX, x2 = (X[j][2] - muX[2]) / normX;
        const double y0 = (Y[j][0] - muY[0]) / normY, y1 = (Y[j][1] - muY[1]) / normY, y2 = (Y[j][2] - muY[2]) / normY;
        a00 += x0 * y0, a01 += x0 * y1, a02 += x0 * y2;
        a10 += x1 * y0, a11 += x1 * y1, a12 += x1 * y2;
        a20 += x2 * y0, a21 += x2 * y1, a22 += x2 * y2;
    }
    A[0][0] = a00, A[0][1] = a01, A[0][2] = a02;
    A[1][0] = a10, A[1][1] = a11, A[1][2] = a12;
    A[2][0] = a20, A[2][1] = a21, A[2][2] = a22;
}

// One Hestenes rotation of columns (g0, g1) of A V and (v0, v1) of V; returns whether it rotated.
PECLR_HD bool rotate_pair(double g0[3], double g1[3], double v0[3], double v1[3]) {
    const double alpha = g0[0] * g0[0] + g0[1] * g0[1] + g0[2] * g0[2];
    const double beta = g1[0] * g1[0] + g1[1] * g1[1] + g1[2] * g1[2];
    const double gamma = g0[0] * g1[0] + g0[1] * g1[1] + g0[2] * g1[2];
    // orthogonal to working precision (also false for NaN, and for a zero column)
    if (!(gamma * gamma > 1.2e-32 * alpha * beta) || !(fabs(gamma) > 1e-300)) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    for (int i = 0; i < 3; ++i) {
        const double a = g0[i], b = g1[i];
        g0[i] = c * a - s * b;
        g1[i] = s * a + c * b;
        const double p = v0[i], q = v1[i];
        v0[i] = c * p - s * q;
        v1[i] = s * p + c * q;
    }
    return true;
}

PECLR_HD void swap_columns(double a[3], double b[3]) {
    for (int i = 0; i < 3; ++i) {
        const double t = a[i];
        a[i] = b[i];
        b[i] = t;
    }
}

// A = U diag(s) V^T with s[0] >= s[1] >= |s[2]|, det(U) = +1; s[2] may be negative (see the header).  Matrices are held by
// COLUMN: Uc[k] is the k-th left singular vector.
PECLR_HD void svd3(const double A[3][3], double Uc[3][3], double s[3], double Vc[3][3]) {
    double g0[3] = {A[0][0], A[1][0], A[2][0]}, g1[3] = {A[0][1], A[1][1], A[2][1]}, g2[3] = {A[0][2], A[1][2], A[2][2]};
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
    PECLR_LOOP
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        bool any = rotate_pair(g0, g1, v0, v1);
        any = rotate_pair(g0, g2, v0, v2) || any;
        any = rotate_pair(g1, g2, v1, v2) || any;
        if (!any) break;
    }
    double n0 = sqrt(g0[0] * g0[0] + g0[1] * g0[1] + g0[2] * g0[2]);
    double n1 = sqrt(g1[0] * g1[0] + g1[1] * g1[1] + g1[2] * g1[2]);
    double n2 = sqrt(g2[0] * g2[0] + g2[1] * g2[1] + g2[2] * g2[2]);
    // largest first (three compare-and-swaps); a swap of two columns of V changes det(V), which the reflection fix sees
    if (n0 < n1) {
        swap_columns(g0, g1), swap_columns(v0, v1);
        const double t = n0;
        n0 = n1, n1 = t;
    }
    if (n1 < n2) {
        swap_columns(g1, g2), swap_columns(v1, v2);
        const double t = n1;
        n1 = n2, n2 = t;
    }
    if (n0 < n1) {
        swap_columns(g0, g1), swap_columns(v0, v1);
        const double t = n0;
        n0 = n1, n1 = t;
    }
    for (int i = 0; i < 3; ++i) {
        Uc[0][i] = g0[i] / n0;
        Uc[1][i] = g1[i] / n1;
        Vc[0][i] = v0[i], Vc[1][i] = v1[i], Vc[2][i] = v2[i];
    }
    Uc[2][0] = Uc[0][1] * Uc[1][2] - Uc[0][2] * Uc[1][1];
    Uc[2][1] = Uc[0][2] * Uc[1][0] - Uc[0][0] * Uc[1][2];
    Uc[2][2] = Uc[0][0] * Uc[1][1] - Uc[0][1] * Uc[1][0];
    s[0] = n0, s[1] = n1;
    s[2] = g2[0] * Uc[2][0] + g2[1] * Uc[2][1] + g2[2] * Uc[2][2];
}

PECLR_HD double det3(const double M[3][3]) {
    return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

// torch.sign
PECLR_HD double sign_of(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : v); }

// R = V U^T, the reflection fix on the last singular pair, R again; returns sum s
PECLR_HD double rotation_from_svd(const double Uc[3][3], double s[3], double Vc[3][3], double R[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) R[i][k] = Vc[0][i] * Uc[0][k] + Vc[1][i] * Uc[1][k] + Vc[2][i] * Uc[2][k];
    const double sg = sign_of(det3(R));
    for (int i = 0; i < 3; ++i) Vc[2][i] *= sg;
    s[2] *= sg;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) R[i][k] = Vc[0][i] * Uc[0][k] + Vc[1][i] * Uc[1][k] + Vc[2][i] * Uc[2][k];
    return s[0] + s[1] + s[2];
}

// The whole fit of Y onto X.  degenerate (normX or normY zero or not finite): every field the outputs use is NaN, which is
// what the reference's 0 / 0 gives.
PECLR_HD bool fit(const double (*X)[3], const double (*Y)[3], int n, Fit& f) {
    centroid(X, n, f.muX);
    centroid(Y, n, f.muY);
    f.normX = centred_norm(X, n, f.muX);
    f.normY = centred_norm(Y, n, f.muY);
    const bool ok = f.normX > 0.0 && f.normX < INFINITY && f.normY > 0.0 && f.normY < INFINITY;
    if (!ok) {
        const double nan = NAN;
        for (int i = 0; i < 3; ++i) {
            f.R[i][0] = f.R[i][1] = f.R[i][2] = nan;
            f.t[i] = nan;
        }
        f.scale_ratio = f.scale = nan;
        return false;
    }
    double A[3][3], Uc[3][3], Vc[3][3], s[3];
    covariance(X, f.muX, f.normX, Y, f.muY, f.normY, n, A);
    svd3(A, Uc, s, Vc);
    f.scale_ratio = rotation_from_svd(Uc, s, Vc, f.R);
    f.scale = f.scale_ratio * f.normX / f.normY;
    for (int k = 0; k < 3; ++k)
        f.t[k] = f.muX[k] - f.scale * (f.muY[0] * f.R[0][k] + f.muY[1] * f.R[1][k] + f.muY[2] * f.R[2][k]);
    return true;
}

// one row of y_transform
PECLR_HD void transform_point(const Fit& f, const double y[3], double out[3]) {
    const double y0 = (y[0] - f.muY[0]) / f.normY, y1 = (y[1] - f.muY[1]) / f.normY, y2 = (y[2] - f.muY[2]) / f.normY;
    const double k = f.normX * f.scale_ratio;
    for (int c = 0; c < 3; ++c) out[c] = k * (y0 * f.R[0][c] + y1 * f.R[1][c] + y2 * f.R[2][c]) + f.muX[c];
}

PECLR_HD void transform_cloud(const Fit& f, const double (*Y)[3], int n, double (*out)[3]) {
    for (int j = 0; j < n; ++j) transform_point(f, Y[j], out[j]);
}

// sqrt(sum_{c < dim} (p[c] - g[c])^2): calculate_epe_statistics' eucledian_dist for one joint
PECLR_HD double joint_distance(const double p[3], const double g[3], int dim) {
    const double d0 = p[0] - g[0], d1 = p[1] - g[1], d2 = p[2] - g[2];
    double s = d0 * d0;
    s += d1 * d1;
    if (dim > 2) s += d2 * d2;
    return sqrt(s);
}

}  // namespace procrustes
}  // namespace peclr
