// What labels.hip (the label side of a supervised sample) and pose_loss.hip (the supervised losses) share: the wave layout --
// one wave per sample, LS samples per workgroup, lane j < 21 owns joint j -- and the float64 pieces of the reference's
// convert_2_5D_to_3D (src/data_loader/utils.py: get_root_depth, get_zroot_constraint_terms).  The operation order of every
// function here is the reference's, and contraction is off from here to the end of the including file: a product and a sum
// are two roundings in both files, so the two agree to the last bit.
#pragma once
#include "common.hpp"

#pragma clang fp contract(off)

namespace peclr {
namespace {

constexpr int LS = 4;  // samples (waves) per workgroup
constexpr int LT = LS * kWave;
constexpr int LJ = 21;
constexpr int kParent = 0, kChild = 2;  // wrist, index MCP (reference data_loader/utils.py:15-16)

__device__ __forceinline__ void load3(const float* __restrict__ p, double out[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (double)p[c];
}
__device__ __forceinline__ void load9(const float* __restrict__ p, double out[9]) {
#pragma unroll
    for (int c = 0; c < 9; ++c) out[c] = (double)p[c];
}
// torch.clamp(x, min = lo): a NaN stays a NaN
__device__ __forceinline__ double clamp_min(double x, double lo) { return x < lo ? lo : x; }

// torch.inverse(K) for a general 3 x 3 matrix: adjugate over determinant
__device__ __forceinline__ void inverse3(const double K[9], double inv[9]) {
    const double c0 = K[4] * K[8] - K[5] * K[7], c1 = K[3] * K[8] - K[5] * K[6], c2 = K[3] * K[7] - K[4] * K[6];
    const double det = K[0] * c0 - K[1] * c1 + K[2] * c2;
    inv[0] = c0 / det;
    inv[1] = (K[2] * K[7] - K[1] * K[8]) / det;
    inv[2] = (K[1] * K[5] - K[2] * K[4]) / det;
    inv[3] = (K[5] * K[6] - K[3] * K[8]) / det;
    inv[4] = (K[0] * K[8] - K[2] * K[6]) / det;
    inv[5] = (K[2] * K[3] - K[0] * K[5]) / det;
    inv[6] = c2 / det;
    inv[7] = (K[1] * K[6] - K[0] * K[7]) / det;
    inv[8] = (K[0] * K[4] - K[1] * K[3]) / det;
}
// get_root_depth with get_zroot_constraint_terms: n the 2.5D wrist, m the 2.5D index MCP, C = 1
__device__ __forceinline__ double root_depth(const double inv[9], const double n[3], const double m[3]) {
    const double xn = inv[0] * n[0] + inv[1] * n[1] + inv[2], yn = inv[3] * n[0] + inv[4] * n[1] + inv[5];
    const double xm = inv[0] * m[0] + inv[1] * m[1] + inv[2], ym = inv[3] * m[0] + inv[4] * m[1] + inv[5];
    const double zn = n[2], zm = m[2];
    const double a = (xn - xm) * (xn - xm) + (yn - ym) * (yn - ym);
    const double b = 2.0 * (zn * (xn * xn + yn * yn - xn * xm - yn * ym) + zm * (xm * xm + ym * ym - xn * xm - yn * ym));
    const double c = (xn * zn - xm * zm) * (xn * zn - xm * zm) + (yn * zn - ym * zm) * (yn * zn - ym * zm) +
                     (zn - zm) * (zn - zm) - 1.0;
    return 0.5 * (-b + sqrt(clamp_min(b * b - 4.0 * a * c, 1e-6))) / clamp_min(a, 1e-6);
}
// convert_2_5D_to_3D for one joint
__device__ __forceinline__ void to_3d(const double inv[9], const double p[3], double z_root, double scale, double out[3]) {
    const double z = (p[2] + z_root) * scale;
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = (inv[3 * r] * p[0] + inv[3 * r + 1] * p[1] + inv[3 * r + 2]) * z;
}

inline int grid_of(int B) { return (B + LS - 1) / LS; }

}  // namespace
}  // namespace peclr
