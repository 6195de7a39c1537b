// Device code the evaluation head (pose.hip) and the training head (pose_train.hip) of the 2.5D pose model share: the fc
// stage on four samples per workgroup, K^-1 and the closed-form root depth.  Both heads round these stages alike.
#pragma once
#include "common.hpp"

#pragma clang fp contract(off)  // products and sums round separately, as the host restatements do

namespace peclr {
namespace pose_head {

constexpr int HS = 4;          // samples per workgroup: one wave each for the per-sample stages
constexpr int HT = HS * kWave;
constexpr int NF = 2048, NO = 64, NH = 128, NJ = 21;
constexpr int FC_PER_WAVE = NO / HS;  // fc outputs per wave
constexpr int KV = NF / (4 * kWave);  // float4 loads per lane per feature row

__device__ __forceinline__ float max_nan(float eps, float v) { return v != v ? v : (v > eps ? v : eps); }  // torch.max: NaN wins
__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : v * 0.01f; }

// fc of samples [b0, b0 + HS) into fc[HS][NO] (LDS): wave w owns outputs [16 w, 16 w + 16); lane l holds features
// 4 l + 256 j (j < 8) of every sample in registers.  The caller synchronises afterwards.
__device__ __forceinline__ void fc_stage(const float* __restrict__ feat, int B, int b0, const float* __restrict__ fc_w,
                                         const float* __restrict__ fc_b, float (*fc)[NO], int wave, int lane) {
    float4 f[HS][KV];
#pragma unroll
    for (int s = 0; s < HS; ++s) {
        const bool ok = b0 + s < B;
        const float4* row = reinterpret_cast<const float4*>(feat + (size_t)(ok ? b0 + s : 0) * NF);
#pragma unroll
        for (int j = 0; j < KV; ++j) f[s][j] = ok ? row[lane + kWave * j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int oo = 0; oo < FC_PER_WAVE; ++oo) {
        const int o = wave * FC_PER_WAVE + oo;
        const float4* wr = reinterpret_cast<const float4*>(fc_w + (size_t)o * NF);
        float acc[HS] = {};
#pragma unroll
        for (int j = 0; j < KV; ++j) {
            const float4 w = wr[lane + kWave * j];
#pragma unroll
            for (int s = 0; s < HS; ++s) {
                acc[s] = fmaf(w.x, f[s][j].x, acc[s]);
                acc[s] = fmaf(w.y, f[s][j].y, acc[s]);
                acc[s] = fmaf(w.z, f[s][j].z, acc[s]);
                acc[s] = fmaf(w.w, f[s][j].w, acc[s]);
            }
        }
#pragma unroll
        for (int s = 0; s < HS; ++s) {
            const float v = wave_sum(acc[s]);
            if (lane == 0) fc[s][o] = v + fc_b[o];
        }
    }
}

// K^-1 by the adjugate in float64, rounded to float32
__device__ __forceinline__ void k_inverse(const float* __restrict__ kk, float* ki) {
    double k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = kk[i];
    const double c00 = k[4] * k[8] - k[5] * k[7], c01 = k[5] * k[6] - k[3] * k[8], c02 = k[3] * k[7] - k[4] * k[6];
    const double det = k[0] * c00 + k[1] * c01 + k[2] * c02;
    ki[0] = (float)(c00 / det), ki[1] = (float)((k[2] * k[7] - k[1] * k[8]) / det), ki[2] = (float)((k[1] * k[5] - k[2] * k[4]) / det);
    ki[3] = (float)(c01 / det), ki[4] = (float)((k[0] * k[8] - k[2] * k[6]) / det), ki[5] = (float)((k[2] * k[3] - k[0] * k[5]) / det);
    ki[6] = (float)(c02 / det), ki[7] = (float)((k[1] * k[6] - k[0] * k[7]) / det), ki[8] = (float)((k[0] * k[4] - k[1] * k[3]) / det);
}

// Eq. (6) / (7) of arXiv:1804.09534 on the two ends of the normalising bone, the eps clamps, clamp(4, 50)
__device__ __forceinline__ float closed_form_zroot(float xm, float ym, float xn, float yn, float zm, float zn, float eps) {
    const float dx = xn - xm, dy = yn - ym;
    float a = dx * dx + dy * dy;
    const float bq = 2.f * (zn * (xn * xn + yn * yn - xn * xm - yn * ym) + zm * (xm * xm + ym * ym - xn * xm - yn * ym));
    const float ex = xn * zn - xm * zm, ey = yn * zn - ym * zm, ez = zn - zm;
    const float c = ex * ex + ey * ey + ez * ez - 1.f;
    float d = bq * bq - 4.f * a * c;
    a = max_nan(eps, a);
    d = max_nan(eps, d);
    const float zr = (-bq + sqrtf(d)) / (2.f * a);
    return zr != zr ? zr : fminf(fmaxf(zr, 4.f), 50.f);
}

}  // namespace pose_head
}  // namespace peclr
