// The fine-tuned 2.5D hand-pose model at evaluation time (reference src/models/rn_25D_wMLPref.py, testing/pred_fh.py,
// testing/fh_utils.py): everything of the two-pass crop -> predict -> re-crop loop that is not the ResNet backbone.
//
//   pose_crop_kernel  fh_utils.preprocess for a batch: cv.warpAffine(img, T[:2], (S, S)) on 8-bit RGB (warp_u8.hpp), the
//                     u8 -> float32 normalisation by a [3][256] table, fp32 [B][S][S][3] (= [B,3,S,S] channels_last) out;
//                     K' = float32(T @ K) (product in float64)
//   pose_head_kernel  pooled features [B,2048] -> fc -> kp25d / zrel (root zeroed) -> K'^-1 -> kp3d_unnorm -> closed-form
//                     z-root (Eq. 6/7 of arXiv:1804.09534, eps clamps) -> clamp(4, 50) -> refinement MLP (eval BatchNorm1d,
//                     LeakyReLU 0.01) -> kp3d; epilogue of pass 1: the re-crop matrix T2 of pred() from kp2d and T1;
//                     epilogue of pass 2: the FreiHAND submission joints (palm -> wrist, joint order, metric scale)
//
// The work is small (the head is ~0.13 MFLOP per image); the point is one launch per stage, no intermediate tensors and no
// host round trip between the two passes.
#include "affine.hpp"
#include "common.hpp"
#include "pose_head.hpp"
#include "warp_u8.hpp"

#pragma clang fp contract(off)  // products and sums round separately, as the host restatements do

namespace peclr {
namespace {
using namespace pose_head;  // the stages shared with the training head (pose_train.hip)

constexpr int CX = 64, CY = 4;  // crop: one thread per output pixel, consecutive lanes = consecutive x

__global__ __launch_bounds__(CX* CY) void pose_crop_kernel(const uint8_t* __restrict__ images, int H, int W,
                                                           const double* __restrict__ T, const double* __restrict__ K,
                                                           const float* __restrict__ table, int S, float* __restrict__ out,
                                                           float* __restrict__ k_out) {
    __shared__ float tab[3 * 256];
    const int b = blockIdx.z;
    const int tid = threadIdx.y * CX + threadIdx.x;
    for (int i = tid; i < 3 * 256; i += CX * CY) tab[i] = table[i];
    const double* t = T + (size_t)b * 9;
    if (K && blockIdx.x == 0 && blockIdx.y == 0 && tid < 9) {  // K' = T @ K, float64 products and sums, then float32
        const int r = tid / 3, c = tid % 3;
        const double* k = K + (size_t)b * 9;
        k_out[(size_t)b * 9 + tid] = (float)(t[3 * r] * k[c] + t[3 * r + 1] * k[3 + c] + t[3 * r + 2] * k[6 + c]);
    }
    __syncthreads();
    const int x = blockIdx.x * CX + threadIdx.x, y = blockIdx.y * CY + threadIdx.y;
    if (x >= S || y >= S) return;
    double mi[6];
    const double m[6] = {t[0], t[1], t[2], t[3], t[4], t[5]};
    invert_affine(m, mi);
    int px[3];
    warp_bilinear_u8(images + (size_t)b * H * W * 3, H, W, mi, x, y, px);
    // BORDER_CONSTANT with borderValue (0.485, 0.456, 0.406) is 0 after saturate_cast<uchar>: the warp's zero taps
    float* o = out + (((size_t)b * S + y) * S + x) * 3;
    o[0] = tab[px[0]], o[1] = tab[256 + px[1]], o[2] = tab[512 + px[2]];
}

// ---- head (HS samples per workgroup and the sizes: pose_head.hpp)
struct MlpParams {
    const float *w0, *b0, *g1, *be1, *rm1, *rv1, *w3, *b3, *g4, *be4, *rm4, *rv4, *w6, *b6;
    float eps1, eps4;
};

struct HeadSmem {
    float w0t[NO][NH];   // Linear(64, 128) weight, transposed: [in][out] (consecutive lanes read consecutive outputs)
    float w3t[NH][NH];   // Linear(128, 128) weight, transposed
    float w6[NH];
    float b0[NH], a1[NH], c1[NH];  // bias; BatchNorm1d as y = x * a + c (a = weight / sqrt(var + eps), c = bias - mean * a)
    float b3[NH], a4[NH], c4[NH];
    float fc[HS][NO];    // fc output (the reference's `out`, root zrel zeroed)
    float ku[HS][NJ][3]; // kp3d_unnorm
    float in[HS][NO];    // MLP input
    float h1[HS][NH], h2[HS][NH];
    float zroot[HS];
};

// the eval-mode BatchNorm1d of torch's CPU kernel: invstd = 1 / sqrt(var + eps), alpha = invstd * weight, beta = bias - mean * alpha
__device__ __forceinline__ void bn_coef(const float* g, const float* be, const float* rm, const float* rv, float eps, int i,
                                        float& a, float& c) {
    const float invstd = 1.f / sqrtf(rv[i] + eps);
    a = invstd * g[i];
    c = be[i] - rm[i] * a;
}

// FreiHAND joint order (fh_utils.convert_order): output joint i is model joint kFhOrder[i]
__constant__ int kFhOrder[NJ] = {0, 1, 6, 11, 16, 2, 7, 12, 17, 3, 8, 13, 18, 4, 9, 14, 19, 5, 10, 15, 20};

__global__ __launch_bounds__(HT) void pose_head_kernel(const float* __restrict__ feat, int B, const float* __restrict__ fc_w,
                                                       const float* __restrict__ fc_b, MlpParams p, const float* __restrict__ K,
                                                       int k_stride, float eps, float* __restrict__ out64,
                                                       float* __restrict__ kp3d, const double* __restrict__ T1,
                                                       double* __restrict__ T2, int S, const double* __restrict__ scale,
                                                       double* __restrict__ fh, int* __restrict__ status) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    HeadSmem& sm = *reinterpret_cast<HeadSmem*>(smem_raw);
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int b0 = blockIdx.x * HS;

    // MLP parameters into LDS
    for (int i = tid; i < NH * NO; i += HT) {
        const int o = i / NO, k = i % NO;
        sm.w0t[k][o] = p.w0[i];
    }
    for (int i = tid; i < NH * NH; i += HT) {
        const int o = i / NH, k = i % NH;
        sm.w3t[k][o] = p.w3[i];
    }
    if (tid < NH) {
        sm.w6[tid] = p.w6[tid];
        sm.b0[tid] = p.b0[tid];
        sm.b3[tid] = p.b3[tid];
        bn_coef(p.g1, p.be1, p.rm1, p.rv1, p.eps1, tid, sm.a1[tid], sm.c1[tid]);
        bn_coef(p.g4, p.be4, p.rm4, p.rv4, p.eps4, tid, sm.a4[tid], sm.c4[tid]);
    }

    fc_stage(feat, B, b0, fc_w, fc_b, sm.fc, wave, lane);
    __syncthreads();

    // per sample (wave s, lanes = joints): root zrel, K'^-1, kp3d_unnorm, MLP input
    const int s = wave, b = b0 + s;
    const bool live = b < B;
    if (live) {
        if (lane == 0) sm.fc[s][2] = 0.f;  // zrel[:, 0] = 0, in place: kp25d sees it
        float ki[9];
        k_inverse(K + (size_t)b * k_stride, ki);
        if (lane < NJ) {
            const float u = sm.fc[s][3 * lane], v = sm.fc[s][3 * lane + 1];
            const float z = lane == 0 ? 0.f : sm.fc[s][3 * lane + 2];
#pragma unroll
            for (int r = 0; r < 3; ++r) sm.ku[s][lane][r] = u * ki[3 * r] + v * ki[3 * r + 1] + ki[3 * r + 2];
            sm.in[s][lane] = z;
            sm.in[s][NJ + 2 * lane] = sm.ku[s][lane][0];
            sm.in[s][NJ + 2 * lane + 1] = sm.ku[s][lane][1];
        }
    }
    __syncthreads();
    if (live && lane == 0) {
        // Eq. (6) / (7) on bones 3 and 8, the eps clamps, clamp(4, 50)
        const float zr = closed_form_zroot(sm.ku[s][3][0], sm.ku[s][3][1], sm.ku[s][8][0], sm.ku[s][8][1], sm.fc[s][3 * 3 + 2],
                                           sm.fc[s][3 * 8 + 2], eps);
        sm.zroot[s] = zr;
        sm.in[s][NO - 1] = zr;
    }
    __syncthreads();

    // MLP: Linear(64, 128) -> BN -> LeakyReLU -> Linear(128, 128) -> BN -> LeakyReLU; thread = (hidden unit, sample pair)
    {
        const int u = tid % NH;
        for (int ss = tid / NH; ss < HS; ss += HT / NH) {
            float acc = 0.f;
            for (int k = 0; k < NO; ++k) acc = fmaf(sm.w0t[k][u], sm.in[ss][k], acc);
            sm.h1[ss][u] = leaky((acc + sm.b0[u]) * sm.a1[u] + sm.c1[u]);
        }
        __syncthreads();
        for (int ss = tid / NH; ss < HS; ss += HT / NH) {
            float acc = 0.f;
            for (int k = 0; k < NH; ++k) acc = fmaf(sm.w3t[k][u], sm.h1[ss][k], acc);
            sm.h2[ss][u] = leaky((acc + sm.b3[u]) * sm.a4[u] + sm.c4[u]);
        }
        __syncthreads();
    }
    if (!live) return;
    // Linear(128, 1): wave s reduces sample s
    float part = fmaf(sm.w6[lane], sm.h2[s][lane], sm.w6[lane + kWave] * sm.h2[s][lane + kWave]);
    part = wave_sum(part);
    const float zroot = sm.zroot[s] + (part + p.b6[0]);

    out64[(size_t)b * NO + lane] = sm.fc[s][lane];
    float k3[3] = {0.f, 0.f, 0.f};
    if (lane < NJ) {
        const float zrel = lane == 0 ? 0.f : sm.fc[s][3 * lane + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            k3[r] = sm.ku[s][lane][r] * (zrel + zroot);
            kp3d[((size_t)b * NJ + lane) * 3 + r] = k3[r];
        }
    }

    if (T1) {
        // pass 1 epilogue: get_bbox_from_pose (NaN coordinates dropped, min / max, int() truncation), the corners through
        // inv(T1)[:2], create_affine_transform_from_bbox (no modify_bbox on this pass)
        const float u = lane < NJ ? sm.fc[s][3 * lane] : NAN, v = lane < NJ ? sm.fc[s][3 * lane + 1] : NAN;
        const bool xv = u == u, yv = v == v;
        const float x_lo = wave_min(xv ? u : INFINITY), x_hi = wave_max(xv ? u : -INFINITY);
        const float y_lo = wave_min(yv ? v : INFINITY), y_hi = wave_max(yv ? v : -INFINITY);
        const bool any_x = __any(xv), any_y = __any(yv);
        // (every lane holds the same reductions: lanes 0..8 write one matrix entry each)
        const bool no_box = !any_x || !any_y;
        const double x1 = trunc((double)x_lo), x2 = trunc((double)x_hi), y1 = trunc((double)y_lo), y2 = trunc((double)y_hi);
        const double* t = T1 + (size_t)b * 9;
        const double m[6] = {t[0], t[1], t[2], t[3], t[4], t[5]};
        double mi[6];
        invert_affine(m, mi);
        const double X1 = mi[0] * x1 + mi[1] * y1 + mi[2], Y1 = mi[3] * x1 + mi[4] * y1 + mi[5];
        const double X2 = mi[0] * x2 + mi[1] * y2 + mi[2], Y2 = mi[3] * x2 + mi[4] * y2 + mi[5];
        const double w = X2 - X1, h = Y2 - Y1;
        const double l = w > h ? w : h;
        const double sc = (0.7 * S) / l;
        const double cx = (X1 + X2) / 2.0, cy = (Y1 + Y2) / 2.0;
        const double half = S / 2.0;
        double e = lane == 8 ? 1.0 : 0.0;
        if (lane == 0 || lane == 4) e = sc;
        if (lane == 2) e = half - sc * cx;
        if (lane == 5) e = half - sc * cy;
        if (no_box) e = __builtin_nan("");
        if (lane < 9) T2[(size_t)b * 9 + lane] = e;
        if (lane == 0) status[b] = no_box ? PECLR_POSE_STATUS_NO_BBOX : 0;
    }
    if (scale) {
        // pass 2 epilogue: float64, palm -> wrist (2 kp[0] - kp[3]), FreiHAND joint order, metric scale; NaN -> status bit
        const int src = lane < NJ ? kFhOrder[lane] : 0;
        const double sb = scale[b];
        bool nan = false;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double at_src = (double)__shfl(k3[r], src, kWave), palm = (double)__shfl(k3[r], 0, kWave);
            const double mcp = (double)__shfl(k3[r], 3, kWave);
            const double v = src == 0 ? 2.0 * palm - mcp : at_src;
            const double o = v * sb;
            if (lane < NJ) {
                nan = nan || o != o;
                fh[((size_t)b * NJ + lane) * 3 + r] = o;
            }
        }
        const bool any_nan = __any(nan);
        if (lane == 0 && any_nan) status[b] |= PECLR_POSE_STATUS_NAN;
    }
}

}  // namespace
}  // namespace peclr

using namespace peclr;

extern "C" int peclr_pose_crop_u8(const uint8_t* images, int B, int H, int W, const double* T, const double* K,
                                  const float* table, int S, float* out, float* k_out, peclr_stream_t stream) {
    if (!images || !T || !table || !out || (K && !k_out)) return PECLR_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || S <= 0 || B > 65535 || S > 65535) return PECLR_ERR_SHAPE;
    dim3 grid((S + CX - 1) / CX, (S + CY - 1) / CY, B);
    hipLaunchKernelGGL(pose_crop_kernel, grid, dim3(CX, CY), 0, static_cast<hipStream_t>(stream), images, H, W, T, K, table, S,
                       out, k_out);
    return launch_status();
}

extern "C" int peclr_pose_head_f32(const float* feat, int B, int n_feat, const float* fc_w, const float* fc_b,
                                   const float* const* mlp, float bn_eps1, float bn_eps2, const float* K, int k_per_sample,
                                   float eps, float* out64, float* kp3d, const double* T1, double* T2, int S,
                                   const double* scale, double* fh, int* status, peclr_stream_t stream) {
    if (!feat || !fc_w || !fc_b || !mlp || !K || !out64 || !kp3d || !status) return PECLR_ERR_NULL;
    for (int i = 0; i < PECLR_POSE_MLP_TENSORS; ++i)
        if (!mlp[i]) return PECLR_ERR_NULL;
    if ((T1 && !T2) || (scale && !fh)) return PECLR_ERR_NULL;
    if (B <= 0 || n_feat != NF || (T1 && scale) || (T1 && S <= 0)) return PECLR_ERR_SHAPE;
    if (!aligned16(feat) || !aligned16(fc_w)) return PECLR_ERR_ALIGN;
    MlpParams p{mlp[0], mlp[1], mlp[2], mlp[3], mlp[4], mlp[5], mlp[6], mlp[7], mlp[8], mlp[9], mlp[10], mlp[11], mlp[12], mlp[13],
                bn_eps1, bn_eps2};
    const size_t smem = sizeof(HeadSmem);
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(pose_head_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)smem) != hipSuccess)
            return launch_status();
        attr = true;
    }
    const int grid = (B + HS - 1) / HS;
    hipLaunchKernelGGL(pose_head_kernel, dim3(grid), dim3(HT), smem, static_cast<hipStream_t>(stream), feat, B, fc_w, fc_b, p, K,
                       k_per_sample ? 9 : 0, eps, out64, kp3d, T1, T2, S, scale, fh, status);
    return launch_status();
}
