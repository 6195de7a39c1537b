// The head of the 2.5D hand-pose model in train mode (reference src/models/rn_25D_wMLPref.py: RN_25D_wMLPref.forward and
// ZrootMLP_ref.forward with BatchNorm1d on batch statistics) and its exact backward.  fp32 (the batch reductions of BatchNorm in float64), no atomics,
// every reduction in a fixed order, a constant number of launches:
//
//   forward  (4)  head_geom_kernel   per 4 samples: fc, root zrel = 0, K^-1, kp3d_unnorm (ku), closed-form z-root (zr), MLP input x
//                 layer_fwd_kernel   x 2: a workgroup owns LC hidden units over all B rows: Linear + BatchNorm (batch statistics,
//                                    running statistics updated) + LeakyReLU; saves the pre-activation p, the activation, mean and invstd
//                 head_out_kernel    per sample: Linear(128, 1), zroot = zr + r, kp3d = ku (zrel + zroot)
//   backward (6)  out_bwd_kernel     per sample: dzroot = Gz + sum G3 ku
//                 layer_bwd_kernel   x 2: the same ownership: upstream gradient of its units (dzroot w6, or dp_next W_next from the
//                                    full dp_next), LeakyReLU and BatchNorm backward, dp, and dW / db / dgamma / dbeta of its units
//                 geom_bwd_kernel    per sample: dx = dp1 W0, back through the MLP input, kp3d and K^-1 to the fc output: do
//                 fc_wgrad_kernel    a workgroup owns 64 of the 2048 columns over all rows: dWfc = do^T feat; dbfc
//                 fc_dgrad_kernel    per 16 samples x 256 columns: dfeat = do Wfc (left out when the features need no gradient)
//
// zr is detached in the reference: the clamps and maxima of the closed form have no backward, and x[:, 63] gets none.
#include "common.hpp"
#include "pose_head.hpp"

#pragma clang fp contract(off)  // as pose.hip: the stages the two heads share round alike

namespace peclr {
namespace {
using namespace pose_head;

constexpr int MAXB = PECLR_POSE_TRAIN_MAX_BATCH;
constexpr int LC = 4;              // hidden units per workgroup of the column-owning kernels
constexpr int LT = 256;            // their threads
constexpr int LR = MAXB / LT;      // rows per thread, in registers
constexpr int LW = LT / kWave;
constexpr float SLOPE = 0.01f;

// the caller's `save` (forward -> backward) and `ws` (backward) buffers, in floats
struct Save {
    float *x, *p1, *h1, *p2, *h2, *ku;
    double* stats;  // per block mean [128], invstd [128]: float64, so that the backward forms xhat from p without a rounding
    __host__ explicit Save(float* s, int B) {
        x = s, p1 = x + (size_t)B * NO, h1 = p1 + (size_t)B * NH, p2 = h1 + (size_t)B * NH, h2 = p2 + (size_t)B * NH;
        float* st = h2 + (size_t)B * NH;
        stats = reinterpret_cast<double*>(st), ku = st + 8 * NH;
    }
};

// sums of v[0 .. LC) over the workgroup, the same bits in every thread: lanes by the butterfly, then the waves in order.
// The batch reductions of BatchNorm run in float64, as the accumulators of torch's CPU kernels do: with few samples the
// terms of the backward nearly cancel (at B = 2: 1 - xhat^2 = eps / (var + eps)), and fp32 sums would set the error.
__device__ __forceinline__ void block_sum(double* v, double (*red)[LC], int wave, int lane) {
#pragma unroll
    for (int c = 0; c < LC; ++c) v[c] = wave_sum(v[c]);
    __syncthreads();  // (red may still be read from the previous call)
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < LC; ++c) red[wave][c] = v[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < LC; ++c) {
        double s = red[0][c];
#pragma unroll
        for (int w = 1; w < LW; ++w) s += red[w][c];
        v[c] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(HT) void head_geom_kernel(const float* __restrict__ feat, int B, const float* __restrict__ fc_w,
                                                       const float* __restrict__ fc_b, const float* __restrict__ K, int k_stride,
                                                       float eps, float* __restrict__ out64, float* __restrict__ ku_out,
                                                       float* __restrict__ x_out) {
    __shared__ float fc[HS][NO];
    __shared__ float ku[HS][NJ][3];
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int b0 = blockIdx.x * HS;
    fc_stage(feat, B, b0, fc_w, fc_b, fc, wave, lane);
    __syncthreads();
    const int s = wave, b = b0 + s;
    const bool live = b < B;
    float* x = x_out + (size_t)(live ? b : 0) * NO;
    if (live && lane < NJ) {
        float ki[9];
        k_inverse(K + (size_t)b * k_stride, ki);
        const float u = fc[s][3 * lane], v = fc[s][3 * lane + 1];
        const float z = lane == 0 ? 0.f : fc[s][3 * lane + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            ku[s][lane][r] = u * ki[3 * r] + v * ki[3 * r + 1] + ki[3 * r + 2];
            ku_out[((size_t)b * NJ + lane) * 3 + r] = ku[s][lane][r];
        }
        x[lane] = z;
        x[NJ + 2 * lane] = ku[s][lane][0];
        x[NJ + 2 * lane + 1] = ku[s][lane][1];
    }
    __syncthreads();
    if (!live) return;
    out64[(size_t)b * NO + lane] = lane == 2 ? 0.f : fc[s][lane];  // zrel[:, 0] = 0, in place: kp25d sees it
    if (lane == 0)
        x[NO - 1] = closed_form_zroot(ku[s][3][0], ku[s][3][1], ku[s][8][0], ku[s][8][1], fc[s][3 * 3 + 2], fc[s][3 * 8 + 2], eps);
}

// Linear(kin, 128) + BatchNorm1d (batch statistics) + LeakyReLU for hidden units [LC blockIdx.x, +LC) of all B rows
__global__ __launch_bounds__(LT) void layer_fwd_kernel(const float* __restrict__ in, int kin, int B, const float* __restrict__ W,
                                                       const float* __restrict__ bias, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ rm,
                                                       float* __restrict__ rv, long long* __restrict__ nbt, float eps, float mom,
                                                       float* __restrict__ p_out, float* __restrict__ h,
                                                       double* __restrict__ stats_out) {
    __shared__ __align__(16) float w[LC][NH];
    __shared__ double red[LW][LC];
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int c0 = blockIdx.x * LC;
    for (int i = tid; i < LC * kin; i += LT) w[i / kin][i % kin] = W[(size_t)(c0 + i / kin) * kin + i % kin];
    __syncthreads();

    float p[LR][LC];
    double sum[LC] = {};
#pragma unroll
    for (int i = 0; i < LR; ++i) {
        const int row = tid + LT * i;
        float acc[LC] = {};  // fp32 FMA in k order: the evaluation head's sum
        if (row < B) {
            const float4* r = reinterpret_cast<const float4*>(in + (size_t)row * kin);
            for (int k4 = 0; k4 < kin / 4; ++k4) {
                const float4 v = r[k4];
#pragma unroll
                for (int c = 0; c < LC; ++c) {
                    acc[c] = fmaf(w[c][4 * k4], v.x, acc[c]);
                    acc[c] = fmaf(w[c][4 * k4 + 1], v.y, acc[c]);
                    acc[c] = fmaf(w[c][4 * k4 + 2], v.z, acc[c]);
                    acc[c] = fmaf(w[c][4 * k4 + 3], v.w, acc[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < LC; ++c) {
            p[i][c] = row < B ? acc[c] + bias[c0 + c] : 0.f;
            sum[c] += p[i][c];
        }
    }
    block_sum(sum, red, wave, lane);
    double mean[LC], sq[LC] = {};
#pragma unroll
    for (int c = 0; c < LC; ++c) mean[c] = sum[c] / B;
#pragma unroll
    for (int i = 0; i < LR; ++i)
        if (tid + LT * i < B)
#pragma unroll
            for (int c = 0; c < LC; ++c) {
                const double d = p[i][c] - mean[c];
                sq[c] += d * d;
            }
    block_sum(sq, red, wave, lane);
    double invstd[LC];
#pragma unroll
    for (int c = 0; c < LC; ++c) invstd[c] = 1.0 / sqrt(sq[c] / B + (double)eps);
#pragma unroll
    for (int i = 0; i < LR; ++i) {
        const int row = tid + LT * i;
        if (row >= B) continue;
        float xh[LC], y[LC];
#pragma unroll
        for (int c = 0; c < LC; ++c) {
            xh[c] = (float)((p[i][c] - mean[c]) * invstd[c]);  // one rounding; from here on fp32, as the evaluation head
            y[c] = leaky(xh[c] * gamma[c0 + c] + beta[c0 + c]);
        }
        *reinterpret_cast<float4*>(p_out + (size_t)row * NH + c0) = make_float4(p[i][0], p[i][1], p[i][2], p[i][3]);
        *reinterpret_cast<float4*>(h + (size_t)row * NH + c0) = make_float4(y[0], y[1], y[2], y[3]);
    }
    if (tid < LC) {
        // every thread holds every unit's statistics: thread c picks unit c without a dynamic register index
        double m = mean[0], q = sq[0], is = invstd[0];
#pragma unroll
        for (int c = 1; c < LC; ++c)
            if (tid == c) m = mean[c], q = sq[c], is = invstd[c];
        const int u = c0 + tid;
        stats_out[u] = m;
        stats_out[NH + u] = is;
        rm[u] = (float)((1.0 - mom) * rm[u] + mom * m);
        rv[u] = (float)((1.0 - mom) * rv[u] + mom * (q / (B - 1)));  // the unbiased variance
    }
    if (blockIdx.x == 0 && tid == 0) *nbt += 1;
}

__global__ __launch_bounds__(HT) void head_out_kernel(int B, const float* __restrict__ h2, const float* __restrict__ w6,
                                                      const float* __restrict__ b6, const float* __restrict__ x,
                                                      const float* __restrict__ ku, const float* __restrict__ out64,
                                                      float* __restrict__ zroot_out, float* __restrict__ kp3d) {
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int b = blockIdx.x * HS + wave;
    if (b >= B) return;
    const float* h = h2 + (size_t)b * NH;
    float part = fmaf(w6[lane], h[lane], w6[lane + kWave] * h[lane + kWave]);  // Linear(128, 1), as the evaluation head sums it
    part = wave_sum(part);
    const float zroot = x[(size_t)b * NO + NO - 1] + (part + b6[0]);
    if (lane == 0) zroot_out[b] = zroot;
    if (lane < NJ) {
        const float zrel = lane == 0 ? 0.f : out64[(size_t)b * NO + 3 * lane + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r) kp3d[((size_t)b * NJ + lane) * 3 + r] = ku[((size_t)b * NJ + lane) * 3 + r] * (zrel + zroot);
    }
}

// --------------------------------------------------------------------------------------------------------------- backward
// sum over r of G3[b][j][r] ku[b][j][r] (0 without G3)
__device__ __forceinline__ float g3_dot_ku(const float* g3, const float* ku, int b, int j) {
    if (!g3) return 0.f;
    const size_t o = ((size_t)b * NJ + j) * 3;
    return g3[o] * ku[o] + g3[o + 1] * ku[o + 1] + g3[o + 2] * ku[o + 2];
}

__global__ __launch_bounds__(HT) void out_bwd_kernel(int B, const float* __restrict__ g3, const float* __restrict__ gz,
                                                     const float* __restrict__ ku, float* __restrict__ dzroot) {
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int b = blockIdx.x * HS + wave;
    if (b >= B) return;
    const float s = wave_sum(lane < NJ ? g3_dot_ku(g3, ku, b, lane) : 0.f);
    if (lane == 0) dzroot[b] = (gz ? gz[b] : 0.f) + s;
}

// Hidden units [LC blockIdx.x, +LC) of one Linear + BatchNorm + LeakyReLU block, all B rows.  Upstream gradient of the
// activation: last = 1: up [B] (dzroot) times wn [128] (w6), and this kernel also sums dw6 / db6; last = 0: up [B][128]
// (the next block's dp) times the unit's column of wn [128][128] (the next Linear's weight).
__global__ __launch_bounds__(LT) void layer_bwd_kernel(int B, int kin, const float* __restrict__ in, const float* __restrict__ p,
                                                       const float* __restrict__ h, const double* __restrict__ stats,
                                                       const float* __restrict__ gamma, const float* __restrict__ up,
                                                       const float* __restrict__ wn, int last, float* __restrict__ dp,
                                                       float* __restrict__ dW, float* __restrict__ db, float* __restrict__ dgamma,
                                                       float* __restrict__ dbeta, float* __restrict__ dw6, float* __restrict__ db6) {
    __shared__ __align__(16) float wcol[LC][NH];
    __shared__ double red[LW][LC];
    __shared__ __align__(16) float dps[MAXB][LC];
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int c0 = blockIdx.x * LC;
    if (!last) {
        for (int i = tid; i < LC * NH; i += LT) wcol[i % LC][i / LC] = wn[(size_t)(i / LC) * NH + c0 + i % LC];
        __syncthreads();
    }

    float dy[LR][LC];
    double xh[LR][LC];  // (p - mean) invstd in float64 from the saved fp32 pre-activations: what the forward rounded once
    double mean[LC], invstd[LC];
#pragma unroll
    for (int c = 0; c < LC; ++c) mean[c] = stats[c0 + c], invstd[c] = stats[NH + c0 + c];
    double sb[LC] = {}, sg[LC] = {}, s6[LC] = {};
    double s_up = 0.0;
#pragma unroll
    for (int i = 0; i < LR; ++i) {
        const int row = tid + LT * i;
        float g[LC] = {};
        float4 hv = make_float4(0.f, 0.f, 0.f, 0.f), xv = hv;
        if (row < B) {
            hv = *reinterpret_cast<const float4*>(h + (size_t)row * NH + c0);
            xv = *reinterpret_cast<const float4*>(p + (size_t)row * NH + c0);
            if (last) {
                const float u = up[row];
                s_up += u;
#pragma unroll
                for (int c = 0; c < LC; ++c) g[c] = u * wn[c0 + c];
                s6[0] += (double)u * hv.x, s6[1] += (double)u * hv.y, s6[2] += (double)u * hv.z, s6[3] += (double)u * hv.w;
            } else {
                const float4* r = reinterpret_cast<const float4*>(up + (size_t)row * NH);
                for (int k4 = 0; k4 < NH / 4; ++k4) {
                    const float4 v = r[k4];
#pragma unroll
                    for (int c = 0; c < LC; ++c) {
                        g[c] = fmaf(wcol[c][4 * k4], v.x, g[c]);
                        g[c] = fmaf(wcol[c][4 * k4 + 1], v.y, g[c]);
                        g[c] = fmaf(wcol[c][4 * k4 + 2], v.z, g[c]);
                        g[c] = fmaf(wcol[c][4 * k4 + 3], v.w, g[c]);
                    }
                }
            }
        }
        const float hh[LC] = {hv.x, hv.y, hv.z, hv.w};
        const float xx[LC] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int c = 0; c < LC; ++c) {
            // the activation's sign is its input's; an input of 0 takes the slope, as torch's backward does
            dy[i][c] = row < B ? (hh[c] > 0.f ? g[c] : SLOPE * g[c]) : 0.f;
            xh[i][c] = row < B ? (xx[c] - mean[c]) * invstd[c] : 0.0;
            sb[c] += dy[i][c];
            sg[c] += dy[i][c] * xh[i][c];
        }
    }
    block_sum(sb, red, wave, lane);
    block_sum(sg, red, wave, lane);
    if (last) {
        block_sum(s6, red, wave, lane);
        double su[LC] = {s_up, 0.0, 0.0, 0.0};
        block_sum(su, red, wave, lane);
        if (blockIdx.x == 0 && tid == 0) db6[0] = (float)su[0];
    }
    double scale[LC];
#pragma unroll
    for (int c = 0; c < LC; ++c) scale[c] = gamma[c0 + c] * invstd[c] / B;
#pragma unroll
    for (int i = 0; i < LR; ++i) {
        const int row = tid + LT * i;
        if (row >= B) continue;
        float d[LC];
#pragma unroll
        for (int c = 0; c < LC; ++c) d[c] = (float)(scale[c] * ((double)B * dy[i][c] - sb[c] - xh[i][c] * sg[c]));
        const float4 dv = make_float4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<float4*>(dp + (size_t)row * NH + c0) = dv;
        *reinterpret_cast<float4*>(&dps[row][0]) = dv;
    }
    __syncthreads();  // dps
    if (tid < LC) {
        double b = sb[0], g = sg[0], w6 = s6[0];
#pragma unroll
        for (int c = 1; c < LC; ++c)
            if (tid == c) b = sb[c], g = sg[c], w6 = s6[c];
        dbeta[c0 + tid] = (float)b;
        dgamma[c0 + tid] = (float)g;
        db[c0 + tid] = 0.f;  // the sum of dp over the batch: exactly 0 in front of a train-mode BatchNorm
        if (last) dw6[c0 + tid] = (float)w6;
    }
    // dW[c][k] = sum_b dp[b][c] in[b][k], rows in order
    for (int i = tid; i < LC * kin; i += LT) {
        const int c = i / kin, k = i % kin;
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc = fmaf(dps[b][c], in[(size_t)b * kin + k], acc);
        dW[(size_t)(c0 + c) * kin + k] = acc;
    }
}

__global__ __launch_bounds__(HT) void geom_bwd_kernel(int B, const float* __restrict__ dp1, const float* __restrict__ w0,
                                                      const float* __restrict__ K, int k_stride, const float* __restrict__ out64,
                                                      const float* __restrict__ zroot, const float* __restrict__ ku,
                                                      const float* __restrict__ g3, const float* __restrict__ g25,
                                                      float* __restrict__ d_out) {
    __shared__ float dx[HS][NO];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int b = blockIdx.x * HS + wave;
    const bool live = b < B;
    if (live) {
        // dx = dp1 W0 (W0 [128][64]: consecutive lanes read consecutive inputs)
        const float* d = dp1 + (size_t)b * NH;
        float acc = 0.f;
        for (int o = 0; o < NH; ++o) acc = fmaf(d[o], w0[o * NO + lane], acc);
        dx[wave][lane] = acc;  // (dx[63], the gradient of the detached zr, is not read)
    }
    __syncthreads();
    if (!live) return;
    float* o = d_out + (size_t)b * NO;
    const float* g = g25 ? g25 + (size_t)b * NO : nullptr;
    if (lane == 0) o[NO - 1] = g ? g[NO - 1] : 0.f;
    if (lane >= NJ) return;
    float ki[9];
    k_inverse(K + (size_t)b * k_stride, ki);
    const float zrel = lane == 0 ? 0.f : out64[(size_t)b * NO + 3 * lane + 2];
    const float zz = zrel + zroot[b];
    const size_t j3 = ((size_t)b * NJ + lane) * 3;
    float dku[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) dku[r] = g3 ? g3[j3 + r] * zz : 0.f;
    dku[0] += dx[wave][NJ + 2 * lane];
    dku[1] += dx[wave][NJ + 2 * lane + 1];
    const float dzrel = g3_dot_ku(g3, ku, b, lane) + dx[wave][lane];
    const float du = dku[0] * ki[0] + dku[1] * ki[3] + dku[2] * ki[6];
    const float dv = dku[0] * ki[1] + dku[1] * ki[4] + dku[2] * ki[7];
    o[3 * lane] = (g ? g[3 * lane] : 0.f) + du;
    o[3 * lane + 1] = (g ? g[3 * lane + 1] : 0.f) + dv;
    o[3 * lane + 2] = lane == 0 ? 0.f : (g ? g[3 * lane + 2] : 0.f) + dzrel;  // the root's zrel was overwritten: no gradient
}

// dWfc[o][n] = sum_b do[b][o] feat[b][n] for columns n in [64 blockIdx.x, +64), rows in order; dbfc by workgroup 0
constexpr int WC = 64, WR = 64;  // columns per workgroup, rows per LDS chunk
__global__ __launch_bounds__(LT) void fc_wgrad_kernel(int B, const float* __restrict__ d_out, const float* __restrict__ feat,
                                                      float* __restrict__ d_w, float* __restrict__ d_b) {
    __shared__ float dos[WR][NO];
    __shared__ float fs[WR][WC];
    const int tid = threadIdx.x, col = tid % WC, og = tid / WC;  // thread: one column, outputs [16 og, +16)
    constexpr int OG = NO / (LT / WC);
    const int n0 = blockIdx.x * WC;
    float acc[OG] = {};
    for (int r0 = 0; r0 < B; r0 += WR) {
        const int rows = min(WR, B - r0);
        __syncthreads();
        for (int i = tid; i < rows * NO; i += LT) dos[i / NO][i % NO] = d_out[(size_t)(r0 + i / NO) * NO + i % NO];
        for (int i = tid; i < rows * WC; i += LT) fs[i / WC][i % WC] = feat[(size_t)(r0 + i / WC) * NF + n0 + i % WC];
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const float f = fs[r][col];
#pragma unroll
            for (int i = 0; i < OG; ++i) acc[i] = fmaf(dos[r][og * OG + i], f, acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < OG; ++i) d_w[(size_t)(og * OG + i) * NF + n0 + col] = acc[i];
    if (blockIdx.x == 0 && tid < NO) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += d_out[(size_t)b * NO + tid];
        d_b[tid] = s;
    }
}

// dfeat[b][n] = sum_o do[b][o] Wfc[o][n]: 16 rows x 256 columns per workgroup
constexpr int DR = 16;
__global__ __launch_bounds__(LT) void fc_dgrad_kernel(int B, const float* __restrict__ d_out, const float* __restrict__ fc_w,
                                                      float* __restrict__ d_feat) {
    __shared__ float dos[DR][NO];
    const int tid = threadIdx.x, n = blockIdx.x * LT + tid, r0 = blockIdx.y * DR;
    const int rows = min(DR, B - r0);
    for (int i = tid; i < DR * NO; i += LT) dos[i / NO][i % NO] = i / NO < rows ? d_out[(size_t)(r0 + i / NO) * NO + i % NO] : 0.f;
    __syncthreads();
    float acc[DR] = {};
    for (int o = 0; o < NO; ++o) {
        const float w = fc_w[(size_t)o * NF + n];
#pragma unroll
        for (int r = 0; r < DR; ++r) acc[r] = fmaf(dos[r][o], w, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < DR; ++r)
        if (r < rows) d_feat[(size_t)(r0 + r) * NF + n] = acc[r];
}

}  // namespace
}  // namespace peclr

using namespace peclr;

extern "C" int peclr_pose_head_train_launches(int backward, int want_d_feat) { return backward ? (want_d_feat ? 6 : 5) : 4; }

extern "C" int peclr_pose_head_train_fwd_f32(const float* feat, int B, int n_feat, const float* fc_w, const float* fc_b,
                                             float* const* mlp, float bn_eps1, float bn_eps2, float momentum1, float momentum2,
                                             int64_t* nbt1, int64_t* nbt2, const float* K, int k_per_sample, float eps,
                                             float* out64, float* kp3d, float* zroot, float* save, peclr_stream_t stream) {
    if (!feat || !fc_w || !fc_b || !mlp || !nbt1 || !nbt2 || !K || !out64 || !kp3d || !zroot || !save) return PECLR_ERR_NULL;
    for (int i = 0; i < PECLR_POSE_MLP_TENSORS; ++i)
        if (!mlp[i]) return PECLR_ERR_NULL;
    if (B < 2 || B > MAXB || n_feat != NF) return PECLR_ERR_SHAPE;
    if (!aligned16(feat) || !aligned16(fc_w) || !aligned16(save)) return PECLR_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Save s(save, B);
    const int per_sample = (B + HS - 1) / HS;
    hipLaunchKernelGGL(head_geom_kernel, dim3(per_sample), dim3(HT), 0, st, feat, B, fc_w, fc_b, K, k_per_sample ? 9 : 0, eps, out64,
                       s.ku, s.x);
    hipLaunchKernelGGL(layer_fwd_kernel, dim3(NH / LC), dim3(LT), 0, st, s.x, NO, B, mlp[0], mlp[1], mlp[2], mlp[3], mlp[4], mlp[5],
                       reinterpret_cast<long long*>(nbt1), bn_eps1, momentum1, s.p1, s.h1, s.stats);
    hipLaunchKernelGGL(layer_fwd_kernel, dim3(NH / LC), dim3(LT), 0, st, s.h1, NH, B, mlp[6], mlp[7], mlp[8], mlp[9], mlp[10], mlp[11],
                       reinterpret_cast<long long*>(nbt2), bn_eps2, momentum2, s.p2, s.h2, s.stats + 2 * NH);
    hipLaunchKernelGGL(head_out_kernel, dim3(per_sample), dim3(HT), 0, st, B, s.h2, mlp[12], mlp[13], s.x, s.ku, out64, zroot, kp3d);
    return launch_status();
}

extern "C" int peclr_pose_head_train_bwd_f32(const float* feat, int B, int n_feat, const float* fc_w, const float* const* mlp,
                                             const float* K, int k_per_sample, const float* out64, const float* zroot,
                                             const float* save, const float* g_kp3d, const float* g_out64, const float* g_zroot,
                                             float* ws, float* d_feat, float* d_fc_w, float* d_fc_b, float* const* d_mlp,
                                             peclr_stream_t stream) {
    if (!feat || !fc_w || !mlp || !K || !out64 || !zroot || !save || !ws || !d_fc_w || !d_fc_b || !d_mlp) return PECLR_ERR_NULL;
    for (int i = 0; i < PECLR_POSE_MLP_TENSORS; ++i)
        if (!mlp[i]) return PECLR_ERR_NULL;
    for (int i = 0; i < PECLR_POSE_MLP_GRADS; ++i)
        if (!d_mlp[i]) return PECLR_ERR_NULL;
    if (B < 2 || B > MAXB || n_feat != NF) return PECLR_ERR_SHAPE;
    if (!aligned16(save) || !aligned16(ws)) return PECLR_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Save s(const_cast<float*>(save), B);
    float *dp2 = ws, *dp1 = dp2 + (size_t)B * NH, *d_out = dp1 + (size_t)B * NH, *dzroot = d_out + (size_t)B * NO;
    const int per_sample = (B + HS - 1) / HS, k_stride = k_per_sample ? 9 : 0;
    hipLaunchKernelGGL(out_bwd_kernel, dim3(per_sample), dim3(HT), 0, st, B, g_kp3d, g_zroot, s.ku, dzroot);
    hipLaunchKernelGGL(layer_bwd_kernel, dim3(NH / LC), dim3(LT), 0, st, B, NH, s.h1, s.p2, s.h2, s.stats + 2 * NH, mlp[8], dzroot,
                       mlp[12], 1, dp2, d_mlp[4], d_mlp[5], d_mlp[6], d_mlp[7], d_mlp[8], d_mlp[9]);
    hipLaunchKernelGGL(layer_bwd_kernel, dim3(NH / LC), dim3(LT), 0, st, B, NO, s.x, s.p1, s.h1, s.stats, mlp[2], dp2, mlp[6], 0,
                       dp1, d_mlp[0], d_mlp[1], d_mlp[2], d_mlp[3], (float*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(geom_bwd_kernel, dim3(per_sample), dim3(HT), 0, st, B, dp1, mlp[0], K, k_stride, out64, zroot, s.ku, g_kp3d,
                       g_out64, d_out);
    hipLaunchKernelGGL(fc_wgrad_kernel, dim3(NF / WC), dim3(LT), 0, st, B, d_out, feat, d_fc_w, d_fc_b);
    if (d_feat)
        hipLaunchKernelGGL(fc_dgrad_kernel, dim3(NF / LT, (B + DR - 1) / DR), dim3(LT), 0, st, B, d_out, fc_w, d_feat);
    return launch_status();
}
