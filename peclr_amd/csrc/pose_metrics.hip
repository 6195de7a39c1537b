// The metrics every supervised step logs (reference src/models/utils.py: calculate_metrics :53-73), for one or two
// (prediction, truth) pairs of [B][21][3] float32 tensors: the Euclidean distance of all n = 21 B joints, their mean and their
// LOWER median (torch.median: element (n - 1) / 2 of the ascending order).  ONE launch, one workgroup per pair.
//
//   distances  thread t owns joints t, t + MT, ...: float64 from the float32 coordinates, summed per thread in that order and
//              folded over the threads by a binary tree; the mean is that sum / n, rounded once.
//   median     an order statistic, and rounding is monotone: the median of the float32-rounded distances IS the rounded float64
//              median.  A distance is never negative, so its float32 bit pattern orders as an unsigned integer, and a radix
//              select over the patterns is exact: four passes of 8 bits from the top, each a 256-bin histogram of the keys
//              that still match the bytes chosen so far.  The keys stay in the caller's workspace (84 KB at B = 1024; every
//              thread reads back only what it wrote itself).  The histogram is one BYTE column per thread in LDS
//              ([256 bins][MT threads], 32 KB; a thread meets at most 168 keys): no two threads ever write one counter, so
//              there is no atomic anywhere and nothing depends on the order in which waves run.
// Any NaN distance makes the pair's mean and median NaN (torch.mean, torch.median); +inf orders last; pred == truth gives +0.
#include "common.hpp"

#pragma clang fp contract(off)

namespace peclr {
namespace {

constexpr int MT = 128;    // threads of a workgroup
constexpr int MJ = 21;     // joints of a sample
constexpr int MBINS = 256;
constexpr int MMAXB = PECLR_POSE_METRICS_MAX_BATCH;
static_assert((MMAXB * MJ + MT - 1) / MT <= 255, "a thread's byte counter must hold every key it owns");
static_assert(MBINS == 2 * MT && MBINS == 4 * kWave, "two bins per thread in the row sums, four per lane in the scan");

__global__ __launch_bounds__(MT) void pose_step_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ truth,
                                                               const float* __restrict__ pred2, const float* __restrict__ truth2,
                                                               int B, uint32_t* __restrict__ workspace, float* __restrict__ out) {
    __shared__ uint32_t hist[MBINS * MT / 4];  // as bytes: [bin][thread]
    __shared__ uint32_t totals[MBINS];
    __shared__ double red[MT];
    __shared__ uint32_t chosen[2];  // the pass's bin, and the rank that is left inside it

    const int t = threadIdx.x;
    const int pair = blockIdx.x;
    const float* __restrict__ P = pair ? pred2 : pred;
    const float* __restrict__ T = pair ? truth2 : truth;
    const int n = B * MJ;
    uint32_t* __restrict__ keys = workspace + (size_t)pair * n;
    uint8_t* const column = reinterpret_cast<uint8_t*>(hist) + t;

    // ---- distances: float64, the key is the float32 rounding's bit pattern
    double acc = 0.0;
    int nan = 0;
    for (int i = t; i < n; i += MT) {
        const size_t at = (size_t)i * 3;
        const double dx = (double)P[at] - (double)T[at], dy = (double)P[at + 1] - (double)T[at + 1],
                     dz = (double)P[at + 2] - (double)T[at + 2];
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        acc += d;
        const float f = (float)d;
        nan |= f != f;
        keys[i] = __float_as_uint(f);
    }
    red[t] = acc;
    const int any_nan = __syncthreads_or(nan);
    for (int o = MT / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    const double sum = red[0];

    // ---- radix select of rank (n - 1) / 2
    uint32_t prefix = 0, rank = (uint32_t)(n - 1) / 2;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int w = t; w < MBINS * MT / 4; w += MT) hist[w] = 0;
        __syncthreads();
        for (int i = t; i < n; i += MT) {
            const uint32_t key = keys[i];
            // (the bytes above this pass's: a shift by 32 is not defined, the first pass takes every key)
            if (shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8))) ++column[((key >> shift) & 255u) * MT];
        }
        __syncthreads();
        // bins t and t + MT: the sum of the row's MT byte counters, read as words (rotated by t: no two lanes on one bank)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int bin = t + h * MT;
            uint32_t s = 0;
            for (int w = 0; w < MT / 4; ++w) {
                const uint32_t v = hist[bin * (MT / 4) + ((w + t) & (MT / 4 - 1))];
                s += (v & 255u) + ((v >> 8) & 255u) + ((v >> 16) & 255u) + (v >> 24);
            }
            totals[bin] = s;
        }
        __syncthreads();
        // the first wave finds the bin that holds the rank: lane l scans bins 4 l .. 4 l + 3 after the lanes below it
        if (t < kWave) {
            uint32_t c[4], mine = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                c[q] = totals[4 * t + q];
                mine += c[q];
            }
            uint32_t incl = mine;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const uint32_t below = __shfl_up(incl, o, kWave);
                if (t >= o) incl += below;
            }
            uint32_t before = incl - mine;
            if (before <= rank && rank < incl) {  // (exactly one lane: the rank is below the number of keys that matched)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (rank >= before && rank < before + c[q]) {
                        chosen[0] = (uint32_t)(4 * t + q);
                        chosen[1] = rank - before;
                    }
                    before += c[q];
                }
            }
        }
        __syncthreads();
        prefix |= chosen[0] << shift;
        rank = chosen[1];
    }
    if (t == 0) {
        const float quiet = __uint_as_float(0x7FC00000u);
        out[2 * pair] = any_nan ? quiet : (float)(sum / (double)n);
        out[2 * pair + 1] = any_nan ? quiet : __uint_as_float(prefix);
    }
}

}  // namespace
}  // namespace peclr

using namespace peclr;

extern "C" int peclr_pose_step_metrics_f32(const float* pred, const float* truth, const float* pred2, const float* truth2, int B,
                                           void* workspace, float* out, peclr_stream_t stream) {
    if (!pred || !truth || !workspace || !out || (pred2 == nullptr) != (truth2 == nullptr)) return PECLR_ERR_NULL;
    if (B < 1 || B > MMAXB) return PECLR_ERR_SHAPE;
    hipLaunchKernelGGL(pose_step_metrics_kernel, dim3(pred2 ? 2 : 1), dim3(MT), 0, static_cast<hipStream_t>(stream), pred, truth,
                       pred2, truth2, B, static_cast<uint32_t*>(workspace), out);
    return launch_status();
}
