// Two-pass hand-pose prediction on images of any size, with a hand box and a left-hand flag per sample (host side:
// peclr_amd/predict.py).  The backbone and the head are the FreiHAND predictor's (pose.hip); what differs is the two ends:
//
//   pose_crop_ragged_kernel  pose_crop_kernel for a packed batch: sample b's image is H x W x 3 bytes at a byte offset of one
//                            buffer, both read from a DEVICE table geom [B][4] int64 = (offset, H, W, flip) -- a hipGraph replay
//                            only refreshes the table.  flip != 0: the crop of img[:, ::-1] (the mirrored read of warp_u8.hpp)
//                            and K' = float32(T @ Kf), Kf = F K M the camera of the mirrored image looking at the mirrored scene.
//   pose_unmap_kernel        after pass 2: the 2D keypoints back through inv(T2) into source pixels (un-mirrored for flip), and
//                            copies of kp3d / the FreiHAND joints with X negated for flip (the mirrored scene back to the real one).
//
// Both are small and latency-bound: one launch per stage, consecutive lanes write consecutive addresses, float64 products and
// sums in the order the host restatements use.
#include "affine.hpp"
#include "common.hpp"
#include "warp_u8.hpp"

#pragma clang fp contract(off)  // products and sums round separately, as the host restatements do

namespace peclr {
namespace {

constexpr int CX = 64, CY = 4;  // crop: one thread per output pixel, consecutive lanes = consecutive x (as pose_crop_kernel)
constexpr int NG = 4;           // geom row: byte offset, H, W, flip
constexpr int NJ = 21;
constexpr int UT = 256;         // unmap: one thread per output coordinate

__global__ __launch_bounds__(CX* CY) void pose_crop_ragged_kernel(const uint8_t* __restrict__ packed, long long total_bytes,
                                                                  const long long* __restrict__ geom,
                                                                  const double* __restrict__ T, const double* __restrict__ K,
                                                                  const float* __restrict__ table, int S, float* __restrict__ out,
                                                                  float* __restrict__ k_out) {
    __shared__ float tab[3 * 256];
    const int b = blockIdx.z;
    const int tid = threadIdx.y * CX + threadIdx.x;
    for (int i = tid; i < 3 * 256; i += CX * CY) tab[i] = table[i];
    const long long* g = geom + (size_t)b * NG;
    const long long off = g[0];
    long long H = g[1], W = g[2];
    const bool flip = g[3] != 0;
    // a row that does not lie inside the buffer is an empty image (every tap outside): nothing is read through it
    if (off < 0 || H < 1 || W < 1 || H > 0x7fffffffLL || W > 0x7fffffffLL || H * W > (total_bytes - off) / 3) H = W = 0;
    const double* t = T + (size_t)b * 9;
    if (K && blockIdx.x == 0 && blockIdx.y == 0 && tid < 9) {  // K' = T @ Kf, float64 products and sums, then float32
        const int r = tid / 3, c = tid % 3;
        const double* k = K + (size_t)b * 9;
        double k0 = k[c], k1 = k[3 + c], k2 = k[6 + c];
        if (flip) {  // Kf = F K M: row 0 mirrored in the image ((W - 1) row 2 - row 0), then column 0 negated
            k0 = (double)(W - 1) * k2 - k0;
            if (c == 0) k0 = -k0, k1 = -k1, k2 = -k2;
        }
        k_out[(size_t)b * 9 + tid] = (float)(t[3 * r] * k0 + t[3 * r + 1] * k1 + t[3 * r + 2] * k2);
    }
    __syncthreads();
    const int x = blockIdx.x * CX + threadIdx.x, y = blockIdx.y * CY + threadIdx.y;
    if (x >= S || y >= S) return;
    double mi[6];
    const double m[6] = {t[0], t[1], t[2], t[3], t[4], t[5]};
    invert_affine(m, mi);
    int px[3];
    const uint8_t* img = packed + (H ? off : 0);
    if (flip)
        warp_bilinear_u8<true>(img, (int)H, (int)W, mi, x, y, px);
    else
        warp_bilinear_u8<false>(img, (int)H, (int)W, mi, x, y, px);
    float* o = out + (((size_t)b * S + y) * S + x) * 3;
    o[0] = tab[px[0]], o[1] = tab[256 + px[1]], o[2] = tab[512 + px[2]];
}

// thread e of B * 63: coordinate e of kp3d / xyz; the first B * 42 threads also write coordinate e of kp2d_src
__global__ __launch_bounds__(UT) void pose_unmap_kernel(const float* __restrict__ out64, const double* __restrict__ T2,
                                                        const long long* __restrict__ geom, const float* __restrict__ kp3d_in,
                                                        const double* __restrict__ fh, int B, double* __restrict__ kp2d_src,
                                                        float* __restrict__ kp3d, double* __restrict__ xyz) {
    const long long e = (long long)blockIdx.x * UT + threadIdx.x;
    if (e < (long long)B * NJ * 3) {
        const int b = (int)(e / (NJ * 3));
        const bool neg = geom[(size_t)b * NG + 3] != 0 && e % 3 == 0;
        const float p = kp3d_in[e];
        const double q = fh[e];
        kp3d[e] = neg ? -p : p;
        xyz[e] = neg ? -q : q;
    }
    if (e < (long long)B * NJ * 2) {
        const int b = (int)(e / (NJ * 2)), j = (int)(e % (NJ * 2)) / 2, c = (int)(e % 2);
        const double* t = T2 + (size_t)b * 9;
        const double m[6] = {t[0], t[1], t[2], t[3], t[4], t[5]};
        double mi[6];
        invert_affine(m, mi);
        const double x = (double)out64[(size_t)b * 64 + 3 * j], y = (double)out64[(size_t)b * 64 + 3 * j + 1];
        double v = mi[3 * c] * x + mi[3 * c + 1] * y + mi[3 * c + 2];
        if (c == 0 && geom[(size_t)b * NG + 3] != 0) v = (double)(geom[(size_t)b * NG + 2] - 1) - v;
        kp2d_src[e] = v;
    }
}

}  // namespace
}  // namespace peclr

using namespace peclr;

extern "C" int peclr_pose_crop_ragged_u8(const uint8_t* packed, int64_t total_bytes, int B, const int64_t* geom, const double* T,
                                         const double* K, const float* table, int S, float* out, float* k_out,
                                         peclr_stream_t stream) {
    if (!packed || !geom || !T || !table || !out || (K && !k_out)) return PECLR_ERR_NULL;
    if (total_bytes <= 0 || B <= 0 || S <= 0 || B > 65535 || S > 65535) return PECLR_ERR_SHAPE;
    dim3 grid((S + CX - 1) / CX, (S + CY - 1) / CY, B);
    hipLaunchKernelGGL(pose_crop_ragged_kernel, grid, dim3(CX, CY), 0, static_cast<hipStream_t>(stream), packed,
                       (long long)total_bytes, reinterpret_cast<const long long*>(geom), T, K, table, S, out, k_out);
    return launch_status();
}

extern "C" int peclr_pose_unmap(const float* out64, const double* T2, const int64_t* geom, const float* kp3d_in, const double* fh,
                                int B, double* kp2d_src, float* kp3d, double* xyz, peclr_stream_t stream) {
    if (!out64 || !T2 || !geom || !kp3d_in || !fh || !kp2d_src || !kp3d || !xyz) return PECLR_ERR_NULL;
    if (B <= 0 || B > (1 << 24)) return PECLR_ERR_SHAPE;
    const int grid = (B * NJ * 3 + UT - 1) / UT;
    hipLaunchKernelGGL(pose_unmap_kernel, dim3(grid), dim3(UT), 0, static_cast<hipStream_t>(stream), out64, T2,
                       reinterpret_cast<const long long*>(geom), kp3d_in, fh, B, kp2d_src, kp3d, xyz);
    return launch_status();
}
