// One destination pixel of cv::warpAffine on an 8-bit, 3-channel image (INTER_LINEAR, BORDER_CONSTANT 0), shared by the
// augmenter's rotation (augment.hip) and the pose model's evaluation crop (pose.hip).
#pragma once
#include "common.hpp"

namespace peclr {

// minv: the INVERSE map [a11 a12 b1 a21 a22 b2] (destination -> source), as imgwarp.cpp forms it from the forward matrix.
// Source coordinates in 10-bit fixed point rounded to 1/32 pixel, bilinear weights as 15-bit integers; taps outside the
// image contribute 0.  Writes the three rounded 8-bit channel values.
// MIRROR (the any-size predictor's left hands, predict.hip): a tap at source column sx reads column W - 1 - sx, so the result is
// that of img[:, ::-1] bit for bit -- the coordinates, weights and border tests are untouched.  (A mirror composed into `minv`
// would round differently at 1/32 pixel.)  The default instantiation is the code of before.
template <bool MIRROR = false>
__device__ __forceinline__ void warp_bilinear_u8(const uint8_t* __restrict__ src, int H, int W, const double* minv, int x, int y,
                                                 int out[3]) {
#pragma clang fp contract(off)  // products and sums round separately, as in the scalar restatement
    const long long xf = ((long long)rint((minv[1] * y + minv[2]) * 1024.0) + 16 + (long long)rint(minv[0] * x * 1024.0)) >> 5;
    const long long yf = ((long long)rint((minv[4] * y + minv[5]) * 1024.0) + 16 + (long long)rint(minv[3] * x * 1024.0)) >> 5;
    const long long sx = xf >> 5, sy = yf >> 5;
    const int fx = (int)(xf & 31), fy = (int)(yf & 31);
    const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    const bool x0ok = sx >= 0 && sx < W, x1ok = sx + 1 >= 0 && sx + 1 < W;
    const bool y0ok = sy >= 0 && sy < H, y1ok = sy + 1 >= 0 && sy + 1 < H;
    int acc[3] = {0, 0, 0};
    if (y0ok && x0ok) {
        const uint8_t* s = src + (MIRROR ? ((size_t)sy * W + (W - 1 - sx)) * 3 : ((size_t)sy * W + sx) * 3);
        acc[0] += s[0] * w00, acc[1] += s[1] * w00, acc[2] += s[2] * w00;
    }
    if (y0ok && x1ok) {
        const uint8_t* s = src + (MIRROR ? ((size_t)sy * W + (W - 2 - sx)) * 3 : ((size_t)sy * W + sx + 1) * 3);
        acc[0] += s[0] * w01, acc[1] += s[1] * w01, acc[2] += s[2] * w01;
    }
    if (y1ok && x0ok) {
        const uint8_t* s = src + (MIRROR ? ((size_t)(sy + 1) * W + (W - 1 - sx)) * 3 : ((size_t)(sy + 1) * W + sx) * 3);
        acc[0] += s[0] * w10, acc[1] += s[1] * w10, acc[2] += s[2] * w10;
    }
    if (y1ok && x1ok) {
        const uint8_t* s = src + (MIRROR ? ((size_t)(sy + 1) * W + (W - 2 - sx)) * 3 : ((size_t)(sy + 1) * W + sx + 1) * 3);
        acc[0] += s[0] * w11, acc[1] += s[1] * w11, acc[2] += s[2] * w11;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (acc[c] + (1 << 14)) >> 15;
}

}  // namespace peclr
