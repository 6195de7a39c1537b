// The inverse of a 2x3 forward matrix as OpenCV forms it, shared by the pose model's crop and re-crop (pose.hip) and the
// any-size predictor's crop and un-mapping (predict.hip).
#pragma once
#include "common.hpp"

namespace peclr {

// cv::invertAffineTransform of the 2x3 forward matrix (imgwarp.cpp), [a11 a12 b1 a21 a22 b2]
__device__ __forceinline__ void invert_affine(const double* m, double* mi) {
#pragma clang fp contract(off)  // products and sums round separately, as the host restatements do
    double d = m[0] * m[4] - m[1] * m[3];
    d = d != 0.0 ? 1.0 / d : 0.0;
    const double a11 = m[4] * d, a22 = m[0] * d, a12 = m[1] * -d, a21 = m[3] * -d;
    mi[0] = a11, mi[1] = a12, mi[3] = a21, mi[4] = a22;
    mi[2] = -a11 * m[2] - a12 * m[5];
    mi[5] = -a21 * m[2] - a22 * m[5];
}

}  // namespace peclr
