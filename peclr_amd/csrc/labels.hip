// The label side of a supervised sample (reference src/data_loader/utils.py: convert_to_2_5D, convert_2_5D_to_3D,
// get_root_depth, get_zroot_constraint_terms; src/data_loader/data_set.py: prepare_supervised_sample, move_wrist_to_palm), for a
// batch, one launch per entry point.
//
//   one wave per sample, LS samples per workgroup; lane j < 21 owns joint j (its three coordinates).  What a sample has once --
//   the bone scale, the inverse camera matrix, the root depth, K' = T K -- EVERY lane computes for itself from the sample's K
//   and its joints 0 and 2 (loads that the whole wave shares; a few dozen float64 operations): no lane hands a value to
//   another, so there is no LDS, no barrier, no shuffle and no atomic.  A sample's outputs depend on that sample alone.
//
// Arithmetic: every stage is evaluated in float64 from float32 inputs and each emitted tensor is rounded to float32 once.  A
// stage that follows reads the ROUNDED tensor, as the reference's chain reads its float32 tensors: the re-creation reads the
// float32 joints, scale and K'.  Contraction is off: a product and a sum are two roundings, as in the NumPy restatement the
// tests compare with.
#include "labels.hpp"  // the wave layout and the pieces pose_loss.hip shares: load3 / load9, inverse3, root_depth, to_3d

#pragma clang fp contract(off)

namespace peclr {
namespace {

// convert_to_2_5D: the length of the wrist -- index-MCP bone
__device__ __forceinline__ double bone_scale(const double w[3], const double c[3]) {
    const double d0 = c[0] - w[0], d1 = c[1] - w[1], d2 = c[2] - w[2];
    return sqrt(d0 * d0 + d1 * d1 + d2 * d2);
}
// convert_to_2_5D for one joint p: (K p) / z in x and y, the depth relative to the wrist over the bone length
__device__ __forceinline__ void to_25d(const double K[9], const double p[3], const double w[3], double scale, double out[3]) {
    out[0] = (K[0] * p[0] + K[1] * p[1] + K[2] * p[2]) / p[2];
    out[1] = (K[3] * p[0] + K[4] * p[1] + K[5] * p[2]) / p[2];
    out[2] = (p[2] - w[2]) / scale;
}
__device__ __forceinline__ void store3(float* __restrict__ p, const double v[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = (float)v[c];
}
// what a later stage reads of an emitted tensor: the float32 value
__device__ __forceinline__ void round3(double v[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (double)(float)v[c];
}

__global__ __launch_bounds__(LT) void joints3d_to_25d_kernel(const float* __restrict__ K, const float* __restrict__ j3d, int B,
                                                             float* __restrict__ j25d, float* __restrict__ scale) {
    const int lane = threadIdx.x % kWave;
    const int b = blockIdx.x * LS + threadIdx.x / kWave;
    if (b >= B || lane >= LJ) return;
    const float* J = j3d + (size_t)b * LJ * 3;
    double k[9], p[3], w[3], c[3], out[3];
    load9(K + (size_t)b * 9, k);
    load3(J + lane * 3, p);
    load3(J + kParent * 3, w);
    load3(J + kChild * 3, c);
    const double s = bone_scale(w, c);
    to_25d(k, p, w, s, out);
    store3(j25d + ((size_t)b * LJ + lane) * 3, out);
    if (lane == 0) scale[b] = (float)s;
}

__global__ __launch_bounds__(LT) void joints25d_to_3d_kernel(const float* __restrict__ j25d, const float* __restrict__ scale,
                                                             const float* __restrict__ K, const float* __restrict__ z_root_calc,
                                                             int B, float* __restrict__ j3d, float* __restrict__ z_root) {
    const int lane = threadIdx.x % kWave;
    const int b = blockIdx.x * LS + threadIdx.x / kWave;
    if (b >= B || lane >= LJ) return;
    const float* J = j25d + (size_t)b * LJ * 3;
    double k[9], inv[9], p[3], n[3], m[3], out[3];
    load9(K + (size_t)b * 9, k);
    load3(J + lane * 3, p);
    load3(J + kParent * 3, n);
    load3(J + kChild * 3, m);
    inverse3(k, inv);
    const double zr = root_depth(inv, n, m);
    to_3d(inv, p, z_root_calc ? (double)z_root_calc[b] : zr, (double)scale[b], out);
    store3(j3d + ((size_t)b * LJ + lane) * 3, out);
    if (lane == 0 && z_root) z_root[b] = (float)zr;
}

// T applied to (u, v, 1); the depth stays
__device__ __forceinline__ void apply_t(const double T[9], double p[3]) {
    const double u = T[0] * p[0] + T[1] * p[1] + T[2], v = T[3] * p[0] + T[4] * p[1] + T[5];
    p[0] = u;
    p[1] = v;
}

__device__ __forceinline__ int mirror_width(int) { return 0; }
__device__ __forceinline__ int mirror_width(int b, const int* __restrict__ mirror_w) { return mirror_w[b]; }

// a joint as the sample has it: with X negated when the sample is a mirrored one (LR: the kernel has the table)
template <bool LR>
__device__ __forceinline__ void load3_lr(const float* p, double v[3], bool left) {
    load3(p, v);
    if (LR && left) v[0] = -v[0];
}

// MIRROR: nothing, or `const int*`, the table mirror_w [B] -- a sample whose entry is W > 0 is the LEFT hand of an image of width
// W, labelled as the right hand of img[:, ::-1]: before anything else K becomes fl32(Kf), Kf = F K M (predict.hip's rule: row 0 <-
// (W - 1) row 2 - row 0, then column 0 negated; float64 from the float32 K -- the product is exact -- and one rounding), and
// joints3d / joints_raw get X negated.  Without the table it is the kernel of before, argument list and code.
template <class... MIRROR>
__global__ __launch_bounds__(LT) void supervised_labels_kernel(const float* __restrict__ K, const float* __restrict__ j3d,
                                                               const double* __restrict__ T, const float* __restrict__ raw_in,
                                                               int B, int use_palm, float* __restrict__ joints,
                                                               float* __restrict__ k_out, float* __restrict__ scale_out,
                                                               float* __restrict__ j3d_out, float* __restrict__ recreated,
                                                               float* __restrict__ raw_out, float* __restrict__ t_out,
                                                               MIRROR... mirror_w) {
    constexpr bool LR = sizeof...(MIRROR) != 0;
    const int lane = threadIdx.x % kWave;
    const int b = blockIdx.x * LS + threadIdx.x / kWave;
    if (b >= B || lane >= LJ) return;
    const size_t at = ((size_t)b * LJ + lane) * 3;
    const float* J = j3d + (size_t)b * LJ * 3;
    const float* R = raw_in ? raw_in + (size_t)b * LJ * 3 : J;
    double k[9], t[9], tf[9], kp[9];
    load9(K + (size_t)b * 9, k);
    const int width = mirror_width(b, mirror_w...);
    const bool left = LR && width > 0;
    if (LR && left) {
#pragma unroll
        for (int c = 0; c < 3; ++c) k[c] = (double)(width - 1) * k[6 + c] - k[c];
        k[0] = -k[0], k[3] = -k[3], k[6] = -k[6];
#pragma unroll
        for (int i = 0; i < 9; ++i) k[i] = (double)(float)k[i];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        t[i] = T[(size_t)b * 9 + i];
        tf[i] = (double)(float)t[i];  // torch.Tensor(transformation_matrix)
    }
    // K' = fl32(T) @ K, rounded: what the stages below read
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            kp[3 * r + c] = (double)(float)(tf[3 * r] * k[c] + tf[3 * r + 1] * k[3 + c] + tf[3 * r + 2] * k[6 + c]);

    double p[3], w[3], c[3], raw[3];
    load3_lr<LR>(J + lane * 3, p, left);
    load3_lr<LR>(J + kParent * 3, w, left);
    load3_lr<LR>(J + kChild * 3, c, left);
    load3_lr<LR>(R + lane * 3, raw, left);

    // joints of this lane's joint, of the wrist and of the index MCP (the root depth needs the last two), and the scale
    double mine[3], n[3], m[3], s;
    if (use_palm) {
        // move_wrist_to_palm, then convert_to_2_5D on the moved (float32) joints with K'
        double r0[3], r2[3];
        load3_lr<LR>(R + kParent * 3, r0, left);
        load3_lr<LR>(R + kChild * 3, r2, left);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            w[i] = (double)(float)((w[i] + c[i]) / 2.0);
            if (lane == kParent) {
                p[i] = w[i];
                raw[i] = (r0[i] + r2[i]) / 2.0;
            }
        }
        s = bone_scale(w, c);
        to_25d(kp, p, w, s, mine);
        to_25d(kp, w, w, s, n);
        to_25d(kp, c, w, s, m);
    } else {
        // convert_to_2_5D with K, then the augmentation matrix
        s = bone_scale(w, c);
        to_25d(k, p, w, s, mine);
        to_25d(k, w, w, s, n);
        to_25d(k, c, w, s, m);
        apply_t(t, mine);
        apply_t(t, n);
        apply_t(t, m);
    }
    store3(joints + at, mine);
    store3(j3d_out + at, p);
    store3(raw_out + at, raw);
    if (lane == 0) scale_out[b] = (float)s;
    if (lane < 9) {
        double k_lane = 0.0, t_lane = 0.0;  // (selected by compares: a lane-indexed read would put the matrices in scratch memory)
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            k_lane = lane == i ? kp[i] : k_lane;
            t_lane = lane == i ? tf[i] : t_lane;
        }
        k_out[(size_t)b * 9 + lane] = (float)k_lane;
        t_out[(size_t)b * 9 + lane] = (float)t_lane;
    }

    // convert_2_5D_to_3D on the emitted joints, scale and K'
    round3(mine);
    round3(n);
    round3(m);
    s = (double)(float)s;
    double inv[9], out[3];
    inverse3(kp, inv);
    to_3d(inv, mine, root_depth(inv, n, m), s, out);
    store3(recreated + at, out);
}

}  // namespace
}  // namespace peclr

using namespace peclr;

extern "C" int peclr_joints3d_to_25d(const float* K, const float* joints3d, int B, float* joints25d, float* scale,
                                     peclr_stream_t stream) {
    if (B <= 0 || !K || !joints3d || !joints25d || !scale) return PECLR_ERR_NULL;
    hipLaunchKernelGGL(joints3d_to_25d_kernel, dim3(grid_of(B)), dim3(LT), 0, static_cast<hipStream_t>(stream), K, joints3d, B,
                       joints25d, scale);
    return launch_status();
}

extern "C" int peclr_joints25d_to_3d(const float* joints25d, const float* scale, const float* K, const float* z_root_calc, int B,
                                     float* joints3d, float* z_root, peclr_stream_t stream) {
    if (B <= 0 || !joints25d || !scale || !K || !joints3d) return PECLR_ERR_NULL;
    hipLaunchKernelGGL(joints25d_to_3d_kernel, dim3(grid_of(B)), dim3(LT), 0, static_cast<hipStream_t>(stream), joints25d, scale, K,
                       z_root_calc, B, joints3d, z_root);
    return launch_status();
}

extern "C" int peclr_supervised_labels(const float* K, const float* joints3d, const double* T, const float* joints_raw, int B,
                                       int use_palm, float* joints, float* k_out, float* scale, float* joints3d_out,
                                       float* joints3d_recreated, float* joints_raw_out, float* t_out, peclr_stream_t stream) {
    if (B <= 0 || !K || !joints3d || !T) return PECLR_ERR_NULL;
    if (!joints || !k_out || !scale || !joints3d_out || !joints3d_recreated || !joints_raw_out || !t_out) return PECLR_ERR_NULL;
    hipLaunchKernelGGL(supervised_labels_kernel<>, dim3(grid_of(B)), dim3(LT), 0, static_cast<hipStream_t>(stream), K, joints3d, T,
                       joints_raw, B, use_palm ? 1 : 0, joints, k_out, scale, joints3d_out, joints3d_recreated, joints_raw_out,
                       t_out);
    return launch_status();
}

extern "C" int peclr_supervised_labels_mirror(const float* K, const float* joints3d, const double* T, const float* joints_raw,
                                              const int* mirror_w, int B, int use_palm, float* joints, float* k_out, float* scale,
                                              float* joints3d_out, float* joints3d_recreated, float* joints_raw_out, float* t_out,
                                              peclr_stream_t stream) {
    if (B <= 0 || !K || !joints3d || !T || !mirror_w) return PECLR_ERR_NULL;
    if (!joints || !k_out || !scale || !joints3d_out || !joints3d_recreated || !joints_raw_out || !t_out) return PECLR_ERR_NULL;
    hipLaunchKernelGGL(supervised_labels_kernel<const int*>, dim3(grid_of(B)), dim3(LT), 0, static_cast<hipStream_t>(stream), K, joints3d,
                       T, joints_raw, B, use_palm ? 1 : 0, joints, k_out, scale, joints3d_out, joints3d_recreated, joints_raw_out,
                       t_out, mirror_w);
    return launch_status();
}
