// The two supervised losses of the 2.5D pose model with their gradients (reference src/models/utils.py: cal_l1_loss :20-50,
// cal_3d_loss :76-104, through convert_2_5D_to_3D / get_root_depth of src/data_loader/utils.py), for a batch.
//
//   forward 1  one wave per sample, LS samples per workgroup, lane j < 21 owns joint j (the layout of labels.hip; the inverse
//              camera matrix and the root depth are every lane's own).  Per sample five UNNORMALISED float64 partial sums
//              (valid; valid |d uv|; valid |d z|; scale x the third; valid |pred3d - joints3d|) go to a [B][5] table, and the
//              unnormalised gradients of the L1 sums (valid x sign) and of the 3D sum (analytic, through the lift and through
//              the closed-form root depth) to two [B][21][3] float64 tensors.  The only value that crosses lanes is a wave sum.
//   forward 2  one workgroup folds the table in a fixed order and writes the four float32 losses and 1 / sum(valid).
//   backward   one launch: upstream gradients (read from the device) x the stored gradients / sum(valid), rounded once.
// A caller that wants the L1 terms or the 3D term alone passes a null truth for the other: that part reads nothing, its sums
// and gradients are zeros.
//
// Float64 from float32 inputs, each emitted float32 tensor rounded once, no atomics: the result depends on no launch geometry
// other than the fold's fixed order.  Contraction is off, as in labels.hip, whose root_depth() this reuses as it is.
#include "labels.hpp"  // the wave layout; load3 / load9, inverse3, root_depth, to_3d, clamp_min

#pragma clang fp contract(off)

namespace peclr {
namespace {

constexpr int FT = 256;  // threads of the fold and of a backward workgroup

// nn.L1Loss's backward: sign(0) = 0
__device__ __forceinline__ double sign_of(double x) { return (double)((x > 0.0) - (x < 0.0)); }
// torch.clamp(x, min = lo)'s backward: the gradient passes where x >= lo (a value AT the minimum passes it; a NaN does not)
__device__ __forceinline__ double pass_min(double x, double lo, double g) { return x >= lo ? g : 0.0; }

// d root_depth / d (u, v, z) of the wrist n (dn) and of the index MCP m (dm).  The forward terms are root_depth()'s, in its
// operation order.  With ac = clamp(a), Dc = clamp(D), D = b^2 - 4 a c and Z = 0.5 (-b + sqrt(Dc)) / ac:
//   dZ/dDc = 0.25 / (sqrt(Dc) ac), dZ/dac = -Z / ac, and through the clamps (pass_min)
//   gD = [D >= 1e-6] dZ/dDc;  ga = [a >= 1e-6] dZ/dac - 4 c gD;  gb = -0.5 / ac + 2 b gD;  gc = -4 a gD.
// gb's first term does not go through a clamp: with both clamps active Z still falls by 0.5 / 1e-6 per unit of b.
__device__ __forceinline__ void root_depth_grad(const double inv[9], const double n[3], const double m[3], double dn[3],
                                                double dm[3]) {
    const double xn = inv[0] * n[0] + inv[1] * n[1] + inv[2], yn = inv[3] * n[0] + inv[4] * n[1] + inv[5];
    const double xm = inv[0] * m[0] + inv[1] * m[1] + inv[2], ym = inv[3] * m[0] + inv[4] * m[1] + inv[5];
    const double zn = n[2], zm = m[2];
    const double a = (xn - xm) * (xn - xm) + (yn - ym) * (yn - ym);
    const double P = xn * xn + yn * yn - xn * xm - yn * ym, Q = xm * xm + ym * ym - xn * xm - yn * ym;
    const double b = 2.0 * (zn * P + zm * Q);
    const double ex = xn * zn - xm * zm, ey = yn * zn - ym * zm, ez = zn - zm;
    const double c = ex * ex + ey * ey + ez * ez - 1.0;
    const double D = b * b - 4.0 * a * c;
    const double ac = clamp_min(a, 1e-6), root = sqrt(clamp_min(D, 1e-6));
    const double Z = 0.5 * (-b + root) / ac;

    const double gD = pass_min(D, 1e-6, 0.25 / (root * ac));
    const double ga = pass_min(a, 1e-6, -Z / ac) - 4.0 * c * gD;
    const double gb = -0.5 / ac + 2.0 * b * gD;
    const double gc = -4.0 * a * gD;

    const double gxn = ga * (2.0 * (xn - xm)) + gb * (2.0 * (zn * (2.0 * xn - xm) - zm * xm)) + gc * (2.0 * ex * zn);
    const double gyn = ga * (2.0 * (yn - ym)) + gb * (2.0 * (zn * (2.0 * yn - ym) - zm * ym)) + gc * (2.0 * ey * zn);
    const double gxm = ga * (-2.0 * (xn - xm)) + gb * (2.0 * (zm * (2.0 * xm - xn) - zn * xn)) + gc * (-2.0 * ex * zm);
    const double gym = ga * (-2.0 * (yn - ym)) + gb * (2.0 * (zm * (2.0 * ym - yn) - zn * yn)) + gc * (-2.0 * ey * zm);
    dn[0] = gxn * inv[0] + gyn * inv[3];
    dn[1] = gxn * inv[1] + gyn * inv[4];
    dn[2] = gb * (2.0 * P) + gc * (2.0 * (ex * xn + ey * yn + ez));
    dm[0] = gxm * inv[0] + gym * inv[3];
    dm[1] = gxm * inv[1] + gym * inv[4];
    dm[2] = gb * (2.0 * Q) + gc * (-2.0 * (ex * xm + ey * ym + ez));
}

__global__ __launch_bounds__(LT) void pose_loss_partials_kernel(const float* __restrict__ pred, const float* __restrict__ joints,
                                                                const float* __restrict__ j3d, const float* __restrict__ scale,
                                                                const float* __restrict__ K, const float* __restrict__ valid,
                                                                const float* __restrict__ z_root_calc, int B,
                                                                double* __restrict__ part, double* __restrict__ g_l1,
                                                                double* __restrict__ g_3d, double* __restrict__ g_zroot) {
    const int lane = threadIdx.x % kWave;
    const int b = blockIdx.x * LS + threadIdx.x / kWave;
    if (b >= B) return;  // (the whole wave: the lanes past joint 20 stay for the wave sums)
    const bool own = lane < LJ;
    const int j = own ? lane : 0;
    const size_t at = ((size_t)b * LJ + j) * 3;
    const float* P = pred + (size_t)b * LJ * 3;
    double p[3], t[3];
    load3(P + j * 3, p);
    if (joints)
        load3(joints + at, t);
    else  // no 2.5D truth: the L1 terms compare pred with itself and vanish
        load3(P + j * 3, t);
    const double s = (double)scale[b];
    const double v = valid ? (double)valid[(size_t)b * LJ + j] : 1.0;

    // ---- the L1 sums and their gradients
    double d[3], sl[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        d[c] = p[c] - t[c];
        sl[c] = v * sign_of(d[c]);
    }
    const double uv = v * fabs(d[0]) + v * fabs(d[1]), z = v * fabs(d[2]);

    const double n_valid = wave_sum(own ? v : 0.0);
    const double sum_uv = wave_sum(own ? uv : 0.0);
    const double sum_z = wave_sum(own ? z : 0.0);

    // ---- the 3D sum; its gradient through (inv (u, v, 1)) (z + Z_root) scale of this lane's joint
    double g3[3] = {0.0, 0.0, 0.0}, sum_3d = 0.0;
    if (j3d) {  // (uniform over the launch)
        double k[9], inv[9], n[3], m[3], g[3], out[3];
        load9(K + (size_t)b * 9, k);
        load3(P + kParent * 3, n);
        load3(P + kChild * 3, m);
        load3(j3d + at, g);
        inverse3(k, inv);
        const double zr = z_root_calc ? (double)z_root_calc[b] : root_depth(inv, n, m);
        to_3d(inv, p, zr, s, out);
        double s3[3], ray[3], l3 = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double e = out[r] - g[r];
            s3[r] = v * sign_of(e);
            l3 += v * fabs(e);
            ray[r] = inv[3 * r] * p[0] + inv[3 * r + 1] * p[1] + inv[3 * r + 2];
        }
        const double depth = (p[2] + zr) * s;
        g3[0] = (s3[0] * inv[0] + s3[1] * inv[3] + s3[2] * inv[6]) * depth;
        g3[1] = (s3[0] * inv[1] + s3[1] * inv[4] + s3[2] * inv[7]) * depth;
        g3[2] = (s3[0] * ray[0] + s3[1] * ray[1] + s3[2] * ray[2]) * s;
        sum_3d = wave_sum(own ? l3 : 0.0);
        const double g_root = wave_sum(own ? g3[2] : 0.0);  // d / d Z_root: every joint's depth moves with it
        if (z_root_calc) {
            if (lane == 0 && g_zroot) g_zroot[b] = g_root;
        } else {
            // ... and through Z_root(pred[0], pred[2]): the wrist's and the index MCP's lanes
            double dn[3], dm[3];
            root_depth_grad(inv, n, m, dn, dm);
#pragma unroll
            for (int c = 0; c < 3; ++c) g3[c] += lane == kParent ? g_root * dn[c] : (lane == kChild ? g_root * dm[c] : 0.0);
        }
    }
    if (own) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            g_l1[at + c] = sl[c];
            g_3d[at + c] = g3[c];
        }
    }
    if (lane == 0) {
        double* row = part + (size_t)b * 5;
        row[0] = n_valid;
        row[1] = sum_uv;
        row[2] = sum_z;
        row[3] = s * sum_z;
        row[4] = sum_3d;
    }
}

// ONE workgroup: thread t adds rows t, t + FT, ... in order, then a binary tree over the threads.
__global__ __launch_bounds__(FT) void pose_loss_fold_kernel(const double* __restrict__ part, int B, float* __restrict__ losses,
                                                            double* __restrict__ inv_valid) {
    __shared__ double red[5][FT];
    const int t = threadIdx.x;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = t; r < B; r += FT)
#pragma unroll
        for (int i = 0; i < 5; ++i) acc[i] += part[(size_t)r * 5 + i];
#pragma unroll
    for (int i = 0; i < 5; ++i) red[i][t] = acc[i];
    __syncthreads();
    for (int o = FT / 2; o > 0; o >>= 1) {
        if (t < o)
#pragma unroll
            for (int i = 0; i < 5; ++i) red[i][t] += red[i][t + o];
        __syncthreads();
    }
    if (t == 0) {
        const double nv = red[0][0];  // 0 valid joints: 0 / 0, NaN losses as in the reference
        losses[0] = (float)(red[1][0] / nv / 2.0);
        losses[1] = (float)(red[2][0] / nv);
        losses[2] = (float)(red[3][0] / nv);
        losses[3] = (float)(red[4][0] / nv / 3.0);
        *inv_valid = 1.0 / nv;
    }
}

__global__ __launch_bounds__(FT) void pose_loss_bwd_kernel(const float* __restrict__ up, const double* __restrict__ g_l1,
                                                           const double* __restrict__ g_3d, const double* __restrict__ g_zroot,
                                                           const float* __restrict__ scale, const double* __restrict__ inv_valid,
                                                           int B, float* __restrict__ grad_pred, float* __restrict__ grad_zroot) {
    const long long i = (long long)blockIdx.x * FT + threadIdx.x;  // one joint
    if (i >= (long long)B * LJ) return;
    const int b = (int)(i / LJ);
    const double inv_n = *inv_valid;
    const double w_uv = (double)up[0] / 2.0, w_z = (double)up[1] + (double)up[2] * (double)scale[b], w_3d = (double)up[3] / 3.0;
    const size_t at = (size_t)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        grad_pred[at + c] = (float)((c < 2 ? w_uv : w_z) * g_l1[at + c] * inv_n + w_3d * g_3d[at + c] * inv_n);
    if (grad_zroot && i % LJ == 0) grad_zroot[b] = (float)(w_3d * g_zroot[b] * inv_n);
}

}  // namespace
}  // namespace peclr

using namespace peclr;

extern "C" int peclr_pose_loss(const float* pred, const float* joints, const float* joints3d, const float* scale, const float* K,
                               const float* joints_valid, const float* z_root_calc, int B, double* partials, double* g_l1,
                               double* g_3d, double* g_zroot, float* losses, double* inv_valid, peclr_stream_t stream) {
    if (B <= 0 || !pred || !scale || (!joints && !joints3d) || (joints3d && !K)) return PECLR_ERR_NULL;
    if (!partials || !g_l1 || !g_3d || !losses || !inv_valid) return PECLR_ERR_NULL;
    hipLaunchKernelGGL(pose_loss_partials_kernel, dim3(grid_of(B)), dim3(LT), 0, static_cast<hipStream_t>(stream), pred, joints,
                       joints3d, scale, K, joints_valid, z_root_calc, B, partials, g_l1, g_3d, g_zroot);
    const int rc = launch_status();
    if (rc != PECLR_OK) return rc;
    hipLaunchKernelGGL(pose_loss_fold_kernel, dim3(1), dim3(FT), 0, static_cast<hipStream_t>(stream), partials, B, losses,
                       inv_valid);
    return launch_status();
}

extern "C" int peclr_pose_loss_bwd(const float* grad_losses, const double* g_l1, const double* g_3d, const double* g_zroot,
                                   const float* scale, const double* inv_valid, int B, float* grad_pred, float* grad_z_root_calc,
                                   peclr_stream_t stream) {
    if (B <= 0 || !grad_losses || !g_l1 || !g_3d || !scale || !inv_valid || !grad_pred) return PECLR_ERR_NULL;
    if (grad_z_root_calc && !g_zroot) return PECLR_ERR_NULL;
    const long long blocks = ((long long)B * LJ + FT - 1) / FT;
    hipLaunchKernelGGL(pose_loss_bwd_kernel, dim3((unsigned)blocks), dim3(FT), 0, static_cast<hipStream_t>(stream), grad_losses,
                       g_l1, g_3d, g_zroot, scale, inv_valid, B, grad_pred, grad_z_root_calc);
    return launch_status();
}
