// Scoring pose predictions on the device (reference src/experiments/evaluation_utils.py): calculate_epe_statistics'
// per-joint Euclidean distance, calc_procrustes_transform and the counts behind get_pck_curves, for a batch, in one launch.
//
//   pose_eval_kernel  one wave per sample, ES samples per workgroup.
//                     stage 1  lane j < 21 loads joint j of the prediction and the ground truth, widens it to float64, leaves
//                              it in LDS and writes the raw distance (rounded once to the input dtype);
//                     stage 2  every lane of the wave runs the SAME serial float64 fit of procrustes.hpp on the wave's two
//                              clouds (LDS broadcast reads; a wave costs what one lane costs, and no lane has to hand its
//                              result to another), lane j < 21 transforms joint j and writes it and its aligned distance,
//                              lanes 0..8 / 0..2 / 0 write R, the translation, the scale and the status bits;
//                     stage 3  PCK: thread i of the workgroup owns (set, joint, threshold) triples i, i + ET, ...: it counts
//                              the workgroup's rounded distances (kept in LDS by stages 1 and 2) under the threshold and adds
//                              the count to counts[set][joint][k] with ONE 64-bit integer atomic.
//
// A sample's outputs depend on that sample alone and on no schedule: the joint sums run in a fixed order inside one lane,
// there are no floating-point atomics, and integer addition does not care in which order workgroups arrive.  The work is
// tiny (B = 128: 16 KiB in, a few hundred float64 operations per sample); like pose_head_kernel the point is one launch, no
// intermediate tensors, no host round trip and no LAPACK call -- so a prediction loop can score each batch inside its hipGraph.
#include "common.hpp"
#include "procrustes.hpp"

#pragma clang fp contract(off)

namespace peclr {
namespace {

constexpr int ES = 8;  // samples (waves) per workgroup: 16 workgroups' worth of count atomics at B = 128
constexpr int ET = ES * kWave;
constexpr int EJ = procrustes::kJoints;

template <typename T>
__global__ __launch_bounds__(ET) void pose_eval_kernel(const T* __restrict__ pred, const T* __restrict__ gt, int B, int dim,
                                                       T* __restrict__ dist, T* __restrict__ aligned, T* __restrict__ rot,
                                                       T* __restrict__ scale, T* __restrict__ trans,
                                                       T* __restrict__ dist_aligned, const T* __restrict__ thr, int n_thr,
                                                       unsigned long long* __restrict__ counts, int* __restrict__ status,
                                                       int* cursor, int capacity, int with_fit) {
    __shared__ double sx[ES][EJ][3], sy[ES][EJ][3];  // ground truth (X) and prediction (Y), float64
    __shared__ T sd[2][ES][EJ];                      // the distances as written out: raw, aligned
    __shared__ int s_row0;
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int b = blockIdx.x * ES + wave;
    const bool live = b < B;

    // streaming form: rows of dist / dist_aligned / status start at the device cursor, which this launch advances (below)
    if (tid == 0) s_row0 = cursor ? cursor[0] : 0;
    __syncthreads();
    const int row0 = s_row0;
    const bool fits = !cursor || (row0 >= 0 && (long long)row0 + B <= (long long)capacity);  // same answer in every workgroup

    if (fits) {
        const size_t row = (size_t)row0 + (size_t)(live ? b : 0);
        bool nan = false;
        if (live && lane < EJ) {
            double p[3], g[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                p[c] = (double)pred[((size_t)b * EJ + lane) * 3 + c];
                g[c] = (double)gt[((size_t)b * EJ + lane) * 3 + c];
                if (c < dim) nan = nan || p[c] != p[c] || g[c] != g[c];
                sx[wave][lane][c] = g[c];
                sy[wave][lane][c] = p[c];
            }
            const T d = (T)procrustes::joint_distance(p, g, dim);
            dist[row * EJ + lane] = d;
            sd[0][wave][lane] = d;
        }
        int bits = __any(nan) ? PECLR_POSE_STATUS_NAN : 0;
        __syncthreads();

        if (live && with_fit) {
            procrustes::Fit f;
            if (!procrustes::fit(sx[wave], sy[wave], EJ, f)) bits |= PECLR_POSE_EVAL_DEGENERATE;
            if (lane < EJ) {
                double out[3];
                procrustes::transform_point(f, sy[wave][lane], out);
                T o[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    o[c] = (T)out[c];
                    if (aligned) aligned[((size_t)b * EJ + lane) * 3 + c] = o[c];
                }
                // the EPE of `aligned` against gt as a second calculate_epe_statistics call sees it: from the ROUNDED cloud
                const double a[3] = {(double)o[0], (double)o[1], (double)o[2]};
                const T d = (T)procrustes::joint_distance(a, sx[wave][lane], 3);
                if (dist_aligned) dist_aligned[row * EJ + lane] = d;
                sd[1][wave][lane] = d;
            }
            double r_lane = 0.0, t_lane = 0.0;  // (selected by compares: a lane-indexed read would keep the whole fit in scratch memory)
#pragma unroll
            for (int i = 0; i < 9; ++i) r_lane = lane == i ? f.R[i / 3][i % 3] : r_lane;
#pragma unroll
            for (int i = 0; i < 3; ++i) t_lane = lane == i ? f.t[i] : t_lane;
            if (rot && lane < 9) rot[(size_t)b * 9 + lane] = (T)r_lane;
            if (trans && lane < 3) trans[(size_t)b * 3 + lane] = (T)t_lane;
            if (scale && lane == 0) scale[b] = (T)f.scale;
        }
        if (live && lane == 0 && bits) status[row] |= bits;
        __syncthreads();

        if (n_thr > 0) {
            const int n_live = min(ES, B - (int)blockIdx.x * ES);
            const int per_set = EJ * n_thr, total = (with_fit ? 2 : 1) * per_set;
            for (int i = tid; i < total; i += ET) {
                const int set = i / per_set, j = (i % per_set) / n_thr;
                const T th = thr[i % n_thr];
                unsigned c = 0;
                for (int s = 0; s < n_live; ++s) c += sd[set][s][j] < th ? 1u : 0u;  // NaN: not under
                if (c) atomicAdd(&counts[i], (unsigned long long)c);
            }
        }
    }

    // (Launches that share a cursor must be ordered on ONE stream: two in flight at once would read the same cursor[0] and
    // draw tickets from the same counter.)
    // The last workgroup to get here advances the cursor: every workgroup read cursor[0] before it took its ticket, so the
    // write cannot overtake a read.  cursor[1] is the ticket counter and is left at 0.  A launch that does not fit writes
    // nothing but still advances, so that the host sees cursor[0] > capacity at its next read.
    if (cursor) {
        __syncthreads();
        if (tid == 0) {
            __threadfence();
            const int ticket = atomicAdd(&cursor[1], 1);
            if (ticket == (int)gridDim.x - 1) {
                cursor[1] = 0;
                cursor[0] = row0 < 0 || row0 > capacity ? row0 : row0 + B;
                __threadfence();
            }
        }
    }
}

template <typename T>
int launch(const void* pred, const void* gt, int B, int dim, void* dist, void* aligned, void* rot, void* scale, void* trans,
           void* dist_aligned, const void* thr, int n_thr, long long* counts, int* status, int* cursor, int capacity,
           int with_fit, hipStream_t stream) {
    const int grid = (B + ES - 1) / ES;
    hipLaunchKernelGGL(pose_eval_kernel<T>, dim3(grid), dim3(ET), 0, stream, static_cast<const T*>(pred),
                       static_cast<const T*>(gt), B, dim, static_cast<T*>(dist), static_cast<T*>(aligned), static_cast<T*>(rot),
                       static_cast<T*>(scale), static_cast<T*>(trans), static_cast<T*>(dist_aligned), static_cast<const T*>(thr),
                       n_thr, reinterpret_cast<unsigned long long*>(counts), status, cursor, capacity, with_fit);
    return launch_status();
}

}  // namespace
}  // namespace peclr

using namespace peclr;

extern "C" int peclr_pose_eval(const void* pred, const void* gt, int B, int dtype, int dim, void* dist, void* aligned, void* rot,
                               void* scale, void* trans, void* dist_aligned, const void* thr, int n_thr, long long* counts,
                               int* status, int* cursor, int capacity, peclr_stream_t stream) {
    // every argument error of this entry point is PECLR_ERR_NULL (-1), before any launch
    if (B <= 0 || !pred || !gt || !dist || !status) return PECLR_ERR_NULL;
    if (dtype != PECLR_DTYPE_F32 && dtype != PECLR_DTYPE_F64) return PECLR_ERR_NULL;
    if (dim != 2 && dim != 3) return PECLR_ERR_NULL;
    const int with_fit = aligned || rot || scale || trans || dist_aligned;
    if (dim == 2 && with_fit) return PECLR_ERR_NULL;
    if (n_thr < 0 || (n_thr > 0 && (!thr || !counts))) return PECLR_ERR_NULL;
    if (cursor && (capacity <= 0 || B > capacity)) return PECLR_ERR_NULL;
    if (n_thr > (1 << 20)) return PECLR_ERR_NULL;  // 2 * 21 * n_thr stays far inside int
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == PECLR_DTYPE_F32
               ? launch<float>(pred, gt, B, dim, dist, aligned, rot, scale, trans, dist_aligned, thr, n_thr, counts, status,
                               cursor, capacity, with_fit, s)
               : launch<double>(pred, gt, B, dim, dist, aligned, rot, scale, trans, dist_aligned, thr, n_thr, counts, status,
                                cursor, capacity, with_fit, s);
}
