// Two-view augmentation, PARAMETER side on the device (include/peclr_hip.h, peclr_augment_draw_views): what
// TwoViewAugmenter.sample_view (peclr_amd/augment.py; reference src/data_loader/sample_augmenter.py:47-129) computes per
// (view, sample) for the recipe flags -- the uniforms, the angle, the rotation centre, the forward and inverse 2x3 matrices, the
// rotated joints, the crop window with margin and jitter, jitter_x / jitter_y, h / s / a / b -- for a whole batch in ONE launch.
//
//   draw_views_kernel<T>   one thread per sample, its views in turn; T the joints' element type (float64 is rounded to
//                          float32 first).
//
// Arithmetic is sample_view's in its own types: float32 where it works on float32 torch tensors (the joints' means, `far`,
// far ** 0.5 * margin, the rounding of the rotated joints), float64 where it uses Python floats (uniform(a, b), the angle and
// `// 1`, the rotation matrix and its inverse, int() truncation toward zero).  Floating-point contraction is off everywhere:
// products and sums round separately, as they do on the host.
//
// Random numbers: Philox4x32-10 keyed by the seed, counter (sample, 4 * view + k, call low word, call high word), k = 0..3;
// call k gives uniform slots 2k (words x, y) and 2k + 1 (words z, w), each Python's random() construction
// ((a >> 5) * 2^26 + (b >> 6)) / 2^53.  The draws of (view, sample) depend on nothing but (seed, call, view, sample).
//
// `call` lives on the device: every workgroup reads it first, and the last one to finish advances it (a ticket, the cursor
// pattern of pose_eval.hip), so a launch recorded into a hipGraph draws afresh on every replay.  Launches that share a counter
// must be ordered on one stream.
#include "affine.hpp"
#include "common.hpp"

namespace peclr {
namespace {

constexpr int DT = kWave;  // threads per workgroup
constexpr int DJ = 21;     // joints
constexpr int NP = PECLR_AUG_PARAM_DOUBLES, NU = PECLR_AUG_DRAW_UNIFORMS, NS = PECLR_AUG_DRAW_SCALARS;

struct DrawRanges {  // include/peclr_hip.h: the `ranges` layout
    double v[PECLR_AUG_DRAW_RANGES];
};
enum { kAngleA = 0, kAngleB, kMarginLo, kMarginHi, kMargin, kJitterHi, kHLo, kHHi, kSLo, kSHi, kALo, kAHi, kBLo, kBHi };
enum { kUAngle = 0, kUMargin, kUJitterX, kUJitterY, kUH, kUS, kUA, kUB };

// Philox4x32-10 (Salmon et al., SC'11); the ten rounds of augment.hip's noise stage
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    }
    return c;
}

// Python's random(): 53 bits from two 32-bit words, exact in float64
__device__ __forceinline__ double unit_double(uint32_t a, uint32_t b) {
#pragma clang fp contract(off)
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// Python's uniform(a, b)
__device__ __forceinline__ double uniform(double a, double b, double u) {
#pragma clang fp contract(off)
    return a + (b - a) * u;
}

// int() of a float: toward zero.  NaN gives 0 and the magnitude stays below 2^40, so that the integer arithmetic after it
// cannot overflow (the host raises or makes an empty window there; here the window is clamped and counted).
__device__ __forceinline__ long long trunc_ll(double f) {
    if (f != f) return 0;
    return (long long)fmin(fmax(f, -1099511627776.0), 1099511627776.0);
}

// _crop_size's centre: int(mean) of the joints' y and x, the means in float32
__device__ __forceinline__ void joints_center(const float (&x)[DJ], const float (&y)[DJ], long long& cx, long long& cy) {
#pragma clang fp contract(off)
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int j = 0; j < DJ; ++j) sx += x[j], sy += y[j];
    cx = trunc_ll((double)(sx / (float)DJ));
    cy = trunc_ll((double)(sy / (float)DJ));
}

// _crop_size's side: int(far ** 0.5 * margin), all float32 (the margin rounds to float32 when it meets the tensor)
__device__ __forceinline__ long long crop_side(const float (&x)[DJ], const float (&y)[DJ], long long cx, long long cy, double margin) {
#pragma clang fp contract(off)
    const float fcx = (float)cx, fcy = (float)cy;
    float far = 0.f;
#pragma unroll
    for (int j = 0; j < DJ; ++j) {
        const float dy = y[j] - fcy, dx = x[j] - fcx;
        const float d = dy * dy + dx * dx;
        far = (j == 0 || d > far || d != d) ? d : far;  // torch.max: NaN wins
    }
    return trunc_ll((double)(sqrtf(far) * (float)margin));
}

template <typename T>
__global__ __launch_bounds__(DT) void draw_views_kernel(const T* __restrict__ joints, int B, int n_views, int H, int W,
                                                        const long long* __restrict__ geom, const int* __restrict__ mirror,
                                                        int flags, DrawRanges rg, uint32_t key0, uint32_t key1,
                                                        unsigned long long* call, int* counters, double* __restrict__ params,
                                                        double* __restrict__ scalars, long long* __restrict__ jitter,
                                                        double* __restrict__ uniforms) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_call;
    const int tid = threadIdx.x;
    if (tid == 0) s_call = call[0];
    __syncthreads();
    const unsigned long long c = s_call;
    const int i = blockIdx.x * DT + tid;  // sample
    bool empty = false;

    for (int v = 0; i < B && v < n_views; ++v) {
        const int n = v * B + i;
        if (geom) H = (int)geom[(size_t)i * PECLR_AUG_GEOM_INT64S + 1], W = (int)geom[(size_t)i * PECLR_AUG_GEOM_INT64S + 2];

        double u[NU];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 r = philox4x32_10(make_uint4((uint32_t)i, (uint32_t)(4 * v + k), (uint32_t)c, (uint32_t)(c >> 32)), key0, key1);
            u[2 * k] = unit_double(r.x, r.y);
            u[2 * k + 1] = unit_double(r.z, r.w);
        }
        if (uniforms) {
#pragma unroll
            for (int s = 0; s < NU; ++s) uniforms[(size_t)n * NU + s] = u[s];
        }

        // the joints as sample_view holds them: float32, a left hand's x <- W - x first (sample_batch's rule)
        float x[DJ], y[DJ];
        const bool left = mirror && mirror[i] != 0;
        const T* src = joints + (size_t)i * DJ * 3;
#pragma unroll
        for (int j = 0; j < DJ; ++j) {
            x[j] = (float)src[j * 3], y[j] = (float)src[j * 3 + 1];
            if (left) x[j] = (float)W - x[j];
        }

        double* p = params + (size_t)n * NP;
        double angle = 0.0;
        if (flags & PECLR_AUG_DRAW_ROTATE) {
            // centre: _crop_size with a zero margin and jitter -- side 0, origin max(centre, 0)
            long long cx, cy;
            joints_center(x, y, cx, cy);
            const double rcx = (double)max(cx, 0ll), rcy = (double)max(cy, 0ll);
            angle = floor(uniform(rg.v[kAngleA], rg.v[kAngleB], u[kUAngle]));  // `// 1`
            const double a = angle * 3.141592653589793 / 180.0;
            const double al = cos(a), be = sin(a);
            const double rot[6] = {al, be, (1.0 - al) * rcx - be * rcy, -be, al, be * rcx + (1.0 - al) * rcy};
#pragma unroll
            for (int j = 0; j < DJ; ++j) {  // (hom @ rot.T).float()
                const double X = (double)x[j], Y = (double)y[j];
                x[j] = (float)(X * rot[0] + Y * rot[1] + rot[2]);
                y[j] = (float)(X * rot[3] + Y * rot[4] + rot[5]);
            }
            invert_affine(rot, p);
            p[6] = 1.0;
        } else {
            p[0] = 1.0, p[1] = 0.0, p[2] = 0.0, p[3] = 0.0, p[4] = 1.0, p[5] = 0.0, p[6] = 0.0;
        }

        const double margin = (flags & PECLR_AUG_DRAW_RANDOM_CROP) ? uniform(rg.v[kMarginLo], rg.v[kMarginHi], u[kUMargin]) : rg.v[kMargin];
        long long jx = 0, jy = 0;
        if (flags & PECLR_AUG_DRAW_CROP) {
            jx = trunc_ll(uniform(0.0, rg.v[kJitterHi], u[kUJitterX]));
            jy = trunc_ll(uniform(0.0, rg.v[kJitterHi], u[kUJitterY]));
        }
        long long cx, cy;
        joints_center(x, y, cx, cy);
        const long long side = crop_side(x, y, cx, cy, margin);
        const long long ox = max(cx - side + jx, 0ll), oy = max(cy - side + jy, 0ll);
        long long x0 = min(ox, (long long)W), y0 = min(oy, (long long)H);
        long long cw = min(ox + 2 * side, (long long)W) - x0, ch = min(oy + 2 * side, (long long)H) - y0;
        if (cw <= 0 || ch <= 0) {
            // the host raises here.  The 1 x 1 window at the nearest pixel inside the image: no pixel stage reads outside
            x0 = max(min(ox, (long long)W - 1), 0ll), y0 = max(min(oy, (long long)H - 1), 0ll);
            cw = ch = 1;
            empty = true;
        }
        p[7] = (double)x0, p[8] = (double)y0, p[9] = (double)cw, p[10] = (double)ch;

        double h = 1.0, s = 1.0, va = 1.0, vb = 0.0;
        if (flags & PECLR_AUG_DRAW_COLOR_JITTER) {
            h = uniform(rg.v[kHLo], rg.v[kHHi], u[kUH]);
            s = uniform(rg.v[kSLo], rg.v[kSHi], u[kUS]);
            va = uniform(rg.v[kALo], rg.v[kAHi], u[kUA]);
            vb = uniform(rg.v[kBLo], rg.v[kBHi], u[kUB]);
            p[11] = 1.0;
        } else {
            p[11] = 0.0;
        }
        p[12] = h, p[13] = s, p[14] = va, p[15] = vb;

        // the collated entries: [view][field][sample], so that each is one contiguous [B]
        double* sc = scalars + (size_t)v * NS * B + i;
        sc[0] = angle, sc[(size_t)B] = margin, sc[(size_t)2 * B] = h, sc[(size_t)3 * B] = s, sc[(size_t)4 * B] = va, sc[(size_t)5 * B] = vb;
        long long* jt = jitter + (size_t)v * 2 * B + i;
        jt[0] = cx - side - ox, jt[(size_t)B] = cy - side - oy;
    }
    if (empty) atomicAdd(&counters[0], 1);  // per SAMPLE: the host raises once for it, at its first empty view

    // The last workgroup to get here advances the counter: every workgroup read call[0] before it took its ticket, so the
    // write cannot overtake a read.  counters[1] is the ticket counter and is left at 0.
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        const int ticket = atomicAdd(&counters[1], 1);
        if (ticket == (int)gridDim.x - 1) {
            counters[1] = 0;
            call[0] = c + 1;
            __threadfence();
        }
    }
}

}  // namespace
}  // namespace peclr

using namespace peclr;

extern "C" int peclr_augment_draw_views(const void* joints, int joints_dtype, int B, int n_views, int H, int W, const int64_t* geom,
                                        const int* mirror, int flags, const double* ranges, uint64_t seed, uint64_t* call,
                                        int* counters, double* params, double* scalars, int64_t* jitter, double* uniforms,
                                        peclr_stream_t stream) {
    if (!joints || !ranges || !call || !counters || !params || !scalars || !jitter) return PECLR_ERR_NULL;
    if (B < 1 || B > 32767 || (n_views != 1 && n_views != 2)) return PECLR_ERR_SHAPE;
    if (!geom && (H < 1 || W < 1)) return PECLR_ERR_SHAPE;
    if (!(flags & PECLR_AUG_DRAW_RESIZE) || (flags & ~PECLR_AUG_DRAW_ALL)) return PECLR_ERR_UNSUPPORTED;
    if (joints_dtype != PECLR_DTYPE_F32 && joints_dtype != PECLR_DTYPE_F64) return PECLR_ERR_UNSUPPORTED;
    DrawRanges rg;
    for (int k = 0; k < PECLR_AUG_DRAW_RANGES; ++k) rg.v[k] = ranges[k];  // host pointer, passed by value to the kernel
    const dim3 grid((B + DT - 1) / DT);
    const uint32_t key0 = (uint32_t)seed, key1 = (uint32_t)(seed >> 32);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long* g = reinterpret_cast<const long long*>(geom);
    unsigned long long* cl = reinterpret_cast<unsigned long long*>(call);
    long long* jt = reinterpret_cast<long long*>(jitter);
    if (joints_dtype == PECLR_DTYPE_F32)
        hipLaunchKernelGGL(draw_views_kernel<float>, grid, dim3(DT), 0, s, static_cast<const float*>(joints), B, n_views, H, W, g,
                           mirror, flags, rg, key0, key1, cl, counters, params, scalars, jt, uniforms);
    else
        hipLaunchKernelGGL(draw_views_kernel<double>, grid, dim3(DT), 0, s, static_cast<const double*>(joints), B, n_views, H, W, g,
                           mirror, flags, rg, key0, key1, cl, counters, params, scalars, jt, uniforms);
    return launch_status();
}
