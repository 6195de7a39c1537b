// Weight gradients of the 16-bit (bf16 / fp16 autocast) 1x1 convolutions:  dW[Cout][Cin] (fp32) = sum over pixels r of
// dY[r][co] * X[r][ci]  -- the contraction runs over the ROWS of two NHWC activations (channels contiguous), so both MFMA
// operands have to be transposed on their way into the matrix cores.  gfx950 does that in the LDS read:
//   * both operands stream global -> LDS by LDS-DMA exactly as they lie in memory (16 pixels x 64 bytes per
//     `lds_dma16`, four lanes per pixel), into the image [32-channel block][pixel][64 B];
//   * `ds_read_b64_tr_b16` hands lane l of a 16-lane group the elements src[(l >> 2) + 4 j][l & 3], j = 0..3, of the 8-byte
//     words its sixteen lanes address: with source lane r pointing at pixel k0 + (r >> 2), channels 4 (r & 3) .. + 3, lane
//     l receives channel l of pixels k0 .. k0 + 3 -- two such reads are the 8-k fragment of v_mfma_f32_32x32x16 (4 consecutive
//     pixels of a 32-channel block are 256 contiguous bytes: all 64 banks once, conflict-free at any pixel offset);
// no VGPR staging, no VALU transposes, no ds_write.  fp32 accumulators go to one fp32 slab per K split
// (peclr_slab_reduce_f32 adds the slabs in a fixed order: deterministic, and the result is the fp32 gradient of the fp32
// master weight -- MIOpen's 16-bit weight gradients need a zero-fill, atomics and a cast back).
// These products are HBM-bound (layer1: 800 k pixels x 320 channels in, 64 KiB out): what counts is bytes in flight --
// two stages of 16 - 20 KiB per workgroup (32 - 40 KiB of LDS), four workgroups per CU (three stages at two to three
// workgroups per CU measured the same or slower: tools/exp/wgrad_h_probe.py).
#include <stdlib.h>

#include "mfma.hpp"

namespace peclr {
namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int WK = 32;                   // pixels per k-step

struct WArgs {
    const h16_t* A;                      // dY [K rows][lda], M = Cout channels
    const h16_t* B;                      // X  [K (or 4 K for stride 2) rows][ldb], N = Cin channels
    float* slabs;                        // [n_slabs][M][ldc]
    int M, N, K, lda, ldb, ldc;
    int kchunk;                          // rows per slab (multiple of WK)
    int stride, Ho, Wo;                  // stride 2: A's rows are the Ho x Wo output pixels, B's row of output pixel (img, oh, ow)
                                         // is input pixel (img, 2 oh, 2 ow) of the 2 Ho x 2 Wo image
    const h16_t* zeros;                  // >= 64 bytes of zeros (rows past K)
};

template <bool F16>
__device__ __forceinline__ f32x16 wmma(const uint4& a, const uint4& b, f32x16 acc) {
    if constexpr (F16) return mma_f16(a, b, acc);
    else return mma_bf16(a, b, acc);
}

// 8 consecutive k (pixels) of one channel per lane out of the pixel-major image: two transposing reads
__device__ __forceinline__ uint4 tr_frag(const unsigned char* base) {
    typedef __attribute__((address_space(3))) s16x4* lp;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(base));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(base + 4 * 64));     // pixels + 4
    const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
    return make_uint4(l2.x, l2.y, h2.x, h2.y);
}

// MB, NB: 32-channel blocks of dY / X per workgroup (MB * NB = 16: every wave a 64 x 64 output block = 2 x 2 MFMA tiles)
template <bool F16, int MB, int NB, bool S2, int NS = 2>
__global__ __launch_bounds__(256, NS == 2 ? 4 : 2) void wgrad_h_kernel(WArgs g) {
    static_assert(MB * NB == 16, "four waves of 64 x 64");
    // NS stages (2: 32 - 40 KiB of LDS, four workgroups per CU; 4: 64 - 80 KiB, two per CU with three steps of run-ahead each --
    // the same bytes in flight from HALF the workgroups, i.e. half the slabs: see wgrad_plan; 4 x 4 block tiles only)
    constexpr int ASZ = MB * 2048, BSZ = NB * 2048;      // bytes per stage: [block][32 pixels][64 B]
    constexpr int STAGE = ASZ + BSZ;
    constexpr int NPA = MB * 2 / 4, NPB = NB * 2 / 4;    // DMA pieces (16 pixels x 64 B of one block) per wave and step
    constexpr int ND = NPA + NPB;
    static_assert(NS * STAGE <= 65536, "LDS-DMA targets below 64 KiB");
    __shared__ __attribute__((aligned(1024))) unsigned char lds[NS * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    typedef __attribute__((address_space(3))) unsigned char* lptr_t;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(__UINTPTR_TYPE__)(lptr_t)lds);
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);

    const int ntn = (g.N + 32 * NB - 1) / (32 * NB);
    const int tm = blockIdx.x / ntn, tn = blockIdx.x % ntn;
    const int m0 = tm * 32 * MB, n0 = tn * 32 * NB;
    const int k_begin = blockIdx.y * g.kchunk;
    const int k_end = min(g.K, k_begin + g.kchunk);
    const int nk = (k_end - k_begin + WK - 1) / WK;

    // wave -> its 64 x 64 block of the MB*32 x NB*32 tile: blocks of two 32-channel rows / columns
    constexpr int WN = NB / 2;                           // waves along N
    const int wm = wave / WN, wn = wave % WN;            // (MB / 2) x (NB / 2) waves

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    // DMA roles: piece q of a stage = (operand, block, 16-pixel half); this wave issues pieces wave_s, wave_s + 4, ...
    // lane l of a piece: pixel (l >> 2) of the half, 16-byte chunk (l & 3) = channels 8 (l & 3) .. + 7 of the block
    const int lpix = lane >> 2, lch = 8 * (lane & 3);
    auto issue = [&](int t) {
        const unsigned st = lds0 + (t % NS) * STAGE;
        const int kbase = k_begin + t * WK;
#pragma unroll
        for (int q = 0; q < ND; ++q) {
            const int piece = wave_s + 4 * q;             // 0 .. 2 (MB + NB) - 1
            const bool isb = piece >= 2 * MB;
            const int pb = isb ? piece - 2 * MB : piece;
            const int blk = pb >> 1, half = pb & 1;
            const int k = kbase + half * 16 + lpix;
            const h16_t* src;
            if (!isb) {
                int ch = m0 + blk * 32;
                ch = ch < g.M ? ch : g.M - 32;            // (blocks past the matrix re-read the last one; masked at the store)
                src = g.A + (size_t)k * g.lda + ch + lch;
            } else {
                int ch = n0 + blk * 32;
                ch = ch < g.N ? ch : g.N - 32;
                size_t row = k;
                if constexpr (S2) {
                    const int ow = k % g.Wo, q2 = k / g.Wo, oh = q2 % g.Ho, img = q2 / g.Ho;
                    row = ((size_t)img * 2 * g.Ho + 2 * oh) * (2 * g.Wo) + 2 * ow;
                }
                src = g.B + row * g.ldb + ch + lch;
            }
            if (k >= k_end) src = g.zeros + lch;
            lds_dma16(src, st + (isb ? ASZ : 0) + blk * 2048 + half * 1024);
        }
    };

    for (int t = 0; t < NS - 1 && t < nk; ++t) issue(t);
    // transposing fragment reads: source-lane role of this lane inside its 16-lane group: pixel (ll >> 2), channels 4 (ll & 3)..;
    // group gq = lane >> 4: channels 16 (gq & 1) .., pixels 8 (gq >> 1) ..
    const int ll = lane & 15, gq = lane >> 4;
    const int foff = (8 * (gq >> 1) + (ll >> 2)) * 64 + (16 * (gq & 1) + 4 * (ll & 3)) * 2;
    for (int t = 0; t < nk; ++t) {
        // stage t has landed: younger than it are the stages t + 1 .. t + NS - 2 (those that exist)
        if (NS > 2 && t + NS - 2 < nk) wait_vmcnt<(NS - 2) * ND>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + NS - 1 < nk) issue(t + NS - 1);
        const unsigned char* sa = lds + (t % NS) * STAGE + (2 * wm) * 2048 + foff;
        const unsigned char* sb = lds + (t % NS) * STAGE + ASZ + (2 * wn) * 2048 + foff;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            uint4 af[2], bf[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) af[a] = tr_frag(sa + a * 2048 + kk * 16 * 64);
#pragma unroll
            for (int b = 0; b < 2; ++b) bf[b] = tr_frag(sb + b * 2048 + kk * 16 * 64);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = wmma<F16>(af[a], bf[b], acc[a][b]);
        }
    }

    // accumulators -> this K split's slab: lane holds column (lane & 31) of 16 rows per tile: 128-byte row segments
    float* slab = g.slabs + (size_t)blockIdx.y * g.M * g.ldc;
    const int i = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int mb = m0 + (2 * wm + a) * 32, nb = n0 + (2 * wn + b) * 32;
            if (mb < g.M && nb < g.N) {
#pragma unroll
                for (int r = 0; r < 16; ++r) slab[(size_t)(mb + mfma32_row(r, kh)) * g.ldc + nb + i] = acc[a][b][r];
            }
        }
}

struct WTile { int mb, nb; };
WTile pick_tile(int M, int N) {
    if (M >= 256 && N <= 64) return {8, 2};
    if (N >= 256 && M <= 64) return {2, 8};
    if (M <= 64) return {2, 8};
    if (N <= 64) return {8, 2};
    return {4, 4};
}

}  // namespace
}  // namespace peclr

using namespace peclr;

namespace {
// Stages and workgroups per launch.  Two stages x 512 workgroups is the general choice (probe: 512 beats 1024 by 15 - 25 % -- half
// the slab traffic -- and 256 by 5 - 40 %).  The bottleneck shapes (one side four times the other) are served better by four
// stages: from 256 workgroups where the slabs are a large share of the traffic (128 <-> 512, 256 <-> 1024: 74 -> 69, 54 -> 52 us with the
// slab reduction), from 512 at 512 <-> 2048 (48.5 -> 44); 64 <- 64 and the stride-2 shortcuts (ratio 2) lose with either
// (tools/exp/wgrad_h_probe.py over the two builds); the 2 x 8 / 8 x 2 block tiles of layer1 would need 80 KiB.
struct WPlan { int stages; long target; };
WPlan wgrad_plan(int M, int N) {
    static const long forced = getenv("PECLR_WGRAD_H_WGS") ? atol(getenv("PECLR_WGRAD_H_WGS")) : 0;
    static const int deep = getenv("PECLR_WGRAD_H_DEEP") ? atoi(getenv("PECLR_WGRAD_H_DEEP")) : 1;
    const long mn = (long)M * N;
    const bool ratio4 = (M == 4 * N || N == 4 * M) && M >= 128 && N >= 128;      // (the 4 x 4 block tile: four of its stages are 64 KiB)
    WPlan p{2, 512};
    if (deep && ratio4) p = mn <= 262144 ? WPlan{4, 256} : WPlan{4, 512};
    if (forced > 0) p.target = forced;
    return p;
}

// one MB x NB block tile: format x (stride 2 | two stages | four stages -- of the 4 x 4 tile only: 2 x 8 / 8 x 2 would need 80 KiB)
template <int MB, int NB>
void wgrad_h_launch(const WArgs& g, dim3 grid, hipStream_t s, bool f16, bool deep) {
    void (*k)(WArgs);
    if (g.stride == 2) k = f16 ? wgrad_h_kernel<true, MB, NB, true> : wgrad_h_kernel<false, MB, NB, true>;
    else k = f16 ? wgrad_h_kernel<true, MB, NB, false> : wgrad_h_kernel<false, MB, NB, false>;
    if constexpr (MB == 4 && NB == 4)
        if (deep) k = f16 ? wgrad_h_kernel<true, 4, 4, false, 4> : wgrad_h_kernel<false, 4, 4, false, 4>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, g);
}
}  // namespace

extern "C" int peclr_wgrad_h_slabs(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0 || M % 32 || N % 32) return 0;
    const WTile t = pick_tile(M, N);
    const long tiles = (long)((M + 32 * t.mb - 1) / (32 * t.mb)) * ((N + 32 * t.nb - 1) / (32 * t.nb));
    const long target = wgrad_plan(M, N).target;
    long s = (target + tiles - 1) / tiles;
    const long max_s = (K + 8 * WK - 1) / (8 * WK);      // at least eight k-steps per slab
    if (s > max_s) s = max_s;
    if (s < 1) s = 1;
    const int kchunk = (int)(((K + s - 1) / s + WK - 1) / WK * WK);
    return (K + kchunk - 1) / kchunk;
}

// dW slabs of a 1x1 convolution from 16-bit activations: A = dY [K][lda] (M = Cout), B = X [K][ldb] (N = Cin) -- stride 2: X
// holds the 2 Ho x 2 Wo input pixels and dY's rows are the Ho x Wo output pixels.  slabs: [n_slabs][M][N] fp32.
extern "C" int peclr_wgrad_h(int dtype, int M, int N, int K, const void* A, int lda, const void* B, int ldb, float* slabs, int n_slabs,
                             int stride, int Ho, int Wo, const void* zeros, peclr_stream_t stream) {
    if (!A || !B || !slabs || !zeros) return PECLR_ERR_NULL;
    if (M <= 0 || N <= 0 || K <= 0 || n_slabs < 1 || (stride != 1 && stride != 2)) return PECLR_ERR_SHAPE;
    if (M % 32 || N % 32 || lda % 8 || ldb % 8 || lda < M || ldb < N) return PECLR_ERR_SHAPE;
    if (stride == 2 && (Ho <= 0 || Wo <= 0 || K % (Ho * Wo))) return PECLR_ERR_SHAPE;
    if (!aligned16(A) || !aligned16(B) || !aligned16(slabs) || !aligned16(zeros)) return PECLR_ERR_ALIGN;
    if (n_slabs != peclr_wgrad_h_slabs(M, N, K)) return PECLR_ERR_WORKSPACE;
    if (dtype != PECLR_DTYPE_BF16 && dtype != PECLR_DTYPE_F16) return PECLR_ERR_UNSUPPORTED;
    WArgs g;
    g.A = static_cast<const h16_t*>(A); g.B = static_cast<const h16_t*>(B); g.slabs = slabs;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = N;
    g.kchunk = ((K + n_slabs - 1) / n_slabs + WK - 1) / WK * WK;
    g.stride = stride; g.Ho = Ho > 0 ? Ho : 1; g.Wo = Wo > 0 ? Wo : 1; g.zeros = static_cast<const h16_t*>(zeros);
    const WTile t = pick_tile(M, N);
    const dim3 grid(((M + 32 * t.mb - 1) / (32 * t.mb)) * ((N + 32 * t.nb - 1) / (32 * t.nb)), n_slabs);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool f16 = dtype == PECLR_DTYPE_F16;
    const bool deep = stride == 1 && wgrad_plan(M, N).stages == 4;
    if (t.mb == 8) wgrad_h_launch<8, 2>(g, grid, s, f16, deep);
    else if (t.mb == 2) wgrad_h_launch<2, 8>(g, grid, s, f16, deep);
    else wgrad_h_launch<4, 4>(g, grid, s, f16, deep);
    return launch_status();
}

// ---- 3x3 / padding-1 / stride-1 weight gradient, 16-bit:  dW[co][tap][ci] = sum over output pixels r of dY[r][co] * X[r + tap][ci].
//
// The contraction runs over a PADDED linear pixel space: every image becomes (H + 1) x (W + 1) slots -- one zero column in
// front of each row (it is also the zero column behind the previous row) and one zero row in front of each image (also the
// zero row behind the previous image) -- so that tap (a, b) of dY's slot p is X's slot p + (a - 1)(W + 1) + (b - 1) for EVERY
// p, borders included: taps that leave the image land on zero slots, dY's own zero slots contribute nothing, and the loop
// needs no per-(pixel, tap) masks (4 - 30 % more MFMA work, on a product that is bound by LDS fragment reads).  Both
// operands are written into LDS by LDS-DMA with the padding applied by the ADDRESS each lane fetches (pad slots read a zero
// line): dY as k-step tiles, X into a RING of slots that every k-step advances by 32 -- each X element is fetched once and
// serves all nine taps through transposing reads (ds_read_b64_tr_b16) at the taps' slot offsets.
// Workgroup: 64 output x 64 input channels x 9 taps; wave = 32 x 32 x 9 (nine accumulators).
//
// The ring has RINGP = 256 slots (a power of two >= 2 * roundup(row pitch + 1, 32) + 96: the k-step's 32 slots, lead and lag of
// the taps, and the groups in flight): 32 KiB serve W <= 62, i.e. every 3x3 of ResNet at 224 x 224 (W3Args); a 512-slot ring
// would leave the 64 KiB an LDS-DMA can address.  Rows of 63 pixels and more run over a COLUMN-SEGMENTED padded space instead
// (W3WArgs): every image is cut into nseg = ceil(W / 61) column segments of near-equal width (seg_base, + 1 for the first
// seg_extra), and each (image, segment) is a PSEUDO-IMAGE of the padded space: a zero row in front, then H rows of
// S = (widest segment) + 2 slots -- slot 0 the image column LEFT of the segment, slots 1 .. Ws the segment's own, slot Ws + 1 the
// column RIGHT of it, the rest (a segment one narrower than the widest) zero.  There the operands differ in what a halo slot
// holds: dY's are zero (every output pixel is summed in exactly one segment), X's are the neighbouring segment's real pixels,
// zero only outside the image.  Tap (a, b) of slot p is X's slot p + (a - 1) S + (b - 1) for every p, as above; 35 <= S + 1 <= 64,
// so lead and lag are 64 slots and the 256-slot ring serves any width (2 - 6 % more slots than the un-segmented space would
// have: 4.5 % at 112 x 112).
// Both spaces run through ONE kernel, wgrad3_h_kernel<F16, Args>: ring, stages, waits, fragment reads and slab store are
// written once, and only the slot -> address map of the DMA lanes (src_of) has an arm per space, chosen by Args::wide.  All
// four instantiations are, instruction for instruction, what two separate kernels compiled to
// (profiles/isa_identity_wgrad_h.txt).  What that takes: the row pitch comes from an overload per argument struct
// (row_pitch), and the lead L is a `const int` whose initialiser is a constant expression in the segmented instantiation, so
// that the lambdas do not capture it and G0 folds; assigning L from a runtime temporary under `if constexpr` was still correct
// but cost the segmented kernel three scalar instructions in its prologue and one SGPR.  The field order of each struct is the
// kernel-argument layout: keep it.
namespace peclr {
namespace {

struct W3Args {
    static constexpr bool wide = false;
    const h16_t* A;                      // dY [images * H * W][lda]
    const h16_t* B;                      // X  [images * H * W][ldb]
    float* slabs;                        // [n_slabs][M][9 * N]
    int M, N, lda, ldb;
    int H, W, images;
    int P;                               // padded slots: images * (H + 1) * (W + 1)
    int pchunk;                          // padded slots per slab (multiple of 32)
    const h16_t* zeros;
    unsigned m_hw, s_hw, m_w, s_w;       // p / ((H + 1)(W + 1)) = mulhi(p, m_hw) >> s_hw for 0 <= p < 2^31; likewise / (W + 1)
};
struct W3WArgs {
    static constexpr bool wide = true;
    const h16_t* A;                      // dY [images * H * W][lda]
    const h16_t* B;                      // X  [images * H * W][ldb]
    float* slabs;                        // [n_slabs][M][9 * N]
    int M, N, lda, ldb;
    int H, W, images;
    int S, nseg, seg_base, seg_extra;
    int P;                               // padded slots: images * nseg * (H + 1) * S
    int pchunk;                          // padded slots per slab (multiple of 32)
    const h16_t* zeros;
    unsigned m_hs, s_hs, m_s, s_s, m_seg, s_seg;     // magic_div by (H + 1) S, by S, by nseg
};
__device__ __forceinline__ int row_pitch(const W3Args& g) { return g.W + 1; }     // slots per row of the padded space
__device__ __forceinline__ int row_pitch(const W3WArgs& g) { return g.S; }

// exact division of a 31-bit number by d >= 2 as a multiply-high and a shift (the loop's two DMA addresses per step took two
// integer divisions each: ~60 vector instructions next to 18 products)
inline void magic_div(unsigned d, unsigned& m, unsigned& sh) {
    unsigned l = 0;
    while ((1ull << l) < d) ++l;                         // ceil(log2 d) >= 1
    m = (unsigned)(((1ull << (31 + l)) / d) + 1);
    sh = l - 1;
}

template <bool F16, typename Args>
__global__ __launch_bounds__(256, 2) void wgrad3_h_kernel(Args g) {
    constexpr bool WIDE = Args::wide;
    constexpr int RINGP = 256;                           // slots of the X ring
    constexpr int NSA = 3;                               // dY stages (two k-steps of run-ahead)
    constexpr int ASZ = 2 * 2048;                        // [2 blocks][32 slots][64 B]
    constexpr int RB = RINGP * 64;                       // ring: [2 blocks][RINGP slots][64 B], FIRST in the LDS: a slot's address is
    constexpr int R0 = 0;                                // ((byte offset) & (RB - 1)) | (block base + channel bytes): two instructions
    constexpr int A0 = 2 * RB;                           // dY stages behind it
    static_assert(A0 + NSA * ASZ <= 65536 && (RB & (RB - 1)) == 0, "LDS-DMA targets below 64 KiB; power-of-two ring");
    __shared__ __attribute__((aligned(1024))) unsigned char lds[A0 + NSA * ASZ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    typedef __attribute__((address_space(3))) unsigned char* lptr_t;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(__UINTPTR_TYPE__)(lptr_t)lds);
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const int S = row_pitch(g), HS = (g.H + 1) * S;
    const int L = WIDE ? 64 : (g.W + 2 + 31) / 32 * 32;  // lead / lag of the ring around the current k-step, in slots (see above)
    if constexpr (WIDE) static_assert(RINGP >= 2 * 64 + 32 + 3 * 32, "k-step, lead, lag, and the groups in flight");
    const int ntn = g.N / 64;
    const int m0 = (int)(blockIdx.x / ntn) * 64, n0 = (int)(blockIdx.x % ntn) * 64;
    const int p_begin = blockIdx.y * g.pchunk;
    const int p_end = min(g.P, p_begin + g.pchunk);
    const int nk = (p_end - p_begin + 31) / 32;
    const int mblk = wave >> 1, nblk = wave & 1;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // DMA: this wave moves piece (block = wave >> 1, 16-slot half = wave & 1) of every 32-slot group; lane = slot (lane >> 2) of
    // the half, channels 8 (lane & 3) .. + 7 of the block.
    const int dblk = wave_s >> 1, dhalf = wave_s & 1;
    const int lch = 8 * (lane & 3);
    auto src_of = [&](const h16_t* base, int ld, int ch0, int p, bool live, bool halo) -> const h16_t* {
        if constexpr (WIDE) {
            // slot p = (pseudo-image q, row hh, slot ww): image q / nseg, segment q % nseg, image row hh - 1, image column
            // (segment's first) + ww - 1.  dY is live in its own columns 1 <= ww <= Ws only, X (halo) also in the two halo
            // slots where that column exists in the image.
            const int q = (int)(__umulhi((unsigned)p, g.m_hs) >> g.s_hs), rem = p - q * HS;          // (p < 0: garbage, not used)
            const int hh = (int)(__umulhi((unsigned)rem, g.m_s) >> g.s_s), ww = rem - hh * S;
            const int img = (int)(__umulhi((unsigned)q, g.m_seg) >> g.s_seg), seg = q - img * g.nseg;
            const int ws = g.seg_base + (seg < g.seg_extra ? 1 : 0);
            const int col = seg * g.seg_base + min(seg, g.seg_extra) + ww - 1;
            const bool slot = halo ? ww <= ws + 1 && col >= 0 && col < g.W : ww >= 1 && ww <= ws;
            const bool real = live && p >= 0 && img < g.images && hh >= 1 && slot;
            const size_t row = ((size_t)img * g.H + (hh - 1)) * g.W + col;
            return real ? base + row * ld + ch0 + lch : g.zeros + lch;
        } else {
            // slot p is real pixel (img, hh - 1, ww - 1) iff hh, ww >= 1, for either operand
            const int img = (int)(__umulhi((unsigned)p, g.m_hw) >> g.s_hw), rem = p - img * HS;      // (p < 0: garbage, not used)
            const int hh = (int)(__umulhi((unsigned)rem, g.m_w) >> g.s_w), ww = rem - hh * S;
            const bool real = live && p >= 0 && img < g.images && hh >= 1 && ww >= 1;
            const size_t row = ((size_t)img * g.H + (hh - 1)) * g.W + (ww - 1);
            return real ? base + row * ld + ch0 + lch : g.zeros + lch;
        }
    };
    auto issue_a = [&](int t) {                           // dY slots [p_begin + 32 t, + 32) -> stage t % NSA
        const int p = p_begin + 32 * t + 16 * dhalf + (lane >> 2);
        lds_dma16(src_of(g.A, g.lda, m0 + 32 * dblk, p, p < p_end, false), lds0 + A0 + (t % NSA) * ASZ + dblk * 2048 + dhalf * 1024);
    };
    auto issue_x = [&](int u) {                           // ring group u: X slots [p_begin - L + 32 u, + 32)
        const int p = p_begin - L + 32 * u + 16 * dhalf + (lane >> 2);
        const unsigned slot0 = (unsigned)(32 * u + 16 * dhalf) & (RINGP - 1);
        lds_dma16(src_of(g.B, g.ldb, n0 + 32 * dblk, p, true, true), lds0 + R0 + dblk * RB + slot0 * 64);
    };
    // k-step t reads ring groups t .. t + 2 L / 32 (slots [32 t, 32 t + 32 + 2 L) relative to p_begin - L); groups are issued two
    // steps ahead of their first use
    const int G0 = 2 * L / 32 + 1;                        // groups the first step needs
    // order of issue: what step 0 needs -- dY(0), ring groups 0 .. G0 - 1 -- first, then what step 1 adds: ring group G0, dY(1)
    issue_a(0);
    for (int u = 0; u < G0; ++u) issue_x(u);
    if (nk > 1) { issue_x(G0); issue_a(1); }
    const int ll = lane & 15, gq = lane >> 4;
    const int fpix = 8 * (gq >> 1) + (ll >> 2);           // slot of this source lane inside a 16-slot k-extent (+ 4 for the second read)
    const int fch = (16 * (gq & 1) + 4 * (ll & 3)) * 2;
    for (int t = 0; t < nk; ++t) {
        // landed: dY(t) and ring groups <= t + G0 - 1; younger than those: dY(t + 1) [1 DMA] and ring group t + G0 [1 DMA]
        if (t + 1 < nk) wait_vmcnt<2>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + 1 < nk) issue_x(t + G0 + 1);              // (the ring slot group it overwrites was last read in step t - 1 at the latest)
        if (t + 2 < nk) issue_a(t + 2);
        const unsigned char* sa = lds + A0 + (t % NSA) * ASZ + mblk * 2048 + fch;
        const unsigned xor_ = (unsigned)(nblk * RB + fch);            // (block base + this lane's channel bytes: bits the mask clears)
        const unsigned xb64 = (unsigned)(32 * t + L + fpix) * 64u;    // byte offset (before the wrap) of this lane's first pixel at shift 0
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const uint4 af = tr_frag(sa + (kk * 16 + fpix) * 64);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int shift = (tap / 3 - 1) * S + (tap % 3 - 1);
                typedef __attribute__((address_space(3))) s16x4* lp;
                const unsigned t0 = xb64 + (unsigned)((kk * 16 + shift) * 64);
                const unsigned a0 = (t0 & (unsigned)(RB - 64)) | xor_, a1 = ((t0 + 256u) & (unsigned)(RB - 64)) | xor_;
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(lds + a0));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(lds + a1));
                const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                acc[tap] = wmma<F16>(af, make_uint4(l2.x, l2.y, h2.x, h2.y), acc[tap]);
            }
        }
    }
    float* slab = g.slabs + (size_t)blockIdx.y * g.M * 9 * g.N;
    const int i = lane & 31, kh = lane >> 5;
    const int mb = m0 + 32 * mblk, nb = n0 + 32 * nblk;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 16; ++r) slab[(size_t)(mb + mfma32_row(r, kh)) * (9 * g.N) + tap * g.N + nb + i] = acc[tap][r];
}

// the column segments of a W-pixel row (W >= 63), and the padded slots of the whole problem (0: too many for the magic divisions,
// which take 31-bit numbers -- the ring reads a little past P)
struct W3Seg { int nseg, base, extra, S; long P; };
W3Seg wide_segments(int images, int H, int W) {
    W3Seg s;
    s.nseg = (W + 60) / 61;
    s.base = W / s.nseg; s.extra = W % s.nseg;
    s.S = s.base + (s.extra ? 1 : 0) + 2;
    s.P = (long)images * s.nseg * (H + 1) * s.S;
    if (s.P > 0x7fffffffL / 2) s.P = 0;
    return s;
}
constexpr int W3W_MIN_W = 63, W3W_MAX_W = 512;           // narrower rows belong to peclr_wgrad3_h; the widest row the tests cover

// slabs of P padded slots under `tiles` 64 x 64 channel tiles, either space
int w3_slabs(long P, long tiles) {
    long s = (512 + tiles - 1) / tiles;                  // two workgroups per CU
    const long max_s = (P + 16 * 32 - 1) / (16 * 32);    // at least sixteen k-steps per slab (the ring warm-up is 3 - 9 groups)
    if (s > max_s) s = max_s;
    if (s < 1) s = 1;
    const long pchunk = ((P + s - 1) / s + 31) / 32 * 32;
    return (int)((P + pchunk - 1) / pchunk);
}

// what both entry points check, in the order that decides a bad call's error code; `shape_ok`: the entry point's own predicate
int w3_check(const void* A, const void* B, const float* slabs, const void* zeros, bool shape_ok, int n_slabs, int want_slabs,
             int dtype) {
    if (!A || !B || !slabs || !zeros) return PECLR_ERR_NULL;
    if (!shape_ok) return PECLR_ERR_SHAPE;
    if (!aligned16(A) || !aligned16(B) || !aligned16(slabs) || !aligned16(zeros)) return PECLR_ERR_ALIGN;
    if (n_slabs != want_slabs) return PECLR_ERR_WORKSPACE;
    if (dtype != PECLR_DTYPE_BF16 && dtype != PECLR_DTYPE_F16) return PECLR_ERR_UNSUPPORTED;
    return PECLR_OK;
}

// the fields both argument structs have (g.P and the address map's own are the caller's), and the launch
template <typename Args>
int w3_launch(Args& g, int dtype, int M, int N, int images, int H, int W, const void* A, const void* B, float* slabs, int n_slabs,
              const void* zeros, peclr_stream_t stream) {
    g.A = static_cast<const h16_t*>(A); g.B = static_cast<const h16_t*>(B); g.slabs = slabs;
    g.M = M; g.N = N; g.lda = M; g.ldb = N; g.H = H; g.W = W; g.images = images;
    g.pchunk = ((g.P + n_slabs - 1) / n_slabs + 31) / 32 * 32;
    g.zeros = static_cast<const h16_t*>(zeros);
    const dim3 grid((M / 64) * (N / 64), n_slabs);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == PECLR_DTYPE_F16) hipLaunchKernelGGL((wgrad3_h_kernel<true, Args>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((wgrad3_h_kernel<false, Args>), grid, dim3(256), 0, s, g);
    return launch_status();
}

}  // namespace
}  // namespace peclr

extern "C" int peclr_wgrad3_h_slabs(int M, int N, int images, int H, int W) {
    if (M <= 0 || N <= 0 || images <= 0 || H <= 0 || W <= 0 || M % 64 || N % 64 || W > 62) return 0;
    return w3_slabs((long)images * (H + 1) * (W + 1), (long)(M / 64) * (N / 64));
}

// dW slabs [n_slabs][Cout][9 * Cin] of a 3x3 / padding-1 / stride-1 convolution from 16-bit NHWC activations dY [images, H, W,
// Cout], X [images, H, W, Cin].
extern "C" int peclr_wgrad3_h(int dtype, int M, int N, int images, int H, int W, const void* A, const void* B, float* slabs,
                              int n_slabs, const void* zeros, peclr_stream_t stream) {
    const bool shape_ok = !(M <= 0 || N <= 0 || images <= 0 || H <= 0 || W <= 0 || M % 64 || N % 64 || W > 62) &&
                          !((long)images * (H + 1) * (W + 1) > 0x7fffffffL / 2);
    if (const int e = w3_check(A, B, slabs, zeros, shape_ok, n_slabs, peclr_wgrad3_h_slabs(M, N, images, H, W), dtype)) return e;
    W3Args g;
    g.P = images * (H + 1) * (W + 1);
    magic_div((unsigned)((H + 1) * (W + 1)), g.m_hw, g.s_hw);
    magic_div((unsigned)(W + 1), g.m_w, g.s_w);
    return w3_launch(g, dtype, M, N, images, H, W, A, B, slabs, n_slabs, zeros, stream);
}

// The same for rows of 63 .. 512 pixels (the column-segmented space).  Slab policy as above, on the segmented slot count.
extern "C" int peclr_wgrad3w_h_slabs(int M, int N, int images, int H, int W) {
    if (M <= 0 || N <= 0 || images <= 0 || H <= 0 || M % 64 || N % 64 || W < W3W_MIN_W || W > W3W_MAX_W) return 0;
    const long P = wide_segments(images, H, W).P;
    if (P <= 0) return 0;
    return w3_slabs(P, (long)(M / 64) * (N / 64));
}

extern "C" int peclr_wgrad3w_h(int dtype, int M, int N, int images, int H, int W, const void* A, const void* B, float* slabs,
                               int n_slabs, const void* zeros, peclr_stream_t stream) {
    const bool dims_ok = !(M <= 0 || N <= 0 || images <= 0 || H <= 0 || M % 64 || N % 64 || W < W3W_MIN_W || W > W3W_MAX_W);
    const W3Seg sg = dims_ok ? wide_segments(images, H, W) : W3Seg{};
    if (const int e = w3_check(A, B, slabs, zeros, dims_ok && !(sg.P <= 0), n_slabs, peclr_wgrad3w_h_slabs(M, N, images, H, W), dtype))
        return e;
    W3WArgs g;
    g.S = sg.S; g.nseg = sg.nseg; g.seg_base = sg.base; g.seg_extra = sg.extra;
    g.P = (int)sg.P;
    magic_div((unsigned)((H + 1) * sg.S), g.m_hs, g.s_hs);
    magic_div((unsigned)sg.S, g.m_s, g.s_s);
    magic_div((unsigned)sg.nseg, g.m_seg, g.s_seg);
    return w3_launch(g, dtype, M, N, images, H, W, A, B, slabs, n_slabs, zeros, stream);
}

// ---- 3x3 / padding-1 / STRIDE-2 weight gradient, 16-bit:  dW[co][a][b][ci] = sum over output pixels (img, oh, ow) of
// dY[img, oh, ow, co] * X[img, 2 oh + a - 1, 2 ow + b - 1, ci], X of 2 Ho x 2 Wo pixels.
//
// X is seen as four PARITY PLANES (row parity pr, column parity pc), each an Ho x Wo image: plane pixel (i, j) is X pixel
// (2 i + pr, 2 j + pc).  Tap row a = 0 meets the odd rows at plane row oh - 1, a = 1 the even rows at oh, a = 2 the odd rows at oh;
// columns alike.  With every plane in the padded space of wgrad3_h_kernel at dY's geometry -- (Ho + 1) x (Wo + 1) slots per
// image, zero row and zero column in front -- tap (a, b) of dY's slot p is slot p - (a == 0)(Wo + 1) - (b == 0) of plane
// (a != 1, b != 1), for every p: (even, even) serves one tap, (even, odd) and (odd, even) two each, (odd, odd) four.  No shift is
// positive (H = 2 Ho, W = 2 Wo: the bottom and right padding is never met), so a ring needs a lead L = roundup(Wo + 2, 32) and no
// lag: the k-step's 32 slots + L <= 64 + the three groups in flight = 192 slots.
// Workgroup: 64 output x 32 input channels x 9 taps, one ring of 192 slots x 64 B per plane (4 x 12 KiB, all filled by
// LDS-DMA, with the four dY stages 64 KiB: what an LDS-DMA can address; two workgroups per CU; three k-steps of run-ahead).  The ring is not a
// power of two: a slot's wrap is one subtract and one unsigned minimum where wgrad3_h_kernel has an AND and an OR.
// Every k-step's dY tile is staged once and feeds all nine taps.  Wave = (32 output channels, 16-slot half of the k-step) x 32
// input channels x 9 taps: nine accumulators and nine products per wave and step, all four waves the same work whatever the
// 4 / 2 / 2 / 1 split of the planes; the two halves of the contraction meet once, behind the loop, through the LDS that the rings
// leave (a + b in fp32: one order), and each wave of a pair stores half the taps.
namespace peclr {
namespace {

struct W3S2Args {
    const h16_t* A;                      // dY [images * Ho * Wo][lda]
    const h16_t* B;                      // X  [images * 2 Ho * 2 Wo][ldb]
    float* slabs;                        // [n_slabs][M][9 * N]
    int M, N, lda, ldb;
    int Ho, Wo, images;
    int P;                               // padded slots: images * (Ho + 1) * (Wo + 1)
    int pchunk;                          // padded slots per slab (multiple of 32)
    const h16_t* zeros;
    unsigned m_hw, s_hw, m_w, s_w;       // magic_div by (Ho + 1)(Wo + 1), by (Wo + 1)
    int rows, gsplit;                    // XCD rows: (slab, one of gsplit groups of input-channel tiles); see s2_rows
};

template <bool F16>
__global__ __launch_bounds__(256, 2) void wgrad3_h_s2_kernel(W3S2Args g) {
    constexpr int RINGP = 192;                           // slots of each plane's ring: six 32-slot groups
    constexpr int NG = RINGP / 32;
    constexpr int AHEAD = 3;                             // k-steps of run-ahead of the DMAs
    constexpr int NSA = AHEAD + 1;                       // dY stages
    constexpr int ASZ = 2 * 2048;                        // [2 blocks][32 slots][64 B]
    constexpr int RB = RINGP * 64;                       // one plane's ring: [RINGP slots][64 B] (one 32-channel block)
    constexpr int A0 = 4 * RB;                           // dY stages behind the four rings
    static_assert(A0 + NSA * ASZ <= 65536, "LDS-DMA targets below 64 KiB");
    static_assert(RINGP >= 32 + 64 + AHEAD * 32, "k-step, lead, and the groups in flight");
    static_assert(2 * 5 * 4096 <= A0 && 2 * 4 * 4096 <= A0, "the exchange of the two k-halves fits the rings");
    __shared__ __attribute__((aligned(1024))) unsigned char lds[A0 + NSA * ASZ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    typedef __attribute__((address_space(3))) unsigned char* lptr_t;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(__UINTPTR_TYPE__)(lptr_t)lds);
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const int S = g.Wo + 1, HS = (g.Ho + 1) * S;
    const int L = (g.Wo + 2 + 31) / 32 * 32;             // lead of the rings in front of the current k-step, in slots: 32 or 64
    // the workgroups of one row -- every 64-channel tile of dY against one group of 32-channel tiles of X, same slab -- run on
    // ONE XCD, side by side: what they share (each dY tile npg times, each X tile M / 64 times) comes from that XCD's L2
    const int npg = g.N / 32 / g.gsplit;                 // input-channel tiles per group
    const XcdTile xt = xcd_tile(blockIdx.x, (g.M / 64) * npg);
    if (xt.row_block >= g.rows) return;
    const int slab_i = xt.row_block / g.gsplit;
    const int m0 = (xt.col_tile / npg) * 64, n0 = ((xt.row_block % g.gsplit) * npg + xt.col_tile % npg) * 32;
    const int p_begin = slab_i * g.pchunk;
    const int p_end = min(g.P, p_begin + g.pchunk);
    const int nk = (p_end - p_begin + 31) / 32;
    const int mblk = wave_s >> 1, khalf = wave_s & 1;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // DMA: of every 32-slot group this wave moves dY's piece (block = wave >> 1, 16-slot half = wave & 1) and the same half of the
    // planes (wave >> 1) and (wave >> 1) + 2; lane = slot (lane >> 2) of the half, channels 8 (lane & 3) .. + 7 of the block.
    const int dblk = wave_s >> 1, dhalf = wave_s & 1;
    const int lch = 8 * (lane & 3);
    // slot p = (img, hh, ww) is output pixel / plane pixel (img, hh - 1, ww - 1) iff hh, ww >= 1
    auto src_of = [&](const h16_t* base, int ld, int ch0, int p, bool live, int plane) -> const h16_t* {
        const int img = (int)(__umulhi((unsigned)p, g.m_hw) >> g.s_hw), rem = p - img * HS;          // (p < 0: garbage, not used)
        const int hh = (int)(__umulhi((unsigned)rem, g.m_w) >> g.s_w), ww = rem - hh * S;
        const bool real = live && p >= 0 && img < g.images && hh >= 1 && ww >= 1;
        size_t row;
        if (plane < 0) row = ((size_t)img * g.Ho + (hh - 1)) * g.Wo + (ww - 1);                      // dY
        else row = ((size_t)img * 2 * g.Ho + 2 * (hh - 1) + (plane >> 1)) * (2 * g.Wo) + 2 * (ww - 1) + (plane & 1);
        return real ? base + row * ld + ch0 + lch : g.zeros + lch;
    };
    auto issue_a = [&](int t) {                           // dY slots [p_begin + 32 t, + 32) -> stage t % NSA
        const int p = p_begin + 32 * t + 16 * dhalf + (lane >> 2);
        lds_dma16(src_of(g.A, g.lda, m0 + 32 * dblk, p, p < p_end, -1), lds0 + A0 + (t % NSA) * ASZ + dblk * 2048 + dhalf * 1024);
    };
    auto issue_x = [&](int u) {                           // ring group u of this wave's two planes: X slots [p_begin - L + 32 u, + 32)
        const int p = p_begin - L + 32 * u + 16 * dhalf + (lane >> 2);
        const unsigned slot0 = (unsigned)(32 * (u % NG) + 16 * dhalf);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int plane = dblk + 2 * j;
            lds_dma16(src_of(g.B, g.ldb, n0, p, true, plane), lds0 + plane * RB + slot0 * 64);
        }
    };
    // k-step t reads ring groups t .. t + L / 32 (slots [32 t, 32 t + 32 + L) relative to p_begin - L).  What step s adds to step
    // s - 1's needs -- ring group G0 + s - 1 [2 DMAs], then dY(s) [1 DMA] -- is issued AHEAD steps before it
    const int G0 = L / 32 + 1;                            // groups the first step needs: 2 or 3
    issue_a(0);
    for (int u = 0; u < G0; ++u) issue_x(u);
    for (int s = 1; s < AHEAD; ++s)
        if (s < nk) { issue_x(G0 + s - 1); issue_a(s); }
    const int ll = lane & 15, gq = lane >> 4;
    const int fpix = 8 * (gq >> 1) + (ll >> 2);           // slot of this source lane inside a 16-slot k-extent (+ 4 for the second read)
    const int fch = (16 * (gq & 1) + 4 * (ll & 3)) * 2;
    for (int t = 0; t < nk; ++t) {
        // landed: dY(t) and ring groups <= t + G0 - 1; younger than those: what the steps t + 1 .. t + AHEAD - 1 that exist add
        static_assert(AHEAD == 3, "the waits below");
        if (t + 2 < nk) wait_vmcnt<6>();
        else if (t + 1 < nk) wait_vmcnt<3>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // (the ring group it overwrites, t + G0 + AHEAD - 1 - NG <= t - 1, was last read in step t - 1, the dY stage too)
        if (t + AHEAD < nk) { issue_x(t + G0 + AHEAD - 1); issue_a(t + AHEAD); }
        const uint4 af = tr_frag(lds + A0 + (t % NSA) * ASZ + mblk * 2048 + fch + (khalf * 16 + fpix) * 64);
        // this lane's first pixel at shift -L, before the wrap: < 160 + 64 + 32 + 4, i.e. below 2 RINGP
        const unsigned x0 = (unsigned)(32 * (t % NG) + khalf * 16 + fpix);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int plane = (tap / 3 != 1 ? 2 : 0) + (tap % 3 != 1 ? 1 : 0);
            const int shift = L - (tap / 3 == 0 ? S : 0) - (tap % 3 == 0 ? 1 : 0);       // >= 0: S + 1 <= L
            typedef __attribute__((address_space(3))) s16x4* lp;
            const unsigned c0 = x0 + (unsigned)shift, c1 = c0 + 4u;
            const unsigned w0 = min(c0, c0 - (unsigned)RINGP), w1 = min(c1, c1 - (unsigned)RINGP);
            const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(lds + plane * RB + fch + w0 * 64u));
            const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(lds + plane * RB + fch + w1 * 64u));
            const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
            acc[tap] = wmma<F16>(af, make_uint4(l2.x, l2.y, h2.x, h2.y), acc[tap]);
        }
    }
    // the two k-halves of a 32-channel block of dY meet: the odd wave hands taps 0 .. 4 to the even one, then the even wave
    // taps 5 .. 8 to the odd one ([wave pair][tap][register][lane] floats where the rings were)
    float* xch = reinterpret_cast<float*>(lds) + mblk * (5 * 1024) + lane;
    __syncthreads();                                     // (every wave has read its last fragments)
    if (khalf) {
#pragma unroll
        for (int tap = 0; tap < 5; ++tap)
#pragma unroll
            for (int r = 0; r < 16; ++r) xch[tap * 1024 + r * 64] = acc[tap][r];
    }
    __syncthreads();
    if (!khalf) {
#pragma unroll
        for (int tap = 0; tap < 5; ++tap)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tap][r] += xch[tap * 1024 + r * 64];
    }
    __syncthreads();
    if (!khalf) {
#pragma unroll
        for (int tap = 5; tap < 9; ++tap)
#pragma unroll
            for (int r = 0; r < 16; ++r) xch[(tap - 5) * 1024 + r * 64] = acc[tap][r];
    }
    __syncthreads();
    if (khalf) {
#pragma unroll
        for (int tap = 5; tap < 9; ++tap)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tap][r] += xch[(tap - 5) * 1024 + r * 64];
    }
    float* slab = g.slabs + (size_t)slab_i * g.M * 9 * g.N;
    const int i = lane & 31, kh = lane >> 5;
    const int mb = m0 + 32 * mblk;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
        if ((tap >= 5) == (khalf != 0)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) slab[(size_t)(mb + mfma32_row(r, kh)) * (9 * g.N) + tap * g.N + n0 + i] = acc[tap][r];
        }
}

constexpr int W3S2_MAX_WO = 62;                          // Wo + 2 <= 64: the lead the 192-slot rings have room for

// padded slots of the stride-2 problem (0: a size the entry points refuse)
long s2_slots(int M, int N, int images, int Ho, int Wo) {
    if (M <= 0 || N <= 0 || images <= 0 || Ho <= 0 || Wo <= 0 || M % 64 || N % 64 || Wo > W3S2_MAX_WO) return 0;
    const long P = (long)images * (Ho + 1) * (Wo + 1);
    return P > 0x7fffffffL / 2 ? 0 : P;
}

// Rows of the XCD-aware tile order (xcd_tile): a slab's tiles as one row where the slabs alone fill the eight XCDs evenly,
// else the input-channel tiles of a slab in 2, 4, .. groups until the rows are a multiple of eight (or the tiles run out)
int s2_gsplit(int n_slabs, int ntn) {
    int gs = 1;
    while ((n_slabs * gs) % 8 && ntn % (2 * gs) == 0) gs *= 2;
    return gs;
}

}  // namespace
}  // namespace peclr

// Slab policy of peclr_wgrad3_h_slabs on the OUTPUT's padded slots, under the kernel's 64 x 32 channel tiles.
extern "C" int peclr_wgrad3s2_h_slabs(int M, int N, int images, int Ho, int Wo) {
    const long P = s2_slots(M, N, images, Ho, Wo);
    if (P <= 0) return 0;
    return w3_slabs(P, (long)(M / 64) * (N / 32));
}

// dW slabs [n_slabs][Cout][9 * Cin] of a 3x3 / padding-1 / stride-2 convolution from 16-bit NHWC activations dY [images, Ho, Wo,
// Cout], X [images, 2 Ho, 2 Wo, Cin].
extern "C" int peclr_wgrad3s2_h(int dtype, int M, int N, int images, int Ho, int Wo, const void* dY, const void* X, float* slabs,
                                int n_slabs, const void* zeros, peclr_stream_t stream) {
    const long P = s2_slots(M, N, images, Ho, Wo);
    if (const int e = w3_check(dY, X, slabs, zeros, P > 0, n_slabs, peclr_wgrad3s2_h_slabs(M, N, images, Ho, Wo), dtype)) return e;
    W3S2Args g;
    g.A = static_cast<const h16_t*>(dY); g.B = static_cast<const h16_t*>(X); g.slabs = slabs;
    g.M = M; g.N = N; g.lda = M; g.ldb = N; g.Ho = Ho; g.Wo = Wo; g.images = images;
    g.P = (int)P;
    g.pchunk = ((g.P + n_slabs - 1) / n_slabs + 31) / 32 * 32;
    g.zeros = static_cast<const h16_t*>(zeros);
    magic_div((unsigned)((Ho + 1) * (Wo + 1)), g.m_hw, g.s_hw);
    magic_div((unsigned)(Wo + 1), g.m_w, g.s_w);
    g.gsplit = s2_gsplit(n_slabs, N / 32);
    g.rows = n_slabs * g.gsplit;
    const dim3 grid((unsigned)((g.rows + 7) / 8 * 8 * ((M / 64) * (N / 32) / g.gsplit)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == PECLR_DTYPE_F16) hipLaunchKernelGGL(wgrad3_h_s2_kernel<true>, grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL(wgrad3_h_s2_kernel<false>, grid, dim3(256), 0, s, g);
    return launch_status();
}
