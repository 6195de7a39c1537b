/*
 * peclr_hip.h -- C ABI of libpeclr_hip.so: the MI355X (gfx950) kernels of the PeCLR
 * pretraining hot path.
 *
 * The reference (dahiyaaneesh/peclr) is pure Python and has NO FFI of its own: every op on
 * its hot path is a chain of stock PyTorch ops.  This header is therefore the boundary a
 * native replacement exports, one entry point per op chain of SURVEY.md section 2.2
 * (K1..K8); each declaration cites the reference lines it replaces (paths relative to the
 * reference root).  INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller; the library never allocates
 *     or frees memory; scratch buffers are caller-provided (sized with the *_jsplit /
 *     *_pick_split_k policy queries).  Buffers are row-major, contiguous, 16-byte aligned.
 *   - one entry point = one kernel launch (so a HIP-event pair around a call times exactly
 *     the kernel that rocprofv3 reports).
 *   - every call is asynchronous on the given hipStream_t (`stream`), re-entrant, keeps no
 *     global mutable state, and may be called concurrently on different streams.
 *   - return value: 0 = ok; negative = argument error (PECLR_ERR_*); positive = hipError_t
 *     of the failed launch.  No exceptions cross the ABI.
 *   - "slabs": a split-K producer writes S partial results [S][rows][cols]; the consuming
 *     kernel sums them on load (fused reduction).  S == 1 means a plain dense tensor.
 *   - row layout of two-view tensors: rows [0,N) are view-1 samples, rows [N,2N) view-2
 *     samples (hybrid2_model.py:30-32).  Multi-GPU gathered tensors repeat that block per
 *     rank; `n_half` (= N per rank) defines the positive-pair map: partner(i) = i + n_half
 *     if (i / n_half) is even else i - n_half.
 */
#ifndef PECLR_HIP_H
#define PECLR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* peclr_stream_t; /* hipStream_t */

#define PECLR_OK 0
#define PECLR_ERR_NULL (-1)        /* required pointer is null */
#define PECLR_ERR_SHAPE (-2)       /* unsupported / inconsistent shape */
#define PECLR_ERR_ALIGN (-3)       /* pointer or leading dimension not 16-byte aligned */
#define PECLR_ERR_WORKSPACE (-4)   /* workspace too small */
#define PECLR_ERR_UNSUPPORTED (-5) /* unsupported flag / dtype */

/* GEMM operand layouts: C[M,N] = A . B  with                                              */
#define PECLR_GEMM_NT 0 /* A[M,K] row-major, B[N,K] row-major  (y = x W^T : nn.Linear fwd) */
#define PECLR_GEMM_NN 1 /* A[M,K] row-major, B[K,N] row-major  (dx = dy W)                 */
#define PECLR_GEMM_TN 2 /* A[K,M] row-major, B[K,N] row-major  (dW = dy^T x)               */

/* align flags */
#define PECLR_ALIGN_CROP 1        /* "crop" in config.augmentation   (hybrid2_model.py:58)  */
#define PECLR_ALIGN_ROTATE 2      /* "rotate" in config.augmentation (hybrid2_model.py:76)  */
#define PECLR_ALIGN_SINGLE_NORM 4 /* SimCLR.contrastive_step: one F.normalize, no alignment
                                     (simclr_model.py:44-47)                                */

int peclr_version(void);
const char* peclr_error_string(int code);
/* Identity of the hipGraph capture `stream` is in (*id_out = 0: not capturing).  Plumbing for the host side, which packs
 * the six-product GEMMs' weight planes once per optimiser step AND once per capture (no reference counterpart: the
 * reference launches eagerly, peclr_training.py:96). */
int peclr_stream_capture_id(void* stream, unsigned long long* id_out);

/* ---- K1 / K2-GEMM and their backward GEMMs -------------------------------------------
 * Replaces nn.Linear forward/backward of the projection head (simclr_model.py:22-26,29-33).
 * fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32 (bit-exact fmaf chain).
 * split_k == 1: C = A.B (+ bias[N] if non-null).  split_k > 1: slabs[s] (each [M,N], ld = N)
 * receive the K-partials, C and bias are ignored (the consumer adds the bias).
 * Feature dimensions (the contiguous dimension of each operand, and N) must be multiples
 * of 4; M (batch rows) is arbitrary.                                                      */
int peclr_gemm_f32(int layout, int M, int N, int K, const float* A, int lda, const float* B,
                   int ldb, float* C, int ldc, const float* bias, int split_k, float* slabs,
                   peclr_stream_t stream);
/* The library's own split-K policy for a given problem (>= 1). */
/* C = op(A) op(B) + addend (same layouts as peclr_gemm_f32, no split-K): the 1x1-convolution input
 * gradient of a bottleneck's first conv with the residual branch's gradient added in the epilogue,
 * dX[R,Cin] = dY[R,Cmid] W[Cmid,Cin] + dRes[R,Cin] -- what autograd otherwise does as MIOpen dgrad +
 * a separate elementwise add over the block input (torchvision Bottleneck, resnet_model.py:15). */
int peclr_gemm_add_f32(int layout, int M, int N, int K, const float* A, int lda, const float* B,
                       int ldb, float* C, int ldc, const float* addend, int ldd,
                       peclr_stream_t stream);
/* The same for bf16 (autocast) backbones: C (bf16) = A[M,K] (bf16) . B[N,K]^T (bf16) + addend (bf16,
 * nullable), fp32 accumulation on v_mfma_f32_32x32x16_bf16; both operands K-contiguous (pass the
 * 1x1 weight transposed, [Cin][Cmid]); K, lda, ldb multiples of 8. */
int peclr_gemm_add_bf16(int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C,
                        int ldc, const void* addend, int ldd, peclr_stream_t stream);
/* the same kernel for IEEE fp16 activations (precision=16 / native AMP): v_mfma_f32_32x32x16_f16 */
int peclr_gemm_add_f16(int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C,
                        int ldc, const void* addend, int ldd, peclr_stream_t stream);
/* fp32 GEMM on the bf16 matrix cores, fp32 accuracy: C[M,N] = A[M,K] . B[N,K]^T (+ addend[M,N], nullable), all fp32,
 * both operands K-contiguous.  Every fp32 operand is split EXACTLY into three bf16 numbers (x = h + m + l by
 * truncation); six of the nine partial products run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, the three
 * dropped ones are <= 2^-24 of the product (one fp32 rounding).  2.67x the fp32 MFMA rate.  Serves the GEMM-shaped fp32
 * work of the backbone (same call sites as peclr_gemm_add_f32: the 1x1-convolution input gradient + residual gradient;
 * and the 1x1 convolutions of the torchvision Bottleneck, resnet_model.py:15).  K, lda, ldb multiples of 4.       */
int peclr_gemm_x6_f32(int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                      const float* addend, int ldd, peclr_stream_t stream);
/* The 1x1 weight gradient on the same scheme: dW[M=Cout, N=Cin] = A[K=R, M]^T . B[K=R, N] with A = dY and B = X as they
 * lie in NHWC memory (K is the slow dimension of both; lda >= M, ldb >= N; M, N, lda, ldb multiples of 4).  K is split
 * over peclr_gemm_x6_tn_slabs(M, N, K) workgroup rows, each writing one fp32 slab [M][N]; add them with
 * peclr_slab_reduce_f32 (fixed order: the result is deterministic, unlike the atomically accumulated split-K weight
 * gradients of the library kernels).  Replaces MIOpen's fp32 weight gradient of the 1x1 convolutions.            */
int peclr_gemm_x6_tn_slabs(int M, int N, int K);
int peclr_gemm_x6_tn_f32(int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* slabs,
                         int n_slabs, peclr_stream_t stream);
/* Optional fusion of a BatchNorm2d(+ReLU) layer's backward REDUCTION into the GEMM that produces the gradient arriving at
 * that layer (the input gradient of the convolution that consumed the layer's output): host struct of device pointers.
 * The epilogue sums, per row block and column, dY' and dY' * xhat (dY' = dY where the ReLU passed -- recomputed from the
 * layer's input x with scale / shift, or read from its 1-bit mask; xhat = (x - mean) * invstd) into
 * partial[ceil(M / tile_rows)][2][N], the layout peclr_bn2d_bwd_finalize_f32 combines with n_split = ceil(M / tile_rows):
 * the separate peclr_bn2d_bwd_reduce pass over dY and x is not needed.  Fixed summation order. */
typedef struct {
    const float* x;             /* the layer's input [M][N], contiguous */
    const float* mean;          /* [N] */
    const float* invstd;        /* [N] */
    const float* scale_shift;   /* [2][N] of the forward */
    const uint32_t* relu_mask;  /* [M][N / 32] or NULL (mask recomputed from x) */
    int relu;
    float* partial;
} peclr_bn_bwd_fuse;

/* "Pair" arithmetic of the packed-weight GEMMs below (round 6; every entry point that takes `pair`: NULL = the six-product
 * arithmetic on planes of peclr_x6_pack_f32).  Non-NULL: Bp holds planes of peclr_x6_pack_pair_f32 -- the weight multiplied by a
 * power of two (*w_scale) and split into TWO fp16 numbers hi + lo -- and the activation operand is scaled and split the same way in
 * the kernel by the power of two that puts *a_absmax (= max |A| over the whole tensor; written by the pass that produced A:
 * `absmax_out` of the peclr_bn2d_* entry points) into [2^14, 2^15).  Three products (hi.hi, hi.lo, lo.hi) on
 * v_mfma_f32_32x32x16_f16 with fp32 accumulation instead of six on the bf16 instruction; the accumulators are multiplied by
 * 1 / (s_a s_w) (exact).  22 - 23 of fp32's 24 significand bits per operand: error against float64 in the class of an fp32 BLAS
 * GEMM (measured per layer on real tensors: tools/exp/fp16_pair_probe.py, tools/exp/pair_probe.py).
 * Both pointers are DEVICE pointers to one float, read by the kernel: no host synchronisation.                                 */
typedef struct {
    const float* a_absmax;
    const float* w_scale;
} peclr_x6_pair;

/* Second generation of the same scheme for a WEIGHT operand (a parameter: constant for a whole step, used by forward,
 * input gradient and fused entry gradient of a 1x1 convolution, resnet_model.py:15): peclr_x6_pack_f32 splits the
 * weight ONCE into three bf16 planes in MFMA fragment order (per 128 output columns x 16 k one 12 KiB chunk of twelve
 * 1 KiB pieces [32-column block][plane]); peclr_gemm_x6p_f32 streams those chunks into LDS by LDS-DMA and only splits the
 * activation operand in the kernel (once per 128 output columns, by the one wave that owns the row).
 *   desc_table: DEVICE array of `count` entries of 8 int64 {src fp32 matrix, dst planes, n, k, ld (floats), transposed,
 *   first chunk, 0}; B_t[n][k] = src[n * ld + k] (transposed = 0: forward, W[Cout][Cin]) or src[k * ld + n]
 *   (transposed = 1: input gradients, B_t = W^T) or, for a T-tap filter W[Cout][T][Cin] read for its input gradient,
 *   transposed = T: B_t[ci][tap * Cout + co] = src[(co * T + tap) * ld + ci]; n % 128 == 0, k % 16 == 0; chunks per matrix = (n / 128) * (k / 16);
 *   dst holds peclr_x6_pack_bytes(n, k) = 6 n k bytes.  One launch packs every matrix of the table.
 *   peclr_gemm_x6p_f32: C[M,N] = A[M,K] . B_t^T (+ addend); tile_rows 256, 128 or 0 (= peclr_gemm_x6p_tile_rows).
 *   stat_partial (nullable; needs stat_shift[N]): the training-mode BatchNorm2d statistics of C (the `conv -> bn` pair of
 *   the torchvision Bottleneck, resnet_model.py:15) from the accumulators, so that no separate pass re-reads the tensor
 *   the GEMM just wrote: float [ceil(M / tile_rows)][2][N] per-row-block sums of (C - shift) and (C - shift)^2, then one
 *   row [N] holding the shift -- exactly the `partial` layout of peclr_bn2d_stats, so peclr_bn2d_finalize_f32 (or the
 *   synchronised route's peclr_bn2d_combine_f64) takes it with n_split = ceil(M / tile_rows).  Fixed summation order. */
int64_t peclr_x6_pack_bytes(int N, int K);
int peclr_x6_pack_f32(const void* desc_table, int count, int total_chunks, peclr_stream_t stream);
/* ... and as fp16 pairs (see peclr_x6_pair): same descriptor table, dst of peclr_x6_pack_pair_bytes(n, k) = 4 n k bytes (8 KiB
 * chunks of eight pieces [32-column block][hi | lo]).  Two launches over the same grid: peclr_x6_absmax_f32 leaves max |W| of
 * matrix d in absmax[d] (float [count]); peclr_x6_pack_pair_f32 multiplies matrix d by the power of two that maximum gives,
 * splits, and leaves the power of two in scales[d] (float [count]: what the GEMMs take as peclr_x6_pair.w_scale).              */
int64_t peclr_x6_pack_pair_bytes(int N, int K);
int peclr_x6_absmax_f32(const void* desc_table, int count, int total_chunks, float* absmax, peclr_stream_t stream);
int peclr_x6_pack_pair_f32(const void* desc_table, int count, int total_chunks, const float* absmax, float* scales,
                           peclr_stream_t stream);
int peclr_gemm_x6p_tile_rows(int M, int N, int K);
int peclr_gemm_x6p_f32(int M, int N, int K, const float* A, int lda, const void* Bp, float* C, int ldc,
                       const float* addend, int ldd, int tile_rows, const float* stat_shift, float* stat_partial,
                       const peclr_bn_bwd_fuse* bn_bwd, const peclr_x6_pair* pair, peclr_stream_t stream);
/* The same product when the addend is the COMPACT input gradient of a 1x1 / stride-2 convolution: the M rows are the pixels
 * of H x W images (H, W even, M a multiple of H * W), addend_half = [images][H / 2][W / 2][ldd], and only the rows at even
 * (h, w) add addend_half[(h / 2, w / 2)].  This is the entry gradient of a ResNet layer's first block -- dY1 . W1 (main
 * branch) + the shortcut's transposed convolution -- without the 4x larger, three-quarters-zero tensor MIOpen's strided
 * input gradient writes and the addend pass reads (resnet_model.py:15; torchvision Bottleneck.downsample).               */
int peclr_gemm_x6p_s2add_f32(int M, int N, int K, const float* A, int lda, const void* Bp, float* C, int ldc,
                             const float* addend_half, int ldd, int H, int W, int tile_rows, const peclr_bn_bwd_fuse* bn_bwd,
                             const peclr_x6_pair* pair, peclr_stream_t stream);
/* ... and when the addend is a gradient that still has to pass a ReLU: addend_mask = the 1-bit mask peclr_bn2d_apply wrote
 * for that ReLU ([M][N / 32] words, bit c % 32 of word c / 32 = output c was positive); addend elements whose bit is clear
 * count as zero.  This is the entry gradient of a residual block whose shortcut is the identity: dY1 . W1 +
 * relu'(out) * d(out) -- the second term is what the block's last BatchNorm backward would otherwise write out as the
 * residual's gradient (4 B per element written, then read back here).  N % 32 == 0.                                       */
int peclr_gemm_x6p_maskadd_f32(int M, int N, int K, const float* A, int lda, const void* Bp, float* C, int ldc,
                               const float* addend, int ldd, const unsigned* addend_mask, int tile_rows,
                               const peclr_bn_bwd_fuse* bn_bwd, const peclr_x6_pair* pair, peclr_stream_t stream);
/* 3x3 / stride-1 / padding-1 convolution of an NHWC fp32 tensor (the middle convolution of the torchvision Bottleneck,
 * resnet_model.py:15) as an implicit GEMM on the same kernel: rows = output pixels, K = 9 * Cin ordered (tap, channel); the
 * activation rows of a k-step come from the pixel the tap points at (zeros outside the image: `zeros` = >= 64 bytes of
 * zeros), the weights from planes packed out of W[Cout][3][3][Cin] (channels_last storage) seen as [Cout][9 * Cin].
 * flip = 1 computes the INPUT GRADIENT dX = conv(dY, flipped filter): pass dY as X, Cin := Cout, Cout := Cin and planes
 * packed with `transposed` = 9 (B_t[ci][tap * Cout + co] = W[co][tap][ci]).  addend, tile_rows and the BatchNorm
 * statistics outputs as in peclr_gemm_x6p_f32.  Cin % 16 == 0, Cout % 128 == 0.                                      */
int peclr_conv3x3_x6p_f32(int NB, int H, int W, int Cin, int Cout, const float* X, const void* Bp, float* Y,
                          const float* addend, int flip, int tile_rows, int variant, const float* zeros, const float* stat_shift,
                          float* stat_partial, const peclr_bn_bwd_fuse* bn_bwd, const peclr_x6_pair* pair, peclr_stream_t stream);
/* (variant 0: every wave loads and splits its rows once per tap; 1: per 16-channel chunk the workgroup splits the pixels its
 *  nine taps touch once into shared planes and the taps read their fragments at the tap's offset -- W <= 64, else as 0.)  */
/* Weight gradients, second generation: C[M, taps * N] = sum_k A[k, M] . B[k shifted by the tap, N], the contraction over the
 * ROWS of two NHWC activations (A = dY [R, Cout], B = X [R, Cin]).  taps = 1: dW = dY^T X of a 1x1 convolution.  taps = 9:
 * the nine [Cout, Cin] products of a 3x3 / stride-1 / padding-1 convolution's weight gradient, X read at the pixel each
 * tap points at (H x W images, K = images * H * W rows; zeros outside the image: `zeros` = >= 64 bytes of zeros), written
 * as columns tap * N + n -- the [Cout][3][3][Cin] storage of a channels_last weight.  K is split over
 * peclr_gemm_x6t_slabs(M, N, K, taps) workgroup rows, each writing one fp32 slab [M][taps * N]; peclr_slab_reduce_f32 adds
 * them in a fixed order (deterministic).  256 x 256 output tiles where the problem has them (an operand row is split once
 * per 256 columns of the other operand), k-step 16 with double-buffered planes; 64-wide sides (layer1) get 64 x 256 /
 * 256 x 64 / 64 x 128 tiles and, for taps = 9, a 64 x 64 block with the taps in two halves.  stride = 2 (the first block of
 * layers 2-4): A's K rows are the H x W OUTPUT pixels, B's 4 K rows the pixels of the 2H x 2W inputs, read at
 * (2 oh + dh, 2 ow + dw) (taps = 1: the 1x1 shortcut, dh = dw = 0; taps = 9: padding 1).  M, N, lda, ldb multiples of 4;
 * W >= 6 when taps = 9 or stride = 2.  Replaces MIOpen's fp32 weight gradients of the Bottleneck's convolutions
 * (resnet_model.py:15).                                                                                                  */
int peclr_gemm_x6t_slabs(int M, int N, int K, int taps);
int peclr_gemm_x6t_f32(int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* slabs, int n_slabs,
                       int taps, int H, int W, int stride, const float* zeros, peclr_stream_t stream);
/* Input gradient of the 3x3 / padding-1 / STRIDE-2 convolution of a layer's first block (resnet_model.py:15), on the same
 * kernel: dY [NB, Ho, Wo, Cout] NHWC -> dX [NB, 2 Ho, 2 Wo, Cin].  Input pixel (2 i + ph, 2 j + pw) receives filter row a only
 * where ph + 1 - a is even, so the transposed convolution splits into four dense ones, one per parity class (ph, pw), with
 * 1, 2, 2 and 4 taps (gridDim.y = class): the same 9 Cout multiply-adds per OUTPUT pixel as the forward, none against the
 * zeros a dilated gradient would hold.  Bp: planes of the filter packed for the input gradient (peclr_x6_pack_f32,
 * transposed = 9, as for peclr_conv3x3_x6p_f32 with flip).  bn_bwd: dX is the gradient arriving at that BatchNorm layer
 * (partial: 4 * ceil(NB Ho Wo / tile_rows) row blocks, class by class).  Cin % 64 == 0, Cout % 16 == 0.  Replaces MIOpen's
 * igemm_bwd on these three convolutions.                                                                                  */
int peclr_conv3x3_s2_dgrad_x6p_f32(int NB, int Ho, int Wo, int Cout, int Cin, const float* dY, const void* Bp, float* dX,
                                   int tile_rows, const float* zeros, const peclr_bn_bwd_fuse* bn_bwd, const peclr_x6_pair* pair,
                                   peclr_stream_t stream);
/* Forward of the STRIDE-2 convolutions of a ResNet layer's first block on the same kernel: taps = 9 the 3x3 / padding-1
 * convolution, taps = 1 the 1x1 downsample convolution; X [NB, H, W, Cin] NHWC (H, W even), Y [NB, H/2, W/2, Cout]; output pixel
 * (oh, ow) reads input pixel (2 oh + dh, 2 ow + dw).  Planes packed as for the stride-1 forward; optional BatchNorm
 * statistics of Y.  (Weight gradients: peclr_gemm_x6t_f32 with stride = 2; input gradients: above / peclr_gemm_x6p_s2add_f32.)  */
int peclr_conv_s2_x6p_f32(int NB, int H, int W, int Cin, int Cout, int taps, const float* X, const void* Bp, float* Y,
                          int tile_rows, const float* zeros, const float* stat_shift, float* stat_partial,
                          const peclr_x6_pair* pair, peclr_stream_t stream);
int peclr_gemm_pick_split_k(int M, int N, int K);

/* out[i] = sum_s slabs[s][i] (+ bias[i % cols] if non-null), i < rows*cols. */
int peclr_slab_reduce_f32(const float* slabs, int n_slabs, int rows, int cols, const float* bias,
                          float* out, peclr_stream_t stream);

/* ---- K2: BatchNorm1d (train or eval) + ReLU --------------------------------------------
 * Replaces nn.BatchNorm1d(H) + nn.ReLU (simclr_model.py:27-28).  Input = split-K slabs of
 * the first Linear plus its bias.  training != 0: batch statistics over all M rows (biased
 * variance), running stats updated with momentum and the unbiased variance,
 * num_batches_tracked incremented (all three nullable).  training == 0: running stats.
 * Outputs: a_pre [M,H] (pre-BN activations, kept for the backward), a_out [M,H],
 * save_mean[H], save_invstd[H].                                                           */
int peclr_bn_relu_fwd_f32(const float* a_slabs, int n_slabs, const float* bias, int M, int H,
                          const float* gamma, const float* beta, float eps, float momentum,
                          int training, float* running_mean, float* running_var,
                          int64_t* num_batches_tracked, float* a_pre, float* a_out,
                          float* save_mean, float* save_invstd, peclr_stream_t stream);
/* Backward of the above: d_a_out -> d_a_pre [M,H], dgamma, dbeta, dbias[H].  training != 0:
 * batch statistics took part in the forward (full BN backward); training == 0: the statistics
 * were constants (frozen BN).                                                               */
int peclr_bn_relu_bwd_f32(const float* d_a_out, const float* a_pre, const float* save_mean,
                          const float* save_invstd, const float* gamma, const float* beta, int M,
                          int H, int training, float* d_a_pre, float* dgamma, float* dbeta,
                          float* dbias, peclr_stream_t stream);

/* ---- K3..K7: projection stats + normalise + un-translate + un-rotate + normalise -------
 * Replaces Hybrid2Model.get_projection_stats / F.normalize / translate_encodings /
 * rotate_encoding / F.normalize (hybrid2_model.py:40-85, utils.py:271-346).
 * p_slabs: [n_slabs][M][D] split-K partials of the second Linear.  D must be 128.
 * jitter_*: int64 [n_pairs] per view exactly as the batch dict holds them
 * (data_set.py:357-384); extent_x / extent_y are float(image_shape[0]) / float(shape[1]).
 * angle1/2: float64 [n_pairs] per view, NOT negated (the kernel applies the minus signs of
 * hybrid2_model.py:74,80).  Pointers of disabled flags may be null.
 * Outputs: p_out [M,D] (reduced raw projections), z_out [M,D], norms [2][M] (clamped
 * ||p|| and clamped post-alignment norm), row_stats [M][8] per-sample
 * {x_mean,x_median,x_min,x_max,y_mean,y_median,y_min,y_max} (nullable).                   */
int peclr_align_fwd_f32(const float* p_slabs, int n_slabs, int M, int D, int n_pairs, int flags,
                        const int64_t* jitter_x1, const int64_t* jitter_x2,
                        const int64_t* jitter_y1, const int64_t* jitter_y2, float extent_x,
                        float extent_y, const double* angle1, const double* angle2, float* p_out,
                        float* z_out, float* norms, float* row_stats, peclr_stream_t stream);
/* Backward: dz [M,D] -> dp [M,D].  Range and centroid are constants (utils.py:312,338-339). */
int peclr_align_bwd_f32(const float* dz, const float* p, const float* z, const float* norms, int M,
                        int D, int n_pairs, int flags, const double* angle1, const double* angle2,
                        float* dp, peclr_stream_t stream);

/* ---- K8: NT-Xent ------------------------------------------------------------------------
 * Replaces vanila_contrastive_loss (utils.py:154-186) without materialising S, exp(S), the
 * mask or the M x (M-1) gather.  One entry point per kernel launch.
 * z_rows: the Mr rows this call owns (global row index = row_offset + r); z_all: all Mg rows
 * (negatives).  Single GPU: z_rows == z_all, Mr == Mg, row_offset == 0.
 *
 * peclr_ntxent_jsplit: the library's column-split policy (how many key-column slices the
 * grid is split into) for the forward (backward == 0) or backward (backward != 0) launch;
 * callers size `partial` / `dz_slabs` with it.
 * peclr_ntxent_fwd_f32: partial[jsplit][Mr] = per-slice sums of exp(S_ij/tau) over j != i,
 * pos[Mr] = S_{i,partner(i)}/tau; sim_out (nullable): [Mr][Mg] per-pair similarities.
 * peclr_ntxent_finalize_f32 (one workgroup, fixed summation order): row_lse[Mr] =
 * log sum_s partial[s][r]; out17[16] = loss_scale * sum_r (row_lse[r] - pos[r]); when row_stats
 * is non-null, out17[0..15] = the batch-mean projection statistics (hybrid2_model.py:92-106)
 * of the [2*n_pairs_stats][8] row_stats matrix.
 * peclr_ntxent_bwd_f32: dz_slabs[s][Mr][D] = per-slice partials of
 *   (*dloss) * grad_scale * inv_tau * sum_{j != i} [e_ij (1/neg_i + 1/neg_j) - 2 [j == partner(i)]] z_j
 * (sum the slabs with peclr_slab_reduce_f32; jsplit == 1 writes the dense dz directly).
 * lse_all[Mg] = row_lse of every global row (all-gathered on multi-GPU); grad_scale = 1/Mg for
 * the reference's mean reduction; dloss: device scalar (the incoming gradient of the loss).  */
int peclr_ntxent_jsplit(int Mr, int Mg, int backward);
int peclr_ntxent_fwd_f32(const float* z_rows, int Mr, int row_offset, const float* z_all, int Mg,
                         int D, int n_half, float inv_tau, float* sim_out, float* partial,
                         float* pos, int jsplit, peclr_stream_t stream);
int peclr_ntxent_finalize_f32(const float* partial, int jsplit, const float* pos, int Mr,
                              float loss_scale, float* row_lse, const float* row_stats,
                              int n_pairs_stats, float* out17, peclr_stream_t stream);
int peclr_ntxent_bwd_f32(const float* z_rows, int Mr, int row_offset, const float* z_all, int Mg,
                         int D, int n_half, float inv_tau, const float* lse_all,
                         const float* dloss, float grad_scale, float* dz_slabs, int jsplit,
                         peclr_stream_t stream);

/* ---- optimiser: LARSWrapper(Adam) fused over a list of tensors --------------------------
 * Replaces pl_bolts LARSWrapper.step + torch.optim.Adam.step as wired by
 * BaseModel.configure_optimizers (base_model.py:57-104).  Two launches per parameter group
 * instead of ~15 launches + 2 host syncs per tensor.
 * ptrs: device array [4][n_tensors] of float* {param, grad, exp_avg, exp_avg_sq};
 * sizes: device array [n_tensors] of int64 element counts.  The work list is n_chunks chunks
 * of at most PECLR_OPT_CHUNK elements: chunk_tensor[c] / chunk_offset[c] give the tensor and
 * the element offset of chunk c (chunks of one tensor are consecutive), and
 * tensor_chunk_begin[t] .. tensor_chunk_begin[t+1] is tensor t's chunk range.
 * peclr_lars_sumsq_f32: norms_ws[2][n_chunks] = per-chunk sums of squares of param and grad.
 * peclr_lars_adam_update_f32: ONE launch for all parameter groups (the reference has two: decayed /
 * not decayed, base_model.py:30-51): tensor_group[t] (device, nullable when n_groups == 1) selects
 * the tensor's entry of the HOST arrays group_lr / group_weight_decay (n_groups <= 8, copied into
 * the kernel arguments).  It combines a tensor's chunk sums in a fixed order (bit-reproducible),
 * applies the LARS trust ratio + weight decay and the Adam update.
 * device_hyper (nullable): DEVICE float[18] = {lr[8], weight_decay[8], bias_corr1, bias_corr2}; when
 * given it overrides the by-value scalars, so a hipGraph that captured the launch can be replayed
 * with new per-step values.
 * use_lars == 0: plain Adam with L2 weight decay (torch.optim.Adam semantics; norms_ws unused).
 * use_lars == 2: LARS, and the scaled gradient (g + wd*p)*trust is ALSO written back over grad, as
 * pl_bolts' LARSWrapper.update_p leaves it (it mutates p.grad in place before the wrapped Adam
 * step); with use_lars == 1 it is consumed in registers only (4 B/param less traffic).
 * bias_corr1/2 = 1 - beta^step, computed by the host.                                        */
#define PECLR_OPT_CHUNK 4096
int peclr_lars_sumsq_f32(float* const* ptrs, const int64_t* sizes, int n_tensors,
                         const int32_t* chunk_tensor, const int64_t* chunk_offset, int n_chunks,
                         float* norms_ws, peclr_stream_t stream);
int peclr_lars_adam_update_f32(float* const* ptrs, const int64_t* sizes, int n_tensors,
                               const int32_t* chunk_tensor, const int64_t* chunk_offset,
                               const int32_t* tensor_chunk_begin, const int32_t* tensor_group,
                               int n_chunks, const float* norms_ws, const float* device_hyper,
                               const float* group_lr, const float* group_weight_decay, int n_groups,
                               float beta1,
                               float beta2, float adam_eps, float bias_corr1, float bias_corr2,
                               int use_lars, float lars_eta, float lars_eps, int lars_clip,
                               peclr_stream_t stream);

/* ---- precision=16: the dynamic loss scaler folded into the optimiser step -------------------
 * Replaces torch.cuda.amp.GradScaler.unscale_/step/update around the optimiser, which Lightning 1.0.8's
 * native-AMP plugin runs when the reference trains at its default `precision: 16`
 * (training_config.json:9, peclr_training.py:78-79).  GradScaler.step reads found_inf back to the host to
 * decide whether to step; here the decision is taken on the device, so the step can live in a hipGraph:
 *   peclr_lars_sumsq_amp_f32        the gradients hold scale*g: norms of g = grad/scale, and
 *                                   amp->found_inf = 1 if any gradient element is inf / nan;
 *   peclr_lars_adam_update_amp_f32  returns without touching param / moments when found_inf is set (with
 *                                   use_lars == 2 it leaves grad/scale in grad, as unscale_ does); else the
 *                                   update on grad/scale with bias corrections 1 - beta^(good_steps + 1), evaluated in
 *                                   double from the double betas (bit-equal to the host's `1 - beta ** step`);
 *   peclr_amp_update                GradScaler.update: found_inf ? scale *= backoff, tracker = 0
 *                                   : (good_steps += 1; ++tracker == interval ? scale *= growth, tracker = 0),
 *                                   then found_inf = 0.  One thread.
 * Launch the three in this order on one stream.  `amp` is DEVICE memory, 16 bytes, owned by the caller
 * (initialise scale = 65536, the rest 0 for torch's defaults).                                         */
typedef struct peclr_amp_state {
    float scale;          /* current loss scale                                   */
    float found_inf;      /* 0 / 1, raised by the sumsq pass, cleared by update   */
    int32_t growth_tracker; /* consecutive steps without inf / nan                */
    int32_t good_steps;   /* optimiser steps actually taken (Adam's `step`)       */
} peclr_amp_state;
int peclr_lars_sumsq_amp_f32(float* const* ptrs, const int64_t* sizes, int n_tensors,
                             const int32_t* chunk_tensor, const int64_t* chunk_offset, int n_chunks,
                             float* norms_ws, peclr_amp_state* amp, peclr_stream_t stream);
int peclr_lars_adam_update_amp_f32(float* const* ptrs, const int64_t* sizes, int n_tensors,
                                   const int32_t* chunk_tensor, const int64_t* chunk_offset,
                                   const int32_t* tensor_chunk_begin, const int32_t* tensor_group,
                                   int n_chunks, const float* norms_ws, const float* device_hyper,
                                   const float* group_lr, const float* group_weight_decay, int n_groups,
                                   double beta1, double beta2, float adam_eps, int use_lars, float lars_eta,
                                   float lars_eps, int lars_clip, const peclr_amp_state* amp,
                                   peclr_stream_t stream);
int peclr_amp_update(peclr_amp_state* amp, float growth_factor, float backoff_factor, int growth_interval,
                     peclr_stream_t stream);

/* ---- backbone glue: fused BatchNorm2d (+ residual add) (+ ReLU), NHWC --------------------
 * Replaces nn.BatchNorm2d + `out += identity` + nn.ReLU between the convolutions of the
 * torchvision ResNet blocks the reference builds (resnet_model.py:15, norm_layer=nn.BatchNorm2d).
 * Activations are NHWC (torch.channels_last): x, residual, y, dy, dx, d_residual are row-major
 * [R = N*H*W][C] of io_dtype (PECLR_DTYPE_F32, or PECLR_DTYPE_BF16 / PECLR_DTYPE_F16 for autocast backbones);
 * statistics, parameters and arithmetic are fp32.  With W = 4 (fp32) / 8 (bf16) channels per
 * 16-byte word, C/W must divide 256 or be a multiple of it (every ResNet width).
 * One entry point = one launch:
 *   forward (training): peclr_bn2d_stats -> peclr_bn2d_finalize_f32 -> peclr_bn2d_apply
 *   forward (eval)    :                     peclr_bn2d_finalize_f32 -> peclr_bn2d_apply
 *   backward          : peclr_bn2d_bwd_reduce -> peclr_bn2d_bwd_finalize_f32 -> peclr_bn2d_bwd_apply
 * partial (forward): [n_split*2 + 1][C] floats = row-slice partial sums (of x - shift and its
 * square) + one row holding the shift; shift (nullable): [C] vector to subtract, default = row 0
 * of x.  partial (backward): [n_split*2][C].  n_split from peclr_bn2d_n_split, or any >= 1.
 * Synchronised statistics across data-parallel ranks (optional; every rank passes the SAME shift,
 * e.g. running_mean): peclr_bn2d_stats -> peclr_bn2d_combine_f64 (totals: double [2*C+1]; the
 * caller stores its row count in the last element) -> the caller SUM-all-reduces totals -> peclr_bn2d_finalize_totals_f32; backward:
 * peclr_bn2d_bwd_reduce -> peclr_bn2d_combine_f64 -> all-reduce ->
 * peclr_bn2d_bwd_finalize_totals_f32 (dgamma/dbeta from the LOCAL totals, dx coefficients from the
 * GLOBAL ones).
 * scale_shift: [2][C] = {gamma*invstd, beta - mean*gamma*invstd}; coef: [2][C] scratch for dx.
 * ReLU mask in the backward: recomputed from x when neither y nor relu_mask is given (valid only
 * if no residual was added); read from relu_mask ([R][C/32] uint32, 1 bit per element, written by
 * peclr_bn2d_apply when its relu_mask argument is non-null; needs C % 32 == 0) or, failing that,
 * from the forward output y.  d_residual (nullable) receives the masked dy.
 * peclr_bn2d_finalize_f32 / peclr_bn2d_bwd_finalize_f32 REWRITE long partial tables (hence no const): with n_split >= 2048 the
 * rows are first summed in slices of 512 by a launch of their own that leaves each slice's sum in the slice's first row and
 * zeros in its other rows -- the table keeps its totals, so a second finalize / combine of the same table gives the same
 * result, but the individual row-block partials are gone.                                      */
#define PECLR_DTYPE_F32 0
#define PECLR_DTYPE_BF16 1
#define PECLR_DTYPE_F16 2   /* IEEE half: precision=16 (native AMP), the reference's default */
int peclr_bn2d_n_split(int R, int C, int io_dtype);
int peclr_bn2d_stats(const void* x, int io_dtype, int R, int C, const float* shift,
                     float* partial, int n_split, peclr_stream_t stream);
int peclr_bn2d_finalize_f32(float* partial, int n_split, int R, int C, int training,
                            float eps, float momentum, const float* gamma, const float* beta,
                            float* running_mean, float* running_var,
                            int64_t* num_batches_tracked, float* save_mean, float* save_invstd,
                            float* scale_shift, peclr_stream_t stream);
int peclr_bn2d_combine_f64(const float* partial, int n_split, int C, double* totals,
                           peclr_stream_t stream);
/* The eval-mode scale / shift tables of MANY BatchNorm2d layers in one launch (what an eval-mode peclr_bn2d_finalize_f32 writes
 * per layer, bit for bit: invstd = 1 / sqrtf(running_var + eps), scale = gamma * invstd, shift = beta - running_mean * scale).
 *   desc_table: DEVICE array of `count` entries of 8 int64 {gamma, beta, running_mean, running_var (fp32 [C] each), out (the
 *   flat fp32 output buffer), C | (bits of the float eps) << 32, offset (floats) of this layer's [2][C] table in `out`, number
 *   of channels of the entries before this one}; total_channels = the sum of C over the table. */
int peclr_bn2d_eval_tables(const void* desc_table, int count, int total_channels, peclr_stream_t stream);
int peclr_bn2d_finalize_totals_f32(const double* totals, const float* shift, int C,
                                   float eps, float momentum, const float* gamma, const float* beta,
                                   float* running_mean, float* running_var,
                                   int64_t* num_batches_tracked, float* save_mean,
                                   float* save_invstd, float* scale_shift, peclr_stream_t stream);
int peclr_bn2d_bwd_finalize_totals_f32(const double* local_totals, const double* global_totals,
                                       int C, int training, const float* scale_shift,
                                       float* dgamma, float* dbeta, float* coef,
                                       peclr_stream_t stream);
/* absmax_out (nullable, here and in the other passes that take it): the pass also leaves max |value it wrote| in *absmax_out -- one
 * atomic maximum per wave on a float its caller ZEROED beforehand (non-negative floats order like their bit patterns; a maximum
 * does not depend on the order, so the result is deterministic).  It costs the pass nothing measurable (it is HBM-bound) and is
 * what the "pair" GEMMs that consume the tensor take as peclr_x6_pair.a_absmax: every activation and every gradient a residual
 * block's convolution reads is written by one of these passes.                                                                  */
int peclr_bn2d_apply(const void* x, const void* residual, int io_dtype, int R, int C,
                     const float* scale_shift, int relu, void* y, uint32_t* relu_mask, float* absmax_out,
                     peclr_stream_t stream);
/* The last pass of a layer's FIRST block, whose shortcut is conv1x1 -> BatchNorm2d (torchvision Bottleneck.downsample behind
 * resnet_model.py:15): y = (relu)(bn(x) + bn_s(res_x)).  res_x is the INPUT of the shortcut's BatchNorm, res_scale_shift its
 * [2][C] table; the residual is fmaf(res_x, scale, shift) rounded to the storage format -- the value peclr_bn2d_apply would
 * have written and this pass read back, so the result is bit-identical -- and the shortcut's apply pass and output tensor
 * disappear.  relu_mask as in peclr_bn2d_apply.                                                                            */
int peclr_bn2d_apply_res_bn(const void* x, const void* res_x, const float* res_scale_shift, int io_dtype, int R, int C,
                            const float* scale_shift, int relu, void* y, uint32_t* relu_mask, float* absmax_out,
                            peclr_stream_t stream);
int peclr_bn2d_bwd_reduce(const void* dy, const void* x, const void* y, const uint32_t* relu_mask,
                          int io_dtype, int R, int C, int relu, const float* save_mean,
                          const float* save_invstd, const float* scale_shift, float* partial,
                          int n_split, peclr_stream_t stream);
int peclr_bn2d_bwd_finalize_f32(float* partial, int n_split, int R, int C, int training,
                                const float* scale_shift, float* dgamma, float* dbeta,
                                float* coef, peclr_stream_t stream);
int peclr_bn2d_bwd_apply(const void* dy, const void* x, const void* y, const uint32_t* relu_mask,
                         int io_dtype, int R, int C, int relu, const float* save_mean,
                         const float* save_invstd, const float* scale_shift, const float* coef,
                         void* dx, void* d_residual, float* absmax_out, peclr_stream_t stream);
/* Backward of peclr_bn2d_apply_res_bn (with relu): the apply passes of BOTH BatchNorm layers in one.  With d = relu_mask . dy -- the
 * d_residual peclr_bn2d_bwd_apply would write for the shortcut layer's backward to read back -- dx is peclr_bn2d_bwd_apply's result
 * for (dy, x, relu_mask) with the tables of the block's last layer, dxs its result for (d, xs, no ReLU) with the s_* tables of the
 * shortcut's layer, both bit for bit; d itself is never written.  The shortcut layer's sums come from peclr_bn2d_bwd_reduce on
 * (dy, xs, relu_mask) with its own statistics -- the same partial table as the reduction of d.  relu_mask is required (C % 32 == 0);
 * absmax_out / s_absmax_out: max |dx| / max |dxs| (nullable, fp32).                                                              */
int peclr_bn2d_bwd_apply_res_bn(const void* dy, const uint32_t* relu_mask, const void* x, const void* xs, int io_dtype,
                                int R, int C, const float* save_mean, const float* save_invstd,
                                const float* scale_shift, const float* coef, const float* s_save_mean,
                                const float* s_save_invstd, const float* s_scale_shift, const float* s_coef, void* dx,
                                void* dxs, float* absmax_out, float* s_absmax_out, peclr_stream_t stream);

/* Encoder tail: the last residual block's BatchNorm2d + `out += identity` + ReLU, then
 * AdaptiveAvgPool2d((1,1)) and `.flatten(1)` (features[7][-1].bn*, features[8] and the flatten of
 * ResNetModel.forward, resnet_model.py:24-26,47), as one pass that never writes the [N][HW][C]
 * activation: only `pooled` = its per-image channel means, fp32 [N][C] -- the encoder output the
 * projection head's first GEMM (peclr_gemm_f32, K1) reads directly -- and the 1-bit ReLU mask.
 * Forward: peclr_bn2d_stats -> peclr_bn2d_finalize_f32 (on x, R = N*HW) -> peclr_bn2d_apply_avgpool.
 * Backward: the pool's gradient is a broadcast, dy[n][p][c] = d_pooled[n][c] / HW, formed on the fly
 * (no [R][C] gradient tensor): peclr_bn2d_bwd_reduce_avgpool -> peclr_bn2d_bwd_finalize_f32 ->
 * peclr_bn2d_bwd_apply_avgpool (dx and d_residual = masked dy, both [R][C] of io_dtype).
 * Needs C % 32 == 0 and a residual (every ResNet's last block).                                  */
int peclr_bn2d_apply_avgpool(const void* x, const void* residual, int io_dtype, int N, int HW, int C,
                             const float* scale_shift, float* pooled, uint32_t* relu_mask,
                             peclr_stream_t stream);
int peclr_bn2d_bwd_reduce_avgpool(const float* d_pooled, const void* x, const uint32_t* relu_mask,
                                  int io_dtype, int N, int HW, int C, const float* save_mean,
                                  const float* save_invstd, const float* scale_shift, float* partial,
                                  int n_split, peclr_stream_t stream);
int peclr_bn2d_bwd_apply_avgpool(const float* d_pooled, const void* x, const uint32_t* relu_mask,
                                 int io_dtype, int N, int HW, int C, const float* save_mean,
                                 const float* save_invstd, const float* scale_shift, const float* coef,
                                 void* dx, void* d_residual, float* absmax_out, peclr_stream_t stream);

/* Stem: BatchNorm2d + ReLU + MaxPool2d(3, stride 2, padding 1) in one pass (features[1..3] of the
 * torchvision ResNet the reference wraps, resnet_model.py:15-26); x is [N][H][W][C] NHWC, the pooled
 * output [N][PH][PW][C] with PH = (H-1)/2 + 1.  The un-pooled activation is never written.  Forward:
 * peclr_bn2d_stats -> peclr_bn2d_finalize_f32 (as above, on x) -> peclr_bn2d_pool_apply, which also
 * writes, per pooled element, a 1-byte tap code (3*dh+dw of the first maximum, row-major, torch's
 * rule) and the x value at that maximum (x_at_max, same dtype/shape as y).  Backward:
 * peclr_bn2d_pool_bwd_reduce (a streaming reduction over dy and x_at_max; partial [n_split][2][C],
 * n_split from peclr_bn2d_pool_n_split or any >= 1) -> peclr_bn2d_bwd_finalize_f32 with R = N*H*W
 * -> peclr_bn2d_pool_bwd_apply (dx on the un-pooled grid: every element gathers from the <= 4
 * windows that hold it).  C/4 (fp32) or C/8 (bf16) must divide 256. */
int peclr_bn2d_pool_n_split(int N, int H, int W, int C, int io_dtype);
int peclr_bn2d_pool_apply(const void* x, int io_dtype, int N, int H, int W, int C,
                          const float* scale_shift, void* y, void* x_at_max, uint8_t* code, float* absmax_out,
                          peclr_stream_t stream);
int peclr_bn2d_pool_bwd_reduce(const void* dy_pool, const void* x_at_max, int io_dtype, int N, int H,
                               int W, int C, const float* save_mean, const float* save_invstd,
                               const float* scale_shift, float* partial, int n_split,
                               peclr_stream_t stream);
int peclr_bn2d_pool_bwd_apply(const void* dy_pool, const void* x, const uint8_t* code, int io_dtype,
                              int N, int H, int W, int C, const float* save_mean,
                              const float* save_invstd, const float* scale_shift, const float* coef,
                              void* dx, peclr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Two-view augmentation, pixel side.
 * Replaces, for a whole batch and both views at once, what SampleAugmenter.transform_sample does
 * per sample with OpenCV on CPU workers for the published recipe (reference
 * src/data_loader/sample_augmenter.py:47-129: rotate_sample :218-247 cv2.warpAffine, crop_sample
 * :166-186, resize_sample :188-216 cv2.resize INTER_AREA, color_jitter_sample :267-293 cv2 BGR<->HSV)
 * plus ToTensor + Normalize (src/data_loader/utils.py:283-293).  The parameter side (random draws,
 * crop box, rotation matrix) comes from the host by default, drawn from Python's `random` in the
 * reference's order (peclr_amd/augment.py), or -- for the recipe flags, TwoViewAugmenter(device_draws=True)
 * -- from peclr_augment_draw_views below, which writes the same `params` on the device.
 *
 * images : [B][H][W][3] uint8 (the reference's HWC images, one size per batch)
 * params : [n_views][B][PECLR_AUG_PARAM_DOUBLES] doubles per (view, sample):
 *            [0..5]  inverse (destination -> source) 2x3 affine of the rotation, row-major
 *            [6]     != 0: rotate            [7..10] crop window x0, y0, width, height (inside the image)
 *            [11]    != 0: colour jitter     [12..15] h, s, a, b factors
 * crops  : [n_views][B][H][W][3] uint8 scratch; only each window (at offset 0,0, row stride W) is written
 * out    : float32, logical shape [n_views*B][3][out_h][out_w]; channels_last != 0 stores it NHWC
 * mean/stdv : HOST pointers to 3 floats each (passed to the kernel by value).
 * 8-bit intermediates sit where the reference has them, so results are bit-identical to the
 * restatement in oracle/augment_oracle.py (whose pixel arithmetic is itself unpinned: OpenCV is
 * not available to check against). */
#define PECLR_AUG_PARAM_DOUBLES 16
int peclr_augment_warp_crop_u8(const uint8_t* images, int B, int H, int W, int n_views,
                               const double* params, uint8_t* crops, peclr_stream_t stream);
int peclr_augment_resize_color_norm(const uint8_t* crops, int B, int H, int W, int n_views,
                                    const double* params, int out_h, int out_w, const float* mean,
                                    const float* stdv, int channels_last, float* out,
                                    peclr_stream_t stream);

/* The reference's other five augmentations (sample_augmenter.py:67-84 sobel_filter / cut_out /
 * gaussian_blur before the rotation, :113-125 gaussian_noise / color_drop after the colour jitter),
 * TwoViewAugmenter(extended=True).  Used only for batches that draw one of them; the parameters
 * (decisions, cut-out box, blur taps, noise table) come from peclr_amd/augment.py.
 *
 * ext : [n_views][B][PECLR_AUG_EXT_INTS] ints per (view, sample):
 *         [0]     PECLR_AUG_EXT_* bits       [1..4] cut-out rows [r0, r1), columns [c0, c1)
 *         [5]     cut-out fill (0..254)       [6]    offset into `coefs` of the view's blur taps (-1: none)
 *         [7]     reserved (0)
 * coefs: Q8 Gaussian taps (sum 256) per blurred view: kx horizontal taps, then ky vertical ones
 *
 * peclr_augment_pre_u8 (stage 0, two launches when blur_tmp != NULL): images -> srcs
 *   [n_views][B][H][W][3] u8, in the reference's order Sobel (3x3 dx + dy of BGR2GRAY, reflect-101,
 *   low byte into all three channels), cut-out, Gaussian blur (separable, reflect-101; rows u8 x Q8
 *   into blur_tmp [n_views][B][H][W][3] u16, columns (sum + 2^15) >> 16).  Samples without a pre-op
 *   are copied.  kx, ky: the batch's odd kernel lengths, at most PECLR_AUG_MAX_BLUR_KSIZE.
 *   blur_tmp may be NULL only if no record has the blur bit (blur is then skipped).
 *   peclr_augment_warp_crop_u8 then runs once per view on srcs (n_views = 1).
 * peclr_augment_resize_color_norm_ext: peclr_augment_resize_color_norm, then per pixel and channel
 *   n = #{k < n_table : noise_table[k] <= u} with u from Philox4x32-10 (key = noise_seed, counter =
 *   (out pixel index, sample, view, call), output word = channel), pixel = (pixel + n) mod 256;
 *   then colour drop (BGR2GRAY into all three channels). */
#define PECLR_AUG_EXT_INTS 8
#define PECLR_AUG_EXT_SOBEL 1
#define PECLR_AUG_EXT_CUT_OUT 2
#define PECLR_AUG_EXT_BLUR 4
#define PECLR_AUG_EXT_NOISE 8
#define PECLR_AUG_EXT_COLOR_DROP 16
#define PECLR_AUG_MAX_BLUR_KSIZE 257
int peclr_augment_pre_u8(const uint8_t* images, int B, int H, int W, int n_views, const int* ext,
                         const int* coefs, int kx, int ky, uint8_t* srcs, uint16_t* blur_tmp,
                         peclr_stream_t stream);
int peclr_augment_resize_color_norm_ext(const uint8_t* crops, int B, int H, int W, int n_views,
                                        const double* params, const int* ext,
                                        const uint32_t* noise_table, int n_table, uint64_t noise_seed,
                                        uint32_t call, int out_h, int out_w, const float* mean,
                                        const float* stdv, int channels_last, float* out,
                                        peclr_stream_t stream);

/* The same four stages for a batch whose images DIFFER IN SIZE (the reference's YouTube-3D-Hands frames next to
 * FreiHAND's 224 x 224; TwoViewAugmenter with a RaggedImages or a list).  Per sample and per view the results are
 * bit-identical to what the entry points above give for that sample alone.  The kernels are the same code over
 * another geometry source; the launch count is the same (no launch per sample or per size).
 *
 * images : ONE packed uint8 buffer, the B images back to back, each [H_i][W_i][3]; image starts need no alignment.
 * geom   : device [B][PECLR_AUG_GEOM_INT64S] int64 per sample, computed by the HOST (peclr_amd/augment.py):
 *            [0] byte offset of the image in `images` (64-bit: a batch may exceed 2^31 bytes)
 *            [1] H_i   [2] W_i
 *            [3] kx_i  [4] ky_i  the image's own odd blur lengths (horizontal from H_i, vertical from W_i: the
 *                                reference's swap), at most PECLR_AUG_MAX_BLUR_KSIZE; read by stage 0 only.
 *                                A record's `coefs` offset points at kx_i horizontal taps, then ky_i vertical ones.
 * srcs / blur_tmp (stage 0): [n_views] copies of the packed layout, total_bytes uint8 / uint16 ELEMENTS per view;
 *   sample i of view v starts at element v * total_bytes + geom[i][0].
 * wins   : device [n_views][B][PECLR_AUG_WIN_INT64S] int64 per (view, sample), computed by the HOST, which knows every
 *          crop window before the launch:
 *            [0] byte offset of the window's first pixel in `crops`
 *            [1] row stride of the window in PIXELS (>= its width)
 *            [2] width, [3] height of the window -- the values of params[7..10]'s cw, ch; for the host (grid size,
 *                slicing a window out of the scratch), not read by the kernels
 * crops  : uint8 scratch addressed only through `wins`.  peclr_amd packs it: window after window, row stride = the
 *          window's width, sum of cw * ch * 3 bytes (the uniform scratch is n_views * B * H * W * 3).
 * Grids take their x, y extent from the batch maximum, passed from the host: max_h x max_w (images, stage 0),
 * max_ch x max_cw (windows, stage 1), out_h x out_w (stage 2).  max_kx, max_ky: the maxima of geom's [3], [4]
 * (checked odd and <= PECLR_AUG_MAX_BLUR_KSIZE, as kx, ky above).  With n_views = 1 and the per-view pointers
 * srcs + v * total_bytes, params + v * B * 16, wins + v * B * 4 (crops unchanged: wins' offsets are absolute) the warp
 * runs once per view after stage 0.  The noise counter stays (out pixel index, sample, view, call): a sample gets the
 * same noise at the same batch position whatever its source size. */
#define PECLR_AUG_GEOM_INT64S 5
#define PECLR_AUG_WIN_INT64S 4
int peclr_augment_pre_ragged_u8(const uint8_t* images, int B, int n_views, const int64_t* geom,
                                int64_t total_bytes, int max_h, int max_w, const int* ext,
                                const int* coefs, int max_kx, int max_ky, uint8_t* srcs,
                                uint16_t* blur_tmp, peclr_stream_t stream);
int peclr_augment_warp_crop_ragged_u8(const uint8_t* images, int B, int n_views, const int64_t* geom,
                                      const double* params, const int64_t* wins, int max_cw,
                                      int max_ch, uint8_t* crops, peclr_stream_t stream);
int peclr_augment_resize_color_norm_ragged(const uint8_t* crops, int B, int n_views,
                                           const int64_t* wins, const double* params, int out_h,
                                           int out_w, const float* mean, const float* stdv,
                                           int channels_last, float* out, peclr_stream_t stream);
int peclr_augment_resize_color_norm_ragged_ext(const uint8_t* crops, int B, int n_views,
                                               const int64_t* wins, const double* params,
                                               const int* ext, const uint32_t* noise_table,
                                               int n_table, uint64_t noise_seed, uint32_t call,
                                               int out_h, int out_w, const float* mean,
                                               const float* stdv, int channels_last, float* out,
                                               peclr_stream_t stream);

/* LEFT HANDS (TwoViewAugmenter / SupervisedAugmenter with is_left): the reference's loader turns a left hand into a right
 * one before augmentation (youtube_loader.py:151-155, cv2.flip(img, 1)).  Here the stage that reads the caller's images
 * reads the flagged samples mirrored -- column W - 1 - c for column c -- and everything else (warp coordinates and weights,
 * border tests, reflect-101 columns, the cut-out box, the blur taps) is in the mirrored image's coordinates: the sample
 * comes out as img[:, ::-1] would through the entry points above, bit for bit, and no flipped copy exists anywhere.
 *
 * mirror : device [B] ints, one per SAMPLE (not per view), non-zero = read mirrored.  Its own pointer: geom keeps its
 *          PECLR_AUG_GEOM_INT64S columns.  One batch mixes left and right hands in one launch per stage.
 * The mirror is applied ONCE, by the stage that reads the caller's images: a batch that runs stage 0 calls
 * peclr_augment_pre_*mirror_u8 and then the plain warp on the per-view sources (which hold the mirrored image already); a
 * batch without stage 0 calls peclr_augment_warp_crop_*mirror_u8.  Stage 2 never sees the caller's images.  The other
 * arguments are those of the entry point without `_mirror`, whose kernels are untouched. */
int peclr_augment_warp_crop_mirror_u8(const uint8_t* images, int B, int H, int W, int n_views,
                                      const double* params, const int* mirror, uint8_t* crops,
                                      peclr_stream_t stream);
int peclr_augment_pre_mirror_u8(const uint8_t* images, int B, int H, int W, int n_views,
                                const int* ext, const int* coefs, int kx, int ky, const int* mirror,
                                uint8_t* srcs, uint16_t* blur_tmp, peclr_stream_t stream);
int peclr_augment_pre_ragged_mirror_u8(const uint8_t* images, int B, int n_views, const int64_t* geom,
                                       int64_t total_bytes, int max_h, int max_w, const int* ext,
                                       const int* coefs, int max_kx, int max_ky, const int* mirror,
                                       uint8_t* srcs, uint16_t* blur_tmp, peclr_stream_t stream);
int peclr_augment_warp_crop_ragged_mirror_u8(const uint8_t* images, int B, int n_views,
                                             const int64_t* geom, const double* params,
                                             const int64_t* wins, int max_cw, int max_ch,
                                             const int* mirror, uint8_t* crops, peclr_stream_t stream);

/* The PARAMETER side on the device (TwoViewAugmenter(device_draws=True)), csrc/augment_draw.hip: ONE launch computes, for
 * every (view, sample) of the batch, what TwoViewAugmenter.sample_view computes on the host for the recipe flags (rotate, crop,
 * random_crop, resize, color_jitter): the uniforms, the angle, the rotation centre, the forward and inverse matrices, the
 * rotated joints, the crop window with margin and jitter, jitter_x / jitter_y and h / s / a / b -- in sample_view's own
 * arithmetic (float32 where it works on float32 tensors, float64 where it uses Python floats, no contraction).  The pixel
 * entry points above then run on the `params` it wrote, unchanged.  No host synchronisation; may be captured into a hipGraph.
 *
 * in   joints   : device [B][21][3], joints_dtype PECLR_DTYPE_F32 or PECLR_DTYPE_F64 (rounded to float32 first); x, y are read
 *      H, W     : the image size of every sample (geom == NULL), >= 1
 *      geom     : NULL, or the device [B][PECLR_AUG_GEOM_INT64S] table of a mixed-size batch; [1], [2] = H_i, W_i are read
 *      mirror   : NULL, or device [B] ints, non-zero = a left hand: its x is read as W - x in float32 before anything else
 *                 (the same table the `_mirror` pixel entry points take)
 *      flags    : PECLR_AUG_DRAW_* bits; RESIZE is required (PECLR_ERR_UNSUPPORTED without it, or with an unknown bit)
 *      ranges   : HOST pointer to PECLR_AUG_DRAW_RANGES doubles, passed to the kernel by value:
 *                   [0] [1]  angle: uniform([0], [1]) // 1 (max_angle, min_angle: the reference's swapped order)
 *                   [2] [3]  crop_margin_range        [4] crop_margin (random_crop off)
 *                   [5]      upper end of crop_box_jitter (both axes draw uniform(0, [5]))
 *                   [6] [7]  hue   [8] [9] saturation   [10] [11] value alpha   [12] [13] value beta
 *      seed     : the Philox4x32-10 key (low word, high word)
 *      call     : device uint64, the call counter: read by every workgroup, advanced by one by the last workgroup to finish.
 *                 Launches that share it must be ordered on one stream.
 *      counters : device int[2]: [0] += the number of SAMPLES of this launch with an EMPTY crop window in a view (cumulative;
 *                 the host path raises ValueError for such a sample, the kernel clamps the window to the 1 x 1 window at the
 *                 nearest pixel inside the image);
 *                 [1] the ticket counter, zero between launches
 * out  params   : [n_views][B][PECLR_AUG_PARAM_DOUBLES], the layout above
 *      scalars  : [n_views][PECLR_AUG_DRAW_SCALARS][B] doubles: angle, crop_margin_scale, h, s, a, b (an entry whose flag is
 *                 off holds its neutral value: 0, the fixed margin, 1, 1, 1, 0)
 *      jitter   : [n_views][2][B] int64: jitter_x, jitter_y
 *      uniforms : NULL, or [n_views][B][PECLR_AUG_DRAW_UNIFORMS] doubles, the raw uniforms in slot order angle, margin,
 *                 jitter x, jitter y, h, s, a, b
 * Random numbers: counter (sample i, 4 * view + k, call low word, call high word) for k = 0..3; call k gives slot 2k from the
 * output words (x, y) and slot 2k + 1 from (z, w): u = ((x >> 5) * 2^26 + (y >> 6)) / 2^53 (Python's random()), and
 * uniform(a, b) = a + (b - a) * u.  A slot whose flag is off is not used, so the draws of (view, sample) depend on nothing but
 * (seed, call, view, sample).  1 <= B <= 32767 and n_views 1 or 2, else PECLR_ERR_SHAPE; null pointers PECLR_ERR_NULL. */
#define PECLR_AUG_DRAW_ROTATE 1
#define PECLR_AUG_DRAW_CROP 2
#define PECLR_AUG_DRAW_RANDOM_CROP 4
#define PECLR_AUG_DRAW_RESIZE 8
#define PECLR_AUG_DRAW_COLOR_JITTER 16
#define PECLR_AUG_DRAW_ALL 31
#define PECLR_AUG_DRAW_RANGES 14
#define PECLR_AUG_DRAW_SCALARS 6
#define PECLR_AUG_DRAW_UNIFORMS 8
int peclr_augment_draw_views(const void* joints, int joints_dtype, int B, int n_views, int H, int W,
                             const int64_t* geom, const int* mirror, int flags, const double* ranges,
                             uint64_t seed, uint64_t* call, int* counters, double* params,
                             double* scalars, int64_t* jitter, double* uniforms,
                             peclr_stream_t stream);

/* ---- 16-bit convolutions of the residual blocks (bf16 / fp16 autocast: BASELINE configs C3 / C5 and the reference's own
 * `precision: 16`, training_config.json:9, peclr_training.py:78-79), csrc/conv_h.hip.  They replace MIOpen's 16-bit
 * convolution kernels behind torchvision's Bottleneck / BasicBlock (resnet_model.py:15) -- forward and input gradient of the
 * 1x1 and 3x3 convolutions, stride 1 and 2 -- with fp32 accumulation on v_mfma_f32_32x32x16_{bf16,f16} and the same fused
 * epilogues as the fp32 kernels above: BatchNorm statistics of the output, the backward reduction of the BatchNorm layer the
 * output gradient arrives at, the residual branch's gradient as a dense / compact stride-2 / 1-bit-masked addend.
 * dtype = PECLR_DTYPE_BF16 or PECLR_DTYPE_F16 for activations, gradients and packed weights alike.
 *   peclr_h_pack: the weight operand, packed ONCE per optimiser step from the fp32 master weights (this is also the cast
 *   autocast performs per forward): device table of `count` entries of 8 int64 {src fp32 matrix, dst, n, k, ld (floats),
 *   transposed (0 / 1 / T as peclr_x6_pack_f32), first chunk, dtype}; per (128 columns, 32 k) one 8 KiB chunk of eight
 *   1 KiB pieces [32-column block][16-k half] in MFMA fragment order; n % 64 == 0, k % 32 == 0; dst holds
 *   peclr_h_pack_bytes(n, k) = 2 * roundup(n, 128) * k bytes.
 *   peclr_gemm_h: C[M,N] = A[M,K] . B_t^T (+ addend): add_h = add_w = 0 dense addend [M][ldd]; add_h, add_w > 0 the addend
 *   holds every second pixel of add_h x add_w images (compact stride-2 shortcut gradient); addend_mask: 1-bit ReLU mask of a
 *   dense addend ([M][N / 32]).  stat_shift / stat_partial and bn_bwd as in peclr_gemm_x6p_f32 (bn_bwd->x points at 16-bit
 *   rows).  Sums are taken of the ROUNDED 16-bit outputs.  lda, ldc, ldd multiples of 8.
 *   peclr_conv_h: taps = 9 (3x3, padding 1) or 1, stride 1 or 2, NHWC; flip = 1 (taps = 9, stride 1): the input gradient
 *   (X = dY, planes packed with transposed = 9).  `zeros`: >= 64 bytes of zeros.  Cin % 32 == 0, Cout % 64 == 0.
 *   tile_rows: 128 or 256 output rows per workgroup, 0 = the library's choice.  3x3 / stride 1 with rows of <= 62 pixels:
 *   PECLR_CONV_H_RING (and the choice of 0) runs the ring form -- a workgroup owns 256 consecutive pixels of the PADDED space
 *   NB x (H + 1) x (W + 1) (one shared zero row / column per image, as peclr_wgrad3_h) and fetches the 256 + 2 (W + 2) input
 *   pixels its nine taps read once per 32-channel chunk instead of once per tap.  peclr_conv_h_row_blocks: the rows the
 *   partial-sum tables (stat_partial: 2 * rows + 1, bn_bwd->partial: 2 * rows) of such a launch have (0: unsupported).
 *   peclr_conv3x3_s2_dgrad_h: input gradient of the 3x3 / stride-2 convolution by parity classes (as the fp32 entry point). */
#define PECLR_CONV_H_RING 1
int64_t peclr_h_pack_bytes(int N, int K);
int peclr_h_pack(const void* desc_table, int count, int total_chunks, peclr_stream_t stream);
int peclr_conv_h_tile_rows(int M, int N);
int peclr_conv_h_row_blocks(int NB, int H, int W, int Cout, int taps, int stride, int tile_rows);
int peclr_gemm_h(int dtype, int M, int N, int K, const void* A, int lda, const void* Bp, void* C, int ldc, const void* addend,
                 int ldd, int add_h, int add_w, const unsigned* addend_mask, int tile_rows, const float* stat_shift,
                 float* stat_partial, const peclr_bn_bwd_fuse* bn_bwd, peclr_stream_t stream);
int peclr_conv_h(int dtype, int NB, int H, int W, int Cin, int Cout, int taps, int stride, const void* X, const void* Bp, void* Y,
                 int flip, int tile_rows, const void* zeros, const float* stat_shift, float* stat_partial,
                 const peclr_bn_bwd_fuse* bn_bwd, peclr_stream_t stream);
int peclr_conv3x3_s2_dgrad_h(int dtype, int NB, int Ho, int Wo, int Cout, int Cin, const void* dY, const void* Bp, void* dX,
                             int tile_rows, const void* zeros, const peclr_bn_bwd_fuse* bn_bwd, peclr_stream_t stream);
/* Prediction (eval mode): the BatchNorm2d (+ residual add) (+ ReLU) behind a convolution, folded into that convolution's
 * epilogue -- per output element, in fp32 on the accumulator,
 *     v = fmaf(acc, scale[col], shift[col]);  if (addend) v += addend;  if (relu) v = max(v, 0);  out = round_to_16_bit(v)
 * ONE rounding per layer (convolution -> peclr_bn2d_apply rounds the convolution's output and then the layer's), and no
 * apply pass over the activation.  scale_shift: that layer's fp32 [2][N] table (scale row, then shift row), 16-byte aligned,
 * as peclr_bn2d_eval_tables or an eval-mode peclr_bn2d_finalize_f32 writes it; NULL is PECLR_ERR_NULL.  The weights are NOT
 * rescaled: the planes peclr_h_pack makes serve unchanged.  ReLU drops a NaN as peclr_bn2d_apply's does (fmaxf).  Shapes,
 * alignment and tile_rows as peclr_gemm_h / peclr_conv_h (forward: no flip); the addend of peclr_gemm_h_bnact is dense
 * ([M][ldd], nullable); no statistics, no backward reduction. */
int peclr_gemm_h_bnact(int dtype, int M, int N, int K, const void* A, int lda, const void* Bp, void* C, int ldc, const void* addend,
                       int ldd, const float* scale_shift, int relu, int tile_rows, peclr_stream_t stream);
int peclr_conv_h_bnact(int dtype, int NB, int H, int W, int Cin, int Cout, int taps, int stride, const void* X, const void* Bp, void* Y,
                       int tile_rows, const void* zeros, const float* scale_shift, int relu, peclr_stream_t stream);
/* Weight gradient of a 16-bit 1x1 convolution (csrc/wgrad_h.hip): dW[Cout][Cin] (fp32) = dY^T X over the rows of two NHWC
 * activations -- A = dY [K][lda] (M = Cout), B = X [K][ldb] (N = Cin); stride = 2 (the 1x1 / stride-2 shortcut): A's K rows are
 * the Ho x Wo output pixels, B holds the 2 Ho x 2 Wo input pixels.  Both operands go global -> LDS by LDS-DMA as they lie in
 * memory and are transposed by the LDS read (ds_read_b64_tr_b16).  K is split over peclr_wgrad_h_slabs(M, N, K) workgroup rows,
 * each writing one fp32 slab [M][N]; peclr_slab_reduce_f32 adds them in a fixed order (deterministic; fp32 gradient of the fp32
 * master weight).  Replaces MIOpen's 16-bit weight gradients (zero-fill + atomic split-K + cast) under resnet_model.py:15.
 * M, N multiples of 32, lda / ldb multiples of 8; `zeros`: >= 64 bytes of zeros. */
/* ... and of the 16-bit 3x3 / padding-1 / stride-1 convolutions: dW[Cout][3][3][Cin] (the storage of a channels_last weight) from
 * dY [images, H, W, M = Cout] and X [images, H, W, N = Cin].  The contraction runs over a PADDED linear pixel space (one shared
 * zero column per row, one shared zero row per image, applied by the addresses the LDS-DMAs fetch), in which tap (a, b) is a
 * uniform shift: X goes through a ring in LDS once and serves all nine taps by transposing reads at the taps' offsets.
 * M, N multiples of 64, W <= 62; slabs [peclr_wgrad3_h_slabs(...)][M][9 N] fp32, summed by peclr_slab_reduce_f32. */
int peclr_wgrad3_h_slabs(int M, int N, int images, int H, int W);
int peclr_wgrad3_h(int dtype, int M, int N, int images, int H, int W, const void* A, const void* B, float* slabs, int n_slabs,
                   const void* zeros, peclr_stream_t stream);
/* ... and the same for rows of 63 <= W <= 512 pixels (narrower ones are refused here: PECLR_ERR_SHAPE / 0 slabs): every image is
 * cut into ceil(W / 61) column segments of near-equal width, each a pseudo-image of the padded space whose rows carry the
 * neighbouring segments' columns of X (zero outside the image) as halo slots, so the same ring holds two padded rows of any
 * width.  Same operands, slab layout and fixed-order reduction as peclr_wgrad3_h. */
int peclr_wgrad3w_h_slabs(int M, int N, int images, int H, int W);
int peclr_wgrad3w_h(int dtype, int M, int N, int images, int H, int W, const void* A, const void* B, float* slabs, int n_slabs,
                    const void* zeros, peclr_stream_t stream);
/* ... and of the 16-bit 3x3 / padding-1 / STRIDE-2 convolutions: dY [images, Ho, Wo, M = Cout], X [images, 2 Ho, 2 Wo, N = Cin]
 * (the OUTPUT size is passed).  X goes through LDS as its four parity planes, each in the padded space of dY's geometry, where
 * every tap is a uniform non-positive shift of one plane; one workgroup owns all nine taps of a 64 x 32 channel tile.
 * M, N multiples of 64, 1 <= Wo <= 62; same slab layout, error codes and fixed-order reduction as peclr_wgrad3_h. */
int peclr_wgrad3s2_h_slabs(int M, int N, int images, int Ho, int Wo);          /* 0: shape refused */
int peclr_wgrad3s2_h(int dtype, int M, int N, int images, int Ho, int Wo, const void* dY, const void* X, float* slabs, int n_slabs,
                     const void* zeros, peclr_stream_t stream);
int peclr_wgrad_h_slabs(int M, int N, int K);
int peclr_wgrad_h(int dtype, int M, int N, int K, const void* A, int lda, const void* B, int ldb, float* slabs, int n_slabs,
                  int stride, int Ho, int Wo, const void* zeros, peclr_stream_t stream);

/* The encoder's stem (csrc/stem.hip): y = conv2d(x, W, stride 2, padding 3) with W [64][3][7][7] -- torchvision ResNet `conv1`
 * behind /root/reference/src/models/resnet_model.py:15 -- for fp32 NHWC images x [N][Hin][Win][3] -> y [N][Ho][Wo][64] NHWC,
 * Ho = (Hin - 1) / 2 + 1.  fmt 0: fp32 output at fp32 accuracy (both operands split exactly into three bf16 numbers, six
 * products, fp32 accumulation, as peclr_gemm_x6p_f32); fmt 1 / 2: bf16 / fp16 output, one product of the operands rounded
 * to that format (what autocast computes; its cast of the images rides in the kernel's staging).  `planes`: the filter in
 * fragment order, peclr_stem_pack_bytes(fmt) bytes written by peclr_stem_pack from the fp32 master weight (element strides of
 * its four dimensions given: any memory format) -- once per optimiser step.  stat_shift / stat_partial (both or neither): the
 * training statistics of y for the BatchNorm that follows, in peclr_bn2d_stats' partial layout with n_split =
 * peclr_stem_workgroups(N, Hin, Win) row blocks: stat_partial [2 n_split + 1][64].  Replaces MIOpen's 7x7 forward (and,
 * with the statistics, the last peclr_bn2d_stats pass of the step). */
int peclr_stem_pack_bytes(int fmt);
int peclr_stem_pack(const float* w, long long stride_n, long long stride_c, long long stride_h, long long stride_w, void* planes,
                    int fmt, peclr_stream_t stream);
int peclr_stem_workgroups(int N, int Hin, int Win);
int peclr_stem_conv7x7_s2(const float* x, int N, int Hin, int Win, const void* planes, int fmt, void* y,
                          const float* stat_shift, float* stat_partial, peclr_stream_t stream);
/* ... and its weight gradient: dW[n][kh][kw][c] = sum over (image, oh, ow) of dY[oh][ow][n] . x[2 oh - 3 + kh][2 ow - 3 + kw][c], with the
 * output pixel as the contraction index of the matrix cores (dY transposed into LDS by 2-byte stores, the image patch
 * gathered by eight ds_read_u16 per fragment).  dY [N][Ho][Wo][64]: fp32 (fmt 0: six products, fp32 accuracy) or bf16 / fp16
 * (fmt 1 / 2: one product, the images rounded to that format as the forward rounds them).  Persistent workgroups each write
 * one fp32 slab [64][224] -- column 32 kh + 4 kw + c; the kw = 7 and c = 3 columns carry no meaning -- slabs
 * [peclr_stem_wgrad_slabs(N, Hin, Win, fmt)][64][224], summed in a fixed order by peclr_slab_reduce_f32 (deterministic, unlike
 * MIOpen's atomically accumulated weight gradient: the last MIOpen kernel of the fp32 step).                                */
int peclr_stem_wgrad_slabs(int N, int Hin, int Win, int fmt);
int peclr_stem_wgrad(const float* x, const void* dY, int N, int Hin, int Win, int fmt, float* slabs, int n_slabs,
                     peclr_stream_t stream);

/* The fine-tuned 2.5D hand-pose model at evaluation time (reference src/models/rn_25D_wMLPref.py and testing/pred_fh.py):
 * the crop and the head of the two-pass crop -> predict -> re-crop loop.  Host side: peclr_amd/pose.py.
 *
 * peclr_pose_crop_u8: fh_utils.preprocess for a batch.  images [B][H][W][3] u8 RGB, T [B][3][3] float64 forward matrices:
 *   out [B][S][S][3] float32 (the [B,3,S,S] channels_last tensor the stem reads) = table[c][warpAffine(img, T[:2], (S, S))],
 *   8-bit INTER_LINEAR with BORDER_CONSTANT 0 (the reference's borderValue saturates to 0 on u8).  table [3][256] float32:
 *   the normalisation of each channel value.  K [B][3][3] float64 (may be NULL): k_out [B][3][3] float32 = float32(T @ K).
 * peclr_pose_head_f32: pooled features feat [B][n_feat = 2048] -> the model's head, one launch.  fc_w [64][2048], fc_b [64];
 *   mlp: host array of PECLR_POSE_MLP_TENSORS device pointers -- zroot_ref.zroot_ref.{0.weight, 0.bias, 1.weight, 1.bias,
 *   1.running_mean, 1.running_var, 3.weight, 3.bias, 4.weight, 4.bias, 4.running_mean, 4.running_var, 6.weight, 6.bias};
 *   bn_eps1 / bn_eps2: the eps of the two BatchNorm1d.  K [B or 1][3][3] float32 (k_per_sample 0: one matrix broadcast).
 *   Out: out64 [B][64] (the fc output with the root's zrel zeroed: kp25d = out64[:, :63]), kp3d [B][21][3].
 *   Pass 1 (T1 != NULL): T2 [B][3][3] float64 = the re-crop matrix of pred() from kp2d and T1 [B][3][3], crop size S;
 *     status[b] = PECLR_POSE_STATUS_NO_BBOX (T2 NaN) when every x or every y of kp2d is NaN, else 0.
 *   Pass 2 (scale != NULL): fh [B][21][3] float64 = FreiHAND joints (palm -> wrist, joint order) times scale[b];
 *     PECLR_POSE_STATUS_NAN is OR-ed into status[b] when one is NaN, status[b] is left as it is otherwise.
 *   At most one of the two epilogues per launch; without either, status is not touched. */
#define PECLR_POSE_MLP_TENSORS 14
#define PECLR_POSE_STATUS_NO_BBOX 1
#define PECLR_POSE_STATUS_NAN 2
int peclr_pose_crop_u8(const uint8_t* images, int B, int H, int W, const double* T, const double* K, const float* table, int S,
                       float* out, float* k_out, peclr_stream_t stream);
int peclr_pose_head_f32(const float* feat, int B, int n_feat, const float* fc_w, const float* fc_b, const float* const* mlp,
                        float bn_eps1, float bn_eps2, const float* K, int k_per_sample, float eps, float* out64, float* kp3d,
                        const double* T1, double* T2, int S, const double* scale, double* fh, int* status,
                        peclr_stream_t stream);

/* The two ends of the same two-pass prediction for images of ANY size in one batch, with a left-hand flag per sample
 * (csrc/predict.hip; host side: peclr_amd/predict.py, HandPosePredictor).  One launch each, no atomics, no host synchronisation.
 *
 * peclr_pose_crop_ragged_u8: peclr_pose_crop_u8 for a packed batch.  packed: total_bytes of u8, the images back to back and
 *   unpadded (image starts need no alignment).  geom: DEVICE table [B][4] int64 = (byte offset of the image in packed, H, W,
 *   flip), read by the kernel -- a captured launch sees whatever the table holds at replay.  T, K, table, S, out, k_out as
 *   peclr_pose_crop_u8; sample b of out is, bit for bit, what that entry point writes for image b alone.  flip != 0: a tap at
 *   source column sx reads column W - 1 - sx, i.e. the crop of img[:, ::-1] (left hands are mirrored into right hands before
 *   the network sees them), and k_out = float32(T @ Kf) with Kf = F K M, the camera of the mirrored image looking at the mirrored
 *   scene, formed in float64 with one product and one difference per entry: r[c] = (W - 1) K[2][c] - K[0][c];
 *   Kf = [[-r[0], r[1], r[2]], [-K[1][0], K[1][1], K[1][2]], [-K[2][0], K[2][1], K[2][2]]].
 *   That offset + 3 H W <= total_bytes for every row is the caller's to guarantee; a row for which it does not hold (or with
 *   H < 1 or W < 1) is treated as an empty image -- every tap outside -- and nothing is read through it.
 * peclr_pose_unmap: after pass 2.  out64 [B][64] (the 2D keypoints of joint j at [3j], [3j + 1], crop pixels), T2 [B][3][3]
 *   float64, geom as above, kp3d_in [B][21][3] float32, fh [B][21][3] float64 (peclr_pose_head_f32's pass-2 outputs; none is
 *   written).  Out: kp2d_src [B][21][2] float64, the keypoints in SOURCE pixels: with mi = cv's invertAffineTransform(T2[:2]),
 *   u = mi[0] x + mi[1] y + mi[2], v = mi[3] x + mi[4] y + mi[5] (float64, left to right, no contraction), and
 *   u = (W - 1) - u for flip; kp3d [B][21][3] float32 and xyz [B][21][3] float64: copies of kp3d_in and fh, X negated for flip. */
int peclr_pose_crop_ragged_u8(const uint8_t* packed, int64_t total_bytes, int B, const int64_t* geom, const double* T,
                              const double* K, const float* table, int S, float* out, float* k_out, peclr_stream_t stream);
int peclr_pose_unmap(const float* out64, const double* T2, const int64_t* geom, const float* kp3d_in, const double* fh, int B,
                     double* kp2d_src, float* kp3d, double* xyz, peclr_stream_t stream);

/* The same head in train mode -- BatchNorm1d on batch statistics, running statistics updated on the device -- and its exact
 * backward (csrc/pose_train.hip; host side: peclr_amd/pose.py, PoseHeadTrain).  fp32 with the batch reductions of BatchNorm
 * in float64, every reduction in a fixed order, no
 * atomics, no host synchronisation; 2 <= B <= PECLR_POSE_TRAIN_MAX_BATCH, anything else is PECLR_ERR_SHAPE before a launch.
 * feat, fc_w, fc_b, mlp (here the running statistics are written), K, k_per_sample, eps, out64, kp3d as peclr_pose_head_f32.
 *
 * peclr_pose_head_train_fwd_f32 -- FOUR launches on `stream`: fc + geometry + the detached closed-form root depth per sample;
 *   Linear + BatchNorm + LeakyReLU twice, each workgroup owning 4 hidden units over all B rows; Linear(128, 1) + kp3d per sample.
 *   momentum1 / momentum2: running = (1 - momentum) running + momentum batch (the variance unbiased); nbt1 / nbt2: the two
 *   num_batches_tracked (int64, += 1).  Out: out64 [B][64], kp3d [B][21][3], zroot [B] (the refined root depth) and
 *   save [PECLR_POSE_TRAIN_SAVE_FLOATS(B)], 16-byte aligned, which the backward reads: x [B][64] (the MLP input), p1, h1, p2,
 *   h2 [B][128] each (the Linear outputs and the activations), per BatchNorm mean [128] and invstd [128] in float64 (the backward
 *   forms xhat from p without another rounding), ku [B][21][3] (kp3d_unnorm).
 * peclr_pose_head_train_bwd_f32 -- SIX launches (five when d_feat is NULL): dzroot per sample; the two column-owning blocks in
 *   reverse (LeakyReLU by the sign of its input, 0 on the slope side; BatchNorm train backward; dW, db, dgamma, dbeta); the
 *   geometry back to the fc output; dWfc / dbfc by slices of 64 columns over all rows; dfeat.  g_kp3d [B][21][3], g_out64 [B][64],
 *   g_zroot [B]: the upstream gradients, each may be NULL (zeros).  ws [PECLR_POSE_TRAIN_WS_FLOATS(B)], 16-byte aligned: dp2, dp1
 *   [B][128] (gradients at the two Linear outputs), do [B][64] (gradient at the fc output), dzroot [B].  Out: d_feat [B][2048]
 *   or NULL, d_fc_w [64][2048], d_fc_b [64], d_mlp: host array of PECLR_POSE_MLP_GRADS device pointers, the gradients of
 *   zroot_ref.zroot_ref.{0.weight, 0.bias, 1.weight, 1.bias, 3.weight, 3.bias, 4.weight, 4.bias, 6.weight, 6.bias} (the two
 *   biases in front of a BatchNorm get 0, which the sum of dp over the batch is exactly).  K gets no gradient.
 * peclr_pose_head_train_launches: the number of launches of the forward (backward = 0) or of the backward. */
#define PECLR_POSE_TRAIN_MAX_BATCH 1024
#define PECLR_POSE_MLP_GRADS 10
#define PECLR_POSE_TRAIN_SAVE_FLOATS(B) ((size_t)(B) * 639 + 1024)
#define PECLR_POSE_TRAIN_WS_FLOATS(B) ((size_t)(B) * 321)
int peclr_pose_head_train_fwd_f32(const float* feat, int B, int n_feat, const float* fc_w, const float* fc_b, float* const* mlp,
                                  float bn_eps1, float bn_eps2, float momentum1, float momentum2, int64_t* nbt1, int64_t* nbt2,
                                  const float* K, int k_per_sample, float eps, float* out64, float* kp3d, float* zroot, float* save,
                                  peclr_stream_t stream);
int peclr_pose_head_train_bwd_f32(const float* feat, int B, int n_feat, const float* fc_w, const float* const* mlp, const float* K,
                                  int k_per_sample, const float* out64, const float* zroot, const float* save, const float* g_kp3d,
                                  const float* g_out64, const float* g_zroot, float* ws, float* d_feat, float* d_fc_w, float* d_fc_b,
                                  float* const* d_mlp, peclr_stream_t stream);
int peclr_pose_head_train_launches(int backward, int want_d_feat);

/* Scoring pose predictions (reference src/experiments/evaluation_utils.py: calculate_epe_statistics, calc_procrustes_transform,
 * get_pck_curves), csrc/pose_eval.hip; host side: peclr_amd/pose_eval.py.  One launch for a batch.
 *
 * peclr_pose_eval: pred, gt [B][21][3], both of `dtype` (PECLR_DTYPE_F32 or PECLR_DTYPE_F64; so is every floating-point
 *   output and thr).  dim = 3, or 2: only x and y enter the distance and the five Procrustes outputs must be NULL.
 *   dist [B][21]: the Euclidean distance per joint, float64 arithmetic, rounded once.
 *   Procrustes alignment of pred onto gt (calc_procrustes_transform(X = gt, Y = pred)), run when at least one of its outputs
 *   is given, each of them nullable: aligned [B][21][3] (y_transform), rot [B][3][3], scale [B], trans [B][3],
 *   dist_aligned [B][21] = the distance of the ROUNDED aligned cloud to gt.  float64 arithmetic whatever the dtype (one-sided
 *   Jacobi SVD of the 3 x 3 covariance, reflection fix on the last singular pair), one rounding on output.
 *   PCK: thr [n_thr] thresholds, counts [2][21][n_thr] 64-bit integers that are ADDED to: counts[0][j][k] += #{b : dist[b][j] <
 *   thr[k]}, counts[1] the same for dist_aligned (only when the alignment runs); the comparison is made in `dtype` on the
 *   values written out, NaN is never under a threshold.  n_thr = 0: no counting (thr, counts may be NULL).
 *   status [B] int32, OR-ed into: PECLR_POSE_STATUS_NAN when a coordinate that enters the distance is NaN,
 *   PECLR_POSE_EVAL_DEGENERATE when the alignment runs and the centred norm of gt or pred is 0 or not finite -- the sample's
 *   Procrustes outputs are then NaN (the reference's 0 / 0), no other sample is touched.
 *   Streaming (cursor != NULL): cursor is a DEVICE int[2] = {rows filled so far, 0}; dist, dist_aligned and status are
 *   buffers of `capacity` rows and sample b goes to row cursor[0] + b; the launch itself advances cursor[0] by B when its
 *   last workgroup finishes, so a hipGraph that captured the launch fills consecutive rows on every replay.  A launch whose
 *   rows would not fit writes nothing (no counts either) and still advances: the host finds cursor[0] > capacity.
 *   aligned / rot / scale / trans are per-launch outputs and never offset.  Every launch that shares a cursor must be
 *   ordered on ONE stream (or one captured graph): two such launches in flight at once would read the same cursor[0] and
 *   draw tickets from the same counter.
 *   A sample's outputs are a pure function of that sample: the same bits alone, at any position of any batch, run to run.
 *   Every argument error is reported as -1 before any launch: B <= 0, NULL pred / gt / dist / status, unknown dtype, dim not
 *   2 or 3, dim = 2 with a Procrustes output, n_thr < 0, n_thr > 2^20, n_thr > 0 with NULL thr or counts, cursor with
 *   capacity <= 0 or B > capacity.                                                                                     */
#define PECLR_DTYPE_F64 3
#define PECLR_POSE_EVAL_DEGENERATE 4
int peclr_pose_eval(const void* pred, const void* gt, int B, int dtype, int dim, void* dist, void* aligned, void* rot, void* scale,
                    void* trans, void* dist_aligned, const void* thr, int n_thr, long long* counts, int* status, int* cursor,
                    int capacity, peclr_stream_t stream);

/* The label side of a supervised sample (reference src/data_loader/utils.py: convert_to_2_5D, convert_2_5D_to_3D, get_root_depth,
 * get_zroot_constraint_terms; data_set.py: prepare_supervised_sample), csrc/labels.hip; host side: peclr_amd/supervised.py.
 * Every tensor is float32 and contiguous except T (float64).  Each entry point is ONE launch on `stream`: no host
 * synchronisation, no atomics, nothing kept between launches -- safe inside a hipGraph capture.  Every stage is evaluated in
 * float64 and each output is rounded to float32 once; a sample's outputs are a pure function of that sample (the same bits
 * alone and at any position of any batch).  Argument errors (B <= 0, a NULL pointer that is not marked nullable) are -1.
 *
 * peclr_joints3d_to_25d: K [B][3][3], joints3d [B][21][3] -> joints25d [B][21][3] = ((K p) / z in x and y, (z - z_wrist) /
 *   scale), scale [B] = |joint 2 - joint 0| (wrist -- index MCP).
 * peclr_joints25d_to_3d: joints25d, scale, K -> joints3d [B][21][3] = (K^-1 (u, v, 1)) (z + z_root) scale, with K^-1 the
 *   adjugate over the determinant and z_root [B] (nullable output) the root of the quadratic of arXiv:1804.09534 eq. 6-7,
 *   with the reference's two clamp(min = 1e-6) (discriminant, leading coefficient).  z_root_calc [B] (nullable): used as the
 *   root depth of the conversion instead; z_root still receives the quadratic's.
 * peclr_supervised_labels: K, joints3d, T [B][3][3] float64 (the augmentation's forward matrix), joints_raw [B][21][3]
 *   (nullable: joints3d then) ->
 *     t_out = fl32(T);  k_out = fl32(T) @ K;
 *     use_palm = 0: joints = T applied to (u, v, 1) of joints3d_to_25d(K, joints3d), depth kept; scale of joints3d;
 *                   joints3d_out = joints3d; joints_raw_out = joints_raw;
 *     use_palm = 1: joints3d_out / joints_raw_out = the input with joint 0 replaced by the mean of joints 0 and 2;
 *                   joints, scale = joints3d_to_25d(k_out, joints3d_out);
 *     joints3d_recreated = joints25d_to_3d(joints, scale, k_out), read as the float32 values written out.           */
int peclr_joints3d_to_25d(const float* K, const float* joints3d, int B, float* joints25d, float* scale, peclr_stream_t stream);
int peclr_joints25d_to_3d(const float* joints25d, const float* scale, const float* K, const float* z_root_calc, int B,
                          float* joints3d, float* z_root, peclr_stream_t stream);
int peclr_supervised_labels(const float* K, const float* joints3d, const double* T, const float* joints_raw, int B, int use_palm,
                            float* joints, float* k_out, float* scale, float* joints3d_out, float* joints3d_recreated,
                            float* joints_raw_out, float* t_out, peclr_stream_t stream);
/* peclr_supervised_labels_mirror: peclr_supervised_labels with mirror_w [B] ints per sample: 0 = the sample as stored,
 *   W > 0 = the LEFT hand of an image of width W, labelled as the right hand of img[:, ::-1].  For such a sample, before
 *   anything else: K <- fl32(Kf), Kf = F K M the camera of the mirrored image looking at the mirrored scene (the predictor's
 *   rule, csrc/predict.hip: row 0 <- (W - 1) row 2 - row 0, then column 0 negated; float64 from the float32 K, the product
 *   being exact, and ONE rounding), and joints3d / joints_raw get X negated.  From there it is peclr_supervised_labels (one
 *   shared kernel body) on those values; a sample with 0 comes out as from peclr_supervised_labels. */
int peclr_supervised_labels_mirror(const float* K, const float* joints3d, const double* T, const float* joints_raw,
                                   const int* mirror_w, int B, int use_palm, float* joints, float* k_out, float* scale,
                                   float* joints3d_out, float* joints3d_recreated, float* joints_raw_out, float* t_out,
                                   peclr_stream_t stream);

/* The supervised losses of the 2.5D pose model with their gradients (reference src/models/utils.py: cal_l1_loss, cal_3d_loss,
 * through convert_2_5D_to_3D / get_root_depth), csrc/pose_loss.hip; host side: peclr_amd/pose_loss.py.  Inputs and emitted
 * losses / gradients are float32 and contiguous; the workspaces between forward and backward are float64.  No host
 * synchronisation, no atomics, nothing kept in the library between calls -- safe inside a hipGraph capture.  Everything is
 * evaluated in float64 and each float32 output is rounded once; sums run in a fixed order (a butterfly over a wave per sample,
 * then one workgroup over the samples), so the result depends on nothing but the inputs.  Argument errors (B <= 0, a NULL
 * pointer that is not marked nullable) are -1.
 *
 * peclr_pose_loss -- TWO launches on `stream` (per-sample partial sums and gradients; the fold):
 *   in   pred [B][21][3]        the 2.5D prediction (u, v, root-relative scale-normalised depth)
 *        joints [B][21][3]      the true 2.5D joints;  joints3d [B][21][3] the true 3D joints
 *        scale [B], K [B][3][3] bone scale and camera matrix of the sample
 *                               (one of joints / joints3d may be NULL, K with joints3d: the three L1 losses, or the 3D loss, are
 *                               then left out -- nothing is read for them, their losses and gradients are 0)
 *        joints_valid [B][21]   (nullable: ones) weight of a joint, 0 / 1 in the reference
 *        z_root_calc [B]        (nullable) a root depth to lift with instead of the closed form of pred's joints 0 and 2
 *   out  losses [4]             loss_2d   = sum valid (|du| + |dv|) / (2 sum valid)
 *                               loss_z    = sum valid |dz| / sum valid
 *                               loss_z_unscaled = sum scale[b] valid |dz| / sum valid
 *                               loss_3d   = sum valid |joints25d_to_3d(pred, scale, K, z_root_calc) - joints3d|_1 / (3 sum valid)
 *                               (sum valid = 0: NaN, the reference's 0 / 0)
 *        inv_valid [1] float64  1 / sum valid
 *   workspaces, float64, read by peclr_pose_loss_bwd:
 *        partials [B][5]        per sample: sum valid, sum valid |d uv|, sum valid |dz|, scale x the third, sum valid |d 3D|
 *        g_l1 [B][21][3]        valid x sign(pred - joints), sign(0) = 0
 *        g_3d [B][21][3]        d (sum valid |d 3D|) / d pred: through the lift of the joint itself and, without z_root_calc,
 *                               through the root depth of joints 0 and 2.  torch.clamp's backward at both clamp(min = 1e-6):
 *                               no gradient through a clamped leading coefficient or discriminant (a value AT the minimum
 *                               passes it), while -b / (2 clamp(a)) keeps its gradient with respect to b
 *        g_zroot [B]            (nullable; written only with z_root_calc) d (sum valid |d 3D|) / d z_root_calc
 * peclr_pose_loss_bwd -- ONE launch:
 *   in   grad_losses [4]        upstream gradients of the four losses, on the device
 *        g_l1, g_3d, g_zroot (nullable unless grad_z_root_calc is given), scale, inv_valid: as above
 *   out  grad_pred [B][21][3]   = (grad_losses[0] / 2 on u, v; grad_losses[1] + grad_losses[2] scale[b] on z) g_l1 / sum valid
 *                                 + grad_losses[3] / 3 g_3d / sum valid
 *        grad_z_root_calc [B]   (nullable) = grad_losses[3] / 3 g_zroot / sum valid                                          */
int peclr_pose_loss(const float* pred, const float* joints, const float* joints3d, const float* scale, const float* K,
                    const float* joints_valid, const float* z_root_calc, int B, double* partials, double* g_l1, double* g_3d,
                    double* g_zroot, float* losses, double* inv_valid, peclr_stream_t stream);
int peclr_pose_loss_bwd(const float* grad_losses, const double* g_l1, const double* g_3d, const double* g_zroot, const float* scale,
                        const double* inv_valid, int B, float* grad_pred, float* grad_z_root_calc, peclr_stream_t stream);

/* ---- the metrics of a supervised step (reference src/models/utils.py: calculate_metrics), csrc/pose_metrics.hip; host side:
 * peclr_amd/pose_metrics.py.  ONE launch on `stream`, one workgroup per pair; no atomics, no host synchronisation, nothing kept
 * in the library between calls -- safe inside a hipGraph capture, and the same bits on every run.
 *   in   pred, truth [B][21][3]    float32, contiguous; 1 <= B <= PECLR_POSE_METRICS_MAX_BATCH (else PECLR_ERR_SHAPE)
 *        pred2, truth2 [B][21][3]  (nullable, both or neither) a second pair, e.g. the 3D joints next to the 2.5D ones
 *        workspace                 at least 2 x 21 x B x 4 bytes (half of it without the second pair): the distances' bit patterns
 *   out  out [4] float32           {mean, median} of the first pair, then of the second (out[2], out[3] are not written without it).
 *                                  The distances |pred - truth|_2 of all n = 21 B joints are float64 from the float32 inputs; the
 *                                  mean is their fixed-order float64 sum / n, rounded once; the median is torch.median's LOWER
 *                                  median -- element (n - 1) / 2 of the ascending float32-rounded distances, found by an exact radix
 *                                  select over their bit patterns (rounding is monotone: it equals the rounded float64 median).
 *                                  A NaN distance makes both values of its pair NaN; +inf orders last; pred == truth gives +0.   */
#define PECLR_POSE_METRICS_MAX_BATCH 1024
int peclr_pose_step_metrics_f32(const float* pred, const float* truth, const float* pred2, const float* truth2, int B,
                                void* workspace, float* out, peclr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PECLR_HIP_H */
