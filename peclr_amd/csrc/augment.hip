// Two-view augmentation on the device: the pixel side of
// SampleAugmenter.transform_sample (reference src/data_loader/sample_augmenter.py:47-129) for the
// published recipe -- rotate (cv2.warpAffine), crop, resize (cv2.resize INTER_AREA), colour jitter
// (cv2 BGR<->HSV) -- followed by ToTensor + Normalize (src/data_loader/utils.py:283-293).
//
// The reference runs this per sample on CPU workers; here a whole batch and both views are two
// launches.  8-bit intermediate images are kept between the stages exactly where the reference has
// them (after the rotation, after the resize, around the HSV round trip), so the arithmetic is the
// integer / float32 arithmetic of oracle/augment_oracle.py and the outputs are bit-identical to it.
//
//   warp_crop_kernel          source images [B][H][W][3] u8 -> the crop window of the rotated image,
//                             [V][B][H][W][3] u8 scratch (only the window is written)
//   resize_color_norm_kernel  crop window -> out_h x out_w (area / integer-box / area-mode bilinear,
//                             chosen per sample like cv::resize does) -> HSV jitter -> normalised
//                             float32, NCHW or NHWC
//
// The reference's other five augmentations (TwoViewAugmenter(extended=True)) add, only for batches that
// draw them:
//   pre_rows_kernel    stage 0: source -> Sobel (low byte of dx + dy) -> cut-out -> [horizontal pass of
//                      the 8-bit fixed-point Gaussian blur into a 16-bit scratch], per-view sources
//                      [V][B][H][W][3] u8; samples without a pre-op are copied unchanged
//   pre_cols_kernel    stage 0: vertical blur pass of the blurred samples, 16-bit scratch -> u8
//   resize_color_norm_kernel<., true>  stage 2 plus Gaussian noise (Philox4x32-10, integer CDF table,
//                      uint8 wrap-around add) and colour drop (BGR2GRAY to all three channels)
// warp_crop_kernel then reads the per-view sources, one launch per view.
//
// Every kernel is written once over a GEOMETRY SOURCE (template parameters SRC / WIN below): the uniform one restates
// the [B][H][W][3] batch of the first four entry points, the ragged one reads per-sample offsets and sizes from device
// tables, so that one batch may mix image sizes (the *_ragged entry points; include/peclr_hip.h has the tables).  Ragged
// grids are sized by the batch maximum; a block outside its own sample's extent leaves before any barrier.  The ragged
// crop scratch is PACKED: the host knows every window before the launch, so window (view, sample) sits at its own byte
// offset with its own width as row stride, and the scratch is the sum of the windows instead of V*B*H*W*3.
//
// LEFT HANDS (the *_mirror entry points): either source wrapped in `Mirrored<>` carries a per-sample table, and the stage that
// reads the caller's images -- pre_rows_kernel when stage 0 runs, warp_crop_kernel otherwise, never both -- reads a flagged
// sample's columns in reverse: the sample is processed exactly as img[:, ::-1] would be (what the reference's YouTube loader
// feeds its augmenter for a left hand), in the same launch as its right-handed neighbours and without a flipped copy.
//
// Work per batch is tiny (B=128: ~40 MB read, ~50 MB written): these kernels exist to take the
// cv2-on-CPU producer off the critical path, not to approach a roofline.  One thread per pixel,
// consecutive lanes = consecutive x, so the float32 NHWC / NCHW stores coalesce.
#include "common.hpp"
#include "warp_u8.hpp"

#pragma clang fp contract(off)  // products and sums round separately, as in the scalar restatement

namespace peclr {
namespace {

constexpr int NP = PECLR_AUG_PARAM_DOUBLES;
constexpr int BX = 64, BY = 4;

struct ViewParam {
    double minv[6];
    bool rotate;
    int x0, y0, cw, ch;
    bool color;
    double h, s, a, b;
};

__device__ __forceinline__ ViewParam load_param(const double* __restrict__ params, int n) {
    const double* p = params + (size_t)n * NP;
    ViewParam v;
#pragma unroll
    for (int i = 0; i < 6; ++i) v.minv[i] = p[i];
    v.rotate = p[6] != 0.0;
    v.x0 = (int)p[7], v.y0 = (int)p[8], v.cw = (int)p[9], v.ch = (int)p[10];
    v.color = p[11] != 0.0;
    v.h = p[12], v.s = p[13], v.a = p[14], v.b = p[15];
    return v;
}

__device__ __forceinline__ long long round_ll(double x) { return (long long)rint(x); }  // half to even

// ---- extension record (include/peclr_hip.h PECLR_AUG_EXT_INTS)
constexpr int NE = PECLR_AUG_EXT_INTS;
constexpr int PRE_RMAX = (PECLR_AUG_MAX_BLUR_KSIZE - 1) / 2;

struct ExtParam {
    int flags;
    int r0, r1, c0, c1;  // cut-out rows [r0, r1), columns [c0, c1)
    int fill;
    int coef;            // offset of this view's horizontal then vertical Q8 blur taps
};

__device__ __forceinline__ ExtParam load_ext(const int* __restrict__ ext, int n) {
    const int* p = ext + (size_t)n * NE;
    return ExtParam{p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
}

// cv::borderInterpolate(BORDER_REFLECT_101) for any offset
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * n - 2;
    i = abs(i) % period;
    return i < n ? i : period - i;
}

// cvtColor(COLOR_BGR2GRAY) on 8-bit data: channel 0 is taken as blue, 14-bit fixed point
__device__ __forceinline__ int gray_u8(int c0, int c1, int c2) { return (1868 * c0 + 9617 * c1 + 4899 * c2 + 8192) >> 14; }

__device__ __forceinline__ int gray_at(const uint8_t* __restrict__ src, int W, int y, int x) {
    const uint8_t* s = src + ((size_t)y * W + x) * 3;
    return gray_u8(s[0], s[1], s[2]);
}

// ---- geometry sources
struct SrcGeom {
    size_t off;  // byte offset of the sample's image in `images`
    int H, W, kx, ky;
};
struct WinGeom {
    size_t off, stride;  // crop window in the scratch: byte offset of its first pixel, bytes per row
};

// image(n): the source image of (view, sample) n = view * B + sample; view_off(n, g): the element offset of n's copy in
// the per-view buffers `srcs` / `blur_tmp`; kRagged: grids are the batch maximum's, so blocks test their own extent.
struct UniformSrc {
    static constexpr bool kRagged = false, kMirror = false;
    int B, H, W, kx, ky;
    __device__ __forceinline__ SrcGeom image(int n) const { return SrcGeom{(size_t)(n % B) * H * W * 3, H, W, kx, ky}; }
    __device__ __forceinline__ size_t view_off(int n, const SrcGeom&) const { return (size_t)n * H * W * 3; }
};
struct UniformWin {  // the window of (view, sample) n at the origin of its own H x W image, rows at the source stride
    int H, W;
    __device__ __forceinline__ WinGeom window(int n) const { return WinGeom{(size_t)n * H * W * 3, (size_t)W * 3}; }
};

constexpr int NG = PECLR_AUG_GEOM_INT64S, NW = PECLR_AUG_WIN_INT64S;
struct RaggedSrc {
    int B;
    const long long* __restrict__ geom;  // [B][NG]
    size_t total;                        // bytes of the packed source = elements of one view of srcs / blur_tmp
    static constexpr bool kRagged = true, kMirror = false;
    __device__ __forceinline__ SrcGeom image(int n) const {
        const long long* g = geom + (size_t)(n % B) * NG;
        // (the lengths are bounded on the host; the clamp only keeps a bad table inside the LDS arrays)
        return SrcGeom{(size_t)g[0], (int)g[1], (int)g[2], min((int)g[3], PECLR_AUG_MAX_BLUR_KSIZE),
                       min((int)g[4], PECLR_AUG_MAX_BLUR_KSIZE)};
    }
    __device__ __forceinline__ size_t view_off(int n, const SrcGeom& g) const { return (size_t)(n / B) * total + g.off; }
};
// A source with LEFT HANDS: `mirror` (one int per SAMPLE, non-zero = a left hand) says whose image the stage reads mirrored,
// column W - 1 - c for column c.  The stage then works on img[:, ::-1] -- warp coordinates and weights, border tests, the
// reflect-101 columns, the cut-out box, the blur taps and the stores are all in the mirrored image's coordinates -- without a
// flipped copy.  The flag is uniform over a block.  A plain source (kMirror false) compiles to the code of before.
template <class SRC>
struct Mirrored : SRC {
    const int* __restrict__ mirror;  // [B]
    static constexpr bool kMirror = true;
    __device__ __forceinline__ bool left(int n) const { return mirror[n % SRC::B] != 0; }
};
template <class SRC>
__device__ __forceinline__ bool reads_mirrored(const SRC& geo, int n) {
    if constexpr (SRC::kMirror)
        return geo.left(n);
    else
        return false;
}

struct RaggedWin {
    const long long* __restrict__ wins;  // [V][B][NW]
    __device__ __forceinline__ WinGeom window(int n) const {
        const long long* w = wins + (size_t)n * NW;
        return WinGeom{(size_t)w[0], (size_t)w[1] * 3};
    }
};

constexpr int SEG = BX + 2 * PRE_RMAX;  // row positions a block of pre_rows_kernel covers, halo included
constexpr int COL_ROWS = 8;               // output rows per thread of pre_cols_kernel (sliding window)

// pixel after Sobel and cut-out at image (y, c), packed c0 | c1 << 8 | c2 << 16.  gt: the block's gray tile
// (rows y-1 .. y+1 at gt[0..2], image column c at gt[.][gi + 1]).  cs: the column of `src` that holds image column c
// (c itself, or W - 1 - c when the image is the caller's read mirrored).
__device__ __forceinline__ uint32_t pre_packed(const uint8_t* __restrict__ src, int W, int y, int c, int cs, const ExtParam& e,
                                               const uint8_t (*gt)[SEG + 2], int gi) {
    int v0, v1, v2;
    if (e.flags & PECLR_AUG_EXT_SOBEL) {
        // 3x3 Sobel dx + dy of the gray image (BORDER_REFLECT_101), stored as its low byte
        const int g00 = gt[0][gi], g01 = gt[0][gi + 1], g02 = gt[0][gi + 2];
        const int g10 = gt[1][gi], g12 = gt[1][gi + 2];
        const int g20 = gt[2][gi], g21 = gt[2][gi + 1], g22 = gt[2][gi + 2];
        const int sx = (g02 - g00) + 2 * (g12 - g10) + (g22 - g20);
        const int sy = (g20 + 2 * g21 + g22) - (g00 + 2 * g01 + g02);
        v0 = v1 = v2 = (sx + sy) & 255;
    } else {
        const uint8_t* s = src + ((size_t)y * W + cs) * 3;
        v0 = s[0], v1 = s[1], v2 = s[2];
    }
    if ((e.flags & PECLR_AUG_EXT_CUT_OUT) && y >= e.r0 && y < e.r1 && c >= e.c0 && c < e.c1) v0 = v1 = v2 = e.fill;
    return (uint32_t)v0 | ((uint32_t)v1 << 8) | ((uint32_t)v2 << 16);
}

// ---- stage 0, rows: Sobel -> cut-out -> [horizontal blur pass (u8 x Q8, exact in 16 bits)]
// A block covers BX columns x BY rows.  Row positions x in [x0 - rx, min(x0 + BX, W) + rx) are evaluated at
// their reflect-101 image column, which always lies in [lo, hi); the gray tile covers [lo - 1, hi + 1).
template <class SRC>
__global__ __launch_bounds__(BX* BY) void pre_rows_kernel(const uint8_t* __restrict__ images, SRC geo,
                                                           const int* __restrict__ ext, const int* __restrict__ coefs,
                                                           uint8_t* __restrict__ srcs, uint16_t* __restrict__ tmp) {
    __shared__ uint8_t gray[BY + 2][SEG + 2];
    __shared__ uint32_t seg[BY][SEG];
    __shared__ int taps[2 * PRE_RMAX + 1];
    const int n = blockIdx.z;  // view * B + sample
    const ExtParam e = load_ext(ext, n);
    const SrcGeom g = geo.image(n);
    const int H = g.H, W = g.W, kx = g.kx;
    const int x0 = blockIdx.x * BX, y0 = blockIdx.y * BY, tid = threadIdx.y * BX + threadIdx.x;
    if (SRC::kRagged && (x0 >= W || y0 >= H)) return;  // block-uniform, before any barrier
    const uint8_t* src = images + g.off;
    const bool left = reads_mirrored(geo, n);  // block-uniform
    const size_t view = geo.view_off(n, g);  // this (view, sample) in srcs / tmp
    const bool blur = (e.flags & PECLR_AUG_EXT_BLUR) && tmp;  // block-uniform
    const int rx = blur ? kx >> 1 : 0;
    const int lo = max(x0 - rx, 0), hi = min(x0 + BX + rx, W);
    if (blur)
        for (int i = tid; i < kx; i += BX * BY) taps[i] = coefs[e.coef + i];
    if (e.flags & PECLR_AUG_EXT_SOBEL) {
        const int gw = hi - lo + 2;
        for (int i = tid; i < (BY + 2) * gw; i += BX * BY) {
            const int j = i / gw, c = i - j * gw;
            const int gy = reflect101(y0 - 1 + j, H), gc = reflect101(lo - 1 + c, W);
            gray[j][c] = (uint8_t)gray_at(src, W, gy, left ? W - 1 - gc : gc);
        }
        __syncthreads();
    }
    const int y = y0 + threadIdx.y;
    const int npos = min(BX, W - x0) + 2 * rx;
    if (y < H) {
        for (int i = threadIdx.x; i < npos; i += BX) {
            const int c = reflect101(x0 - rx + i, W);
            const int gi = min(max(c - lo, 0), hi - lo - 1);  // == c - lo (see above); the clamp only bounds LDS
            seg[threadIdx.y][i] = pre_packed(src, W, y, c, left ? W - 1 - c : c, e,
                                             (const uint8_t(*)[SEG + 2])gray[threadIdx.y], gi);
        }
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W || y >= H) return;
    if (!blur) {
        const uint32_t p = seg[threadIdx.y][threadIdx.x];
        uint8_t* d = srcs + view + ((size_t)y * W + x) * 3;
        d[0] = (uint8_t)p, d[1] = (uint8_t)(p >> 8), d[2] = (uint8_t)(p >> 16);
        return;
    }
    // channels 0 and 2 share one 32-bit accumulator: each sum is at most 255 * 256 < 2^16
    uint32_t a02 = 0u, a1 = 0u;
    for (int k = 0; k < kx; ++k) {
        const uint32_t t = (uint32_t)taps[k], p = seg[threadIdx.y][threadIdx.x + k];
        a02 += t * (p & 0x00FF00FFu);
        a1 += t * ((p >> 8) & 0xFFu);
    }
    uint16_t* d = tmp + view + ((size_t)y * W + x) * 3;
    d[0] = (uint16_t)a02, d[1] = (uint16_t)a1, d[2] = (uint16_t)(a02 >> 16);
}

// ---- stage 0, columns: vertical blur pass (16-bit x Q8, (acc + 2^15) >> 16) of the blurred samples.
// Each thread produces COL_ROWS consecutive rows from one pass over the COL_ROWS + ky - 1 input rows.
template <class SRC>
__global__ __launch_bounds__(BX* BY) void pre_cols_kernel(SRC geo, const int* __restrict__ ext,
                                                           const int* __restrict__ coefs,
                                                           const uint16_t* __restrict__ tmp, uint8_t* __restrict__ srcs) {
    __shared__ int taps[2 * PRE_RMAX + 1];
    const int n = blockIdx.z;
    const ExtParam e = load_ext(ext, n);
    if (!(e.flags & PECLR_AUG_EXT_BLUR)) return;  // block-uniform; pre_rows_kernel wrote this sample already
    const SrcGeom g = geo.image(n);
    const int H = g.H, W = g.W, kx = g.kx, ky = g.ky;
    if (SRC::kRagged && (blockIdx.x * BX >= W || blockIdx.y * (BY * COL_ROWS) >= H)) return;  // as in pre_rows_kernel
    const size_t view = geo.view_off(n, g);
    for (int i = threadIdx.y * BX + threadIdx.x; i < ky; i += BX * BY) taps[i] = coefs[e.coef + kx + i];
    __syncthreads();
    const int x = blockIdx.x * BX + threadIdx.x, y0 = (blockIdx.y * BY + threadIdx.y) * COL_ROWS;
    if (x >= W || y0 >= H) return;
    const int ry = ky >> 1;
    const uint16_t* t = tmp + view + (size_t)x * 3;
    uint32_t acc[COL_ROWS][3] = {};
    for (int r = 0; r < COL_ROWS + ky - 1; ++r) {
        const uint16_t* s = t + (size_t)reflect101(y0 - ry + r, H) * W * 3;
        const uint32_t v0 = s[0], v1 = s[1], v2 = s[2];
#pragma unroll
        for (int j = 0; j < COL_ROWS; ++j) {
            const int k = r - j;
            if (k >= 0 && k < ky) {
                const uint32_t c = (uint32_t)taps[k];
                acc[j][0] += c * v0, acc[j][1] += c * v1, acc[j][2] += c * v2;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < COL_ROWS; ++j) {
        if (y0 + j >= H) break;
        uint8_t* d = srcs + view + ((size_t)(y0 + j) * W + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = (uint8_t)((acc[j][c] + (1u << 15)) >> 16);
    }
}

// ---- stage 1: rotation (8-bit warpAffine, bilinear, zero border), evaluated on the crop window only
// (After stage 0 the per-view sources ARE the mirrored images of the left samples: that warp runs on a plain source.)
template <class SRC, class WIN>
__global__ __launch_bounds__(BX* BY) void warp_crop_kernel(const uint8_t* __restrict__ images, SRC geo, WIN win,
                                                            const double* __restrict__ params,
                                                            uint8_t* __restrict__ crops) {
    const int n = blockIdx.z;  // view * B + sample
    const ViewParam v = load_param(params, n);
    const int cx = blockIdx.x * BX + threadIdx.x, cy = blockIdx.y * BY + threadIdx.y;
    if (cx >= v.cw || cy >= v.ch) return;
    const SrcGeom g = geo.image(n);
    const WinGeom wg = win.window(n);
    const int H = g.H, W = g.W;
    const uint8_t* src = images + g.off;
    uint8_t* dst = crops + wg.off + (size_t)cy * wg.stride + (size_t)cx * 3;
    const int x = v.x0 + cx, y = v.y0 + cy;
    const bool left = reads_mirrored(geo, n);  // block-uniform
    if (!v.rotate) {
        const uint8_t* s = src + ((size_t)y * W + (left ? W - 1 - x : x)) * 3;
        dst[0] = s[0], dst[1] = s[1], dst[2] = s[2];
        return;
    }
    // 10-bit fixed-point source coordinates, rounded to 1/32 pixel (warp_u8.hpp)
    int px[3];
    if (left)
        warp_bilinear_u8<true>(src, H, W, v.minv, x, y, px);
    else
        warp_bilinear_u8(src, H, W, v.minv, x, y, px);
    dst[0] = (uint8_t)px[0], dst[1] = (uint8_t)px[1], dst[2] = (uint8_t)px[2];
}

// ---- stage 2 helpers: cv::resize(INTER_AREA) paths
enum ResizeMode { kCopy = 0, kAreaFast = 1, kArea = 2, kLinear = 3 };

struct Axis {  // one direction of the resize
    double scale, inv_scale;
    int iscale;
    bool fast, shrink;
};

__device__ __forceinline__ Axis make_axis(int ssize, int dsize) {
    Axis a;
    a.inv_scale = (double)dsize / ssize;
    a.scale = 1.0 / a.inv_scale;
    a.iscale = (int)rint(a.scale);
    a.fast = fabs(a.scale - a.iscale) < 2.220446049250313e-16;
    a.shrink = a.scale >= 1.0;
    return a;
}

// area-mode bilinear coefficients (11-bit fixed point) of destination index d
__device__ __forceinline__ void linear_coef(int d, int ssize, const Axis& ax, int& ofs, int& c0, int& c1) {
    int s = (int)floor(d * ax.scale);
    float f = (float)((d + 1) - (s + 1) * ax.inv_scale);
    f = f <= 0.f ? 0.f : f - floorf(f);
    if (s < 0) f = 0.f, s = 0;
    if (s >= ssize - 1) f = 0.f, s = ssize - 1;
    ofs = s;
    c0 = (int)fminf(fmaxf(rintf((1.f - f) * 2048.f), -32768.f), 32767.f);
    c1 = (int)fminf(fmaxf(rintf(f * 2048.f), -32768.f), 32767.f);
}

// taps of destination index d in the general area path: up to `first + count` weights
struct AreaTaps {
    int sx1, sx2;      // full-weight cells [sx1, sx2)
    float w_lo, w_mid, w_hi;
    bool has_lo, has_hi;
};

__device__ __forceinline__ AreaTaps area_taps(int d, int ssize, double scale) {
    AreaTaps t;
    const double f1 = d * scale, f2 = f1 + scale;
    const double cell = fmin(scale, ssize - f1);
    int sx1 = (int)ceil(f1), sx2 = (int)floor(f2);
    sx2 = min(sx2, ssize - 1);
    sx1 = min(sx1, sx2);
    t.sx1 = sx1, t.sx2 = sx2;
    t.has_lo = sx1 - f1 > 1e-3;
    t.w_lo = (float)((sx1 - f1) / cell);
    t.w_mid = (float)(1.0 / cell);
    t.has_hi = f2 - sx2 > 1e-3;
    t.w_hi = (float)(fmin(fmin(f2 - sx2, 1.0), cell) / cell);
    return t;
}

__device__ __forceinline__ void row_area(const uint8_t* __restrict__ row, const AreaTaps& tx, float buf[3]) {
    buf[0] = buf[1] = buf[2] = 0.f;
    if (tx.has_lo) {
        const uint8_t* s = row + (size_t)(tx.sx1 - 1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) buf[c] = buf[c] + (float)s[c] * tx.w_lo;
    }
    for (int sx = tx.sx1; sx < tx.sx2; ++sx) {
        const uint8_t* s = row + (size_t)sx * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) buf[c] = buf[c] + (float)s[c] * tx.w_mid;
    }
    if (tx.has_hi) {
        const uint8_t* s = row + (size_t)tx.sx2 * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) buf[c] = buf[c] + (float)s[c] * tx.w_hi;
    }
}

__device__ __forceinline__ int clamp_u8(float v) { return (int)fminf(fmaxf(rintf(v), 0.f), 255.f); }

// ---- stage 2 helpers: 8-bit BGR <-> HSV (H in [0,180)) and the jitter between them
__device__ __forceinline__ void color_jitter(int px[3], const ViewParam& v) {
    const int b = px[0], g = px[1], r = px[2];
    const int vmax = max(max(b, g), r), vmin = min(min(b, g), r), diff = vmax - vmin;
    const long long sdiv = vmax ? round_ll(1044480.0 / (1.0 * vmax)) : 0;            // (255 << 12) / v
    const long long hdiv = diff ? round_ll(737280.0 / (6.0 * diff)) : 0;             // (180 << 12) / (6 diff)
    const int sat = (int)((diff * sdiv + 2048) >> 12);
    long long hn = vmax == r ? (g - b) : (vmax == g ? (b - r + 2 * diff) : (r - g + 4 * diff));
    int hue = (int)((hn * hdiv + 2048) >> 12);
    if (hue < 0) hue += 180;
    // the reference scales in float64, clips to [0,255] and truncates to 8 bits
    const int h8 = (int)fmin(fmax(hue * v.h, 0.0), 255.0);
    const int s8 = (int)fmin(fmax(sat * v.s, 0.0), 255.0);
    const int v8 = (int)fmin(fmax(vmax * v.a + v.b, 0.0), 255.0);
    // HSV -> BGR in float32
    const float s = (float)s8 * (1.f / 255.f), val = (float)v8 * (1.f / 255.f);
    float bb, gg, rr;
    if (s == 0.f) {
        bb = gg = rr = val;
    } else {
        float hh = (float)h8 * (6.f / 180.f);
        if (hh >= 6.f) hh = hh - 6.f;
        int sector = (int)floorf(hh);
        float f = hh - (float)sector;
        if ((unsigned)sector >= 6u) sector = 0, f = 0.f;
        float tab[4];
        tab[0] = val;
        tab[1] = val * (1.f - s);
        tab[2] = val * (1.f - s * f);
        tab[3] = val * (1.f - s * (1.f - f));
        // (b, g, r) table indices per sector, packed 2 bits each
        constexpr unsigned kB = 1u | (1u << 2) | (3u << 4) | (0u << 6) | (0u << 8) | (2u << 10);
        constexpr unsigned kG = 3u | (0u << 2) | (0u << 4) | (2u << 6) | (1u << 8) | (1u << 10);
        constexpr unsigned kR = 0u | (2u << 2) | (1u << 4) | (1u << 6) | (3u << 8) | (0u << 10);
        bb = tab[(kB >> (2 * sector)) & 3u];
        gg = tab[(kG >> (2 * sector)) & 3u];
        rr = tab[(kR >> (2 * sector)) & 3u];
    }
    px[0] = clamp_u8(bb * 255.f), px[1] = clamp_u8(gg * 255.f), px[2] = clamp_u8(rr * 255.f);
}

struct Norm {
    float mean[3], stdv[3];
};

// ---- stage 2 extension: Gaussian noise and colour drop
struct PostExt {
    const int* ext;
    const uint32_t* table;  // noise CDF thresholds: n = #{k : table[k] <= u}
    int n_table;
    uint32_t key0, key1, call;
};

// Philox4x32-10 (Salmon et al., SC'11)
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

__device__ __forceinline__ int noise_value(const uint32_t* __restrict__ table, int n_table, uint32_t u) {
    int lo = 0, hi = n_table;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (table[mid] <= u)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// image += clamp(rint(N(0, std)), 0, 255) with uint8 wrap-around, then colour drop
__device__ __forceinline__ void post_ops(int px[3], const PostExt& pe, int n, int B, int pixel) {
    const int flags = pe.ext[(size_t)n * NE];
    if (flags & PECLR_AUG_EXT_NOISE) {
        // counter (pixel, sample, view, call); output word c is channel c
        const uint4 r = philox4x32_10(make_uint4((uint32_t)pixel, (uint32_t)(n % B), (uint32_t)(n / B), pe.call), pe.key0, pe.key1);
        px[0] = (px[0] + noise_value(pe.table, pe.n_table, r.x)) & 255;
        px[1] = (px[1] + noise_value(pe.table, pe.n_table, r.y)) & 255;
        px[2] = (px[2] + noise_value(pe.table, pe.n_table, r.z)) & 255;
    }
    if (flags & PECLR_AUG_EXT_COLOR_DROP) px[0] = px[1] = px[2] = gray_u8(px[0], px[1], px[2]);
}

// ---- stage 2: resize -> colour jitter -> ToTensor/Normalize
template <bool NHWC, bool EXT, class WIN>
__global__ __launch_bounds__(BX* BY) void resize_color_norm_kernel(const uint8_t* __restrict__ crops, int B, WIN win,
                                                                    const double* __restrict__ params, int out_h, int out_w,
                                                                    Norm norm, float* __restrict__ out, PostExt pe) {
    const int n = blockIdx.z;
    const int dx = blockIdx.x * BX + threadIdx.x, dy = blockIdx.y * BY + threadIdx.y;
    if (dx >= out_w || dy >= out_h) return;
    const ViewParam v = load_param(params, n);
    const WinGeom wg = win.window(n);
    const uint8_t* img = crops + wg.off;
    const size_t stride = wg.stride;
    const int sw = v.cw, sh = v.ch;
    int px[3];
    const Axis ax = make_axis(sw, out_w), ay = make_axis(sh, out_h);
    int mode;
    if (sw == out_w && sh == out_h)
        mode = kCopy;
    else if (ax.shrink && ay.shrink)
        mode = (ax.fast && ay.fast) ? kAreaFast : kArea;
    else
        mode = kLinear;

    if (mode == kCopy) {
        const uint8_t* s = img + dy * stride + (size_t)dx * 3;
        px[0] = s[0], px[1] = s[1], px[2] = s[2];
    } else if (mode == kAreaFast) {
        int sum[3] = {0, 0, 0};
        for (int j = 0; j < ay.iscale; ++j) {
            const uint8_t* s = img + (size_t)(dy * ay.iscale + j) * stride + (size_t)dx * ax.iscale * 3;
            for (int i = 0; i < ax.iscale; ++i, s += 3) sum[0] += s[0], sum[1] += s[1], sum[2] += s[2];
        }
        if (ax.iscale == 2 && ay.iscale == 2) {
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = (sum[c] + 2) >> 2;
        } else {
            const float inv = (float)(1.0 / (ax.iscale * ay.iscale));
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = clamp_u8((float)sum[c] * inv);
        }
    } else if (mode == kArea) {
        const AreaTaps tx = area_taps(dx, sw, ax.scale), ty = area_taps(dy, sh, ay.scale);
        float acc[3] = {0.f, 0.f, 0.f}, buf[3];
        if (ty.has_lo) {
            row_area(img + (size_t)(ty.sx1 - 1) * stride, tx, buf);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + buf[c] * ty.w_lo;
        }
        for (int sy = ty.sx1; sy < ty.sx2; ++sy) {
            row_area(img + (size_t)sy * stride, tx, buf);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + buf[c] * ty.w_mid;
        }
        if (ty.has_hi) {
            row_area(img + (size_t)ty.sx2 * stride, tx, buf);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + buf[c] * ty.w_hi;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = clamp_u8(acc[c]);
    } else {
        int xo, xa0, xa1, yo, yb0, yb1;
        linear_coef(dx, sw, ax, xo, xa0, xa1);
        linear_coef(dy, sh, ay, yo, yb0, yb1);
        const int x1 = min(xo + 1, sw - 1), y1 = min(yo + 1, sh - 1);
        const uint8_t *r0 = img + (size_t)yo * stride, *r1 = img + (size_t)y1 * stride;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int s0 = r0[(size_t)xo * 3 + c] * xa0 + r0[(size_t)x1 * 3 + c] * xa1;
            const int s1 = r1[(size_t)xo * 3 + c] * xa0 + r1[(size_t)x1 * 3 + c] * xa1;
            const int o = (((yb0 * (s0 >> 4)) >> 16) + ((yb1 * (s1 >> 4)) >> 16) + 2) >> 2;
            px[c] = min(max(o, 0), 255);
        }
    }
    if (v.color) color_jitter(px, v);
    if (EXT) post_ops(px, pe, n, B, dy * out_w + dx);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = ((float)px[c] / 255.f - norm.mean[c]) / norm.stdv[c];
        if (NHWC)
            out[(((size_t)n * out_h + dy) * out_w + dx) * 3 + c] = t;
        else
            out[(((size_t)n * 3 + c) * out_h + dy) * out_w + dx] = t;
    }
}

}  // namespace
}  // namespace peclr

using namespace peclr;

namespace {

inline bool bad_batch(int B, int n_views) { return B <= 0 || n_views <= 0 || (long long)B * n_views > 65535; }

inline bool bad_ksize(int kx, int ky) {
    return kx < 1 || ky < 1 || !(kx & 1) || !(ky & 1) || kx > PECLR_AUG_MAX_BLUR_KSIZE || ky > PECLR_AUG_MAX_BLUR_KSIZE;
}

// stage 0 over the grid of an ext_h x ext_w image (the batch maximum for a ragged batch); mirror: the left-hand table, or
// nullptr for the plain source
template <class SRC>
int launch_pre(const uint8_t* images, SRC geo, int n_views, int ext_h, int ext_w, const int* ext, const int* coefs,
               const int* mirror, uint8_t* srcs, uint16_t* blur_tmp, hipStream_t s) {
    dim3 grid((ext_w + BX - 1) / BX, (ext_h + BY - 1) / BY, geo.B * n_views);
    if (mirror)
        hipLaunchKernelGGL(pre_rows_kernel<Mirrored<SRC>>, grid, dim3(BX, BY), 0, s, images, Mirrored<SRC>{geo, mirror}, ext, coefs,
                           srcs, blur_tmp);
    else
        hipLaunchKernelGGL(pre_rows_kernel<SRC>, grid, dim3(BX, BY), 0, s, images, geo, ext, coefs, srcs, blur_tmp);
    if (blur_tmp) {
        dim3 gcol((ext_w + BX - 1) / BX, (ext_h + BY * COL_ROWS - 1) / (BY * COL_ROWS), geo.B * n_views);
        hipLaunchKernelGGL(pre_cols_kernel<SRC>, gcol, dim3(BX, BY), 0, s, geo, ext, coefs, blur_tmp, srcs);
    }
    return launch_status();
}

template <class SRC, class WIN>
int launch_warp(const uint8_t* images, SRC geo, WIN win, int n_views, int ext_h, int ext_w, const double* params,
                const int* mirror, uint8_t* crops, hipStream_t s) {
    dim3 grid((ext_w + BX - 1) / BX, (ext_h + BY - 1) / BY, geo.B * n_views);
    if (mirror)
        hipLaunchKernelGGL((warp_crop_kernel<Mirrored<SRC>, WIN>), grid, dim3(BX, BY), 0, s, images, Mirrored<SRC>{geo, mirror}, win,
                           params, crops);
    else
        hipLaunchKernelGGL((warp_crop_kernel<SRC, WIN>), grid, dim3(BX, BY), 0, s, images, geo, win, params, crops);
    return launch_status();
}

// stage 2; pe == nullptr: the recipe's form (no noise, no colour drop)
template <class WIN>
int launch_resize(const uint8_t* crops, int B, int n_views, WIN win, const double* params, int out_h, int out_w,
                  const float* mean, const float* stdv, int channels_last, float* out, const PostExt* pe, hipStream_t s) {
    Norm norm;
    for (int c = 0; c < 3; ++c) {
        norm.mean[c] = mean[c];  // host pointers: three floats each, passed by value to the kernel
        norm.stdv[c] = stdv[c];
        if (!(norm.stdv[c] > 0.f)) return PECLR_ERR_SHAPE;
    }
    dim3 grid((out_w + BX - 1) / BX, (out_h + BY - 1) / BY, B * n_views);
    const PostExt post = pe ? *pe : PostExt{};
    if (pe && channels_last)
        hipLaunchKernelGGL((resize_color_norm_kernel<true, true, WIN>), grid, dim3(BX, BY), 0, s, crops, B, win, params, out_h, out_w, norm, out, post);
    else if (pe)
        hipLaunchKernelGGL((resize_color_norm_kernel<false, true, WIN>), grid, dim3(BX, BY), 0, s, crops, B, win, params, out_h, out_w, norm, out, post);
    else if (channels_last)
        hipLaunchKernelGGL((resize_color_norm_kernel<true, false, WIN>), grid, dim3(BX, BY), 0, s, crops, B, win, params, out_h, out_w, norm, out, post);
    else
        hipLaunchKernelGGL((resize_color_norm_kernel<false, false, WIN>), grid, dim3(BX, BY), 0, s, crops, B, win, params, out_h, out_w, norm, out, post);
    return launch_status();
}

}  // namespace

extern "C" int peclr_augment_warp_crop_u8(const uint8_t* images, int B, int H, int W, int n_views, const double* params,
                                          uint8_t* crops, peclr_stream_t stream) {
    if (!images || !params || !crops) return PECLR_ERR_NULL;
    if (H <= 0 || W <= 0 || bad_batch(B, n_views)) return PECLR_ERR_SHAPE;
    return launch_warp(images, UniformSrc{B, H, W, 1, 1}, UniformWin{H, W}, n_views, H, W, params, nullptr, crops,
                       static_cast<hipStream_t>(stream));
}

extern "C" int peclr_augment_resize_color_norm(const uint8_t* crops, int B, int H, int W, int n_views, const double* params,
                                               int out_h, int out_w, const float* mean, const float* stdv,
                                               int channels_last, float* out, peclr_stream_t stream) {
    if (!crops || !params || !mean || !stdv || !out) return PECLR_ERR_NULL;
    if (H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || bad_batch(B, n_views)) return PECLR_ERR_SHAPE;
    return launch_resize(crops, B, n_views, UniformWin{H, W}, params, out_h, out_w, mean, stdv, channels_last, out, nullptr,
                         static_cast<hipStream_t>(stream));
}

extern "C" int peclr_augment_pre_u8(const uint8_t* images, int B, int H, int W, int n_views, const int* ext,
                                    const int* coefs, int kx, int ky, uint8_t* srcs, uint16_t* blur_tmp,
                                    peclr_stream_t stream) {
    if (!images || !ext || !coefs || !srcs) return PECLR_ERR_NULL;
    if (H <= 0 || W <= 0 || bad_batch(B, n_views)) return PECLR_ERR_SHAPE;
    if (bad_ksize(kx, ky)) return PECLR_ERR_SHAPE;
    return launch_pre(images, UniformSrc{B, H, W, kx, ky}, n_views, H, W, ext, coefs, nullptr, srcs, blur_tmp,
                      static_cast<hipStream_t>(stream));
}

extern "C" int peclr_augment_resize_color_norm_ext(const uint8_t* crops, int B, int H, int W, int n_views,
                                                   const double* params, const int* ext, const uint32_t* noise_table,
                                                   int n_table, uint64_t noise_seed, uint32_t call, int out_h, int out_w,
                                                   const float* mean, const float* stdv, int channels_last, float* out,
                                                   peclr_stream_t stream) {
    if (!crops || !params || !ext || !noise_table || !mean || !stdv || !out) return PECLR_ERR_NULL;
    if (H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || bad_batch(B, n_views) || n_table < 0 || n_table > 255)
        return PECLR_ERR_SHAPE;
    const PostExt pe{ext, noise_table, n_table, (uint32_t)noise_seed, (uint32_t)(noise_seed >> 32), call};
    return launch_resize(crops, B, n_views, UniformWin{H, W}, params, out_h, out_w, mean, stdv, channels_last, out, &pe,
                         static_cast<hipStream_t>(stream));
}

// ---- the same four stages for a batch whose images differ in size (tables: include/peclr_hip.h)
extern "C" int peclr_augment_pre_ragged_u8(const uint8_t* images, int B, int n_views, const int64_t* geom,
                                           int64_t total_bytes, int max_h, int max_w, const int* ext, const int* coefs,
                                           int max_kx, int max_ky, uint8_t* srcs, uint16_t* blur_tmp,
                                           peclr_stream_t stream) {
    if (!images || !geom || !ext || !coefs || !srcs) return PECLR_ERR_NULL;
    if (max_h <= 0 || max_w <= 0 || total_bytes <= 0 || bad_batch(B, n_views)) return PECLR_ERR_SHAPE;
    if (bad_ksize(max_kx, max_ky)) return PECLR_ERR_SHAPE;
    const RaggedSrc geo{B, reinterpret_cast<const long long*>(geom), (size_t)total_bytes};
    return launch_pre(images, geo, n_views, max_h, max_w, ext, coefs, nullptr, srcs, blur_tmp,
                      static_cast<hipStream_t>(stream));
}

extern "C" int peclr_augment_warp_crop_ragged_u8(const uint8_t* images, int B, int n_views, const int64_t* geom,
                                                 const double* params, const int64_t* wins, int max_cw, int max_ch,
                                                 uint8_t* crops, peclr_stream_t stream) {
    if (!images || !geom || !params || !wins || !crops) return PECLR_ERR_NULL;
    if (max_cw <= 0 || max_ch <= 0 || bad_batch(B, n_views)) return PECLR_ERR_SHAPE;
    const RaggedSrc geo{B, reinterpret_cast<const long long*>(geom), 0};
    return launch_warp(images, geo, RaggedWin{reinterpret_cast<const long long*>(wins)}, n_views, max_ch, max_cw, params,
                       nullptr, crops, static_cast<hipStream_t>(stream));
}

extern "C" int peclr_augment_resize_color_norm_ragged(const uint8_t* crops, int B, int n_views, const int64_t* wins,
                                                      const double* params, int out_h, int out_w, const float* mean,
                                                      const float* stdv, int channels_last, float* out,
                                                      peclr_stream_t stream) {
    if (!crops || !wins || !params || !mean || !stdv || !out) return PECLR_ERR_NULL;
    if (out_h <= 0 || out_w <= 0 || bad_batch(B, n_views)) return PECLR_ERR_SHAPE;
    return launch_resize(crops, B, n_views, RaggedWin{reinterpret_cast<const long long*>(wins)}, params, out_h, out_w, mean,
                         stdv, channels_last, out, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" int peclr_augment_resize_color_norm_ragged_ext(const uint8_t* crops, int B, int n_views, const int64_t* wins,
                                                          const double* params, const int* ext,
                                                          const uint32_t* noise_table, int n_table, uint64_t noise_seed,
                                                          uint32_t call, int out_h, int out_w, const float* mean,
                                                          const float* stdv, int channels_last, float* out,
                                                          peclr_stream_t stream) {
    if (!crops || !wins || !params || !ext || !noise_table || !mean || !stdv || !out) return PECLR_ERR_NULL;
    if (out_h <= 0 || out_w <= 0 || bad_batch(B, n_views) || n_table < 0 || n_table > 255) return PECLR_ERR_SHAPE;
    const PostExt pe{ext, noise_table, n_table, (uint32_t)noise_seed, (uint32_t)(noise_seed >> 32), call};
    return launch_resize(crops, B, n_views, RaggedWin{reinterpret_cast<const long long*>(wins)}, params, out_h, out_w, mean,
                         stdv, channels_last, out, &pe, static_cast<hipStream_t>(stream));
}

// ---- left hands: stage 0 or stage 1 of a batch in which `mirror` [B] (device, one int per sample, non-zero = left) flags the
// samples whose image is read mirrored.  Whichever stage reads the caller's images takes the flags -- stage 0 when it runs (the
// warp then reads the per-view sources through the entry points above), stage 1 otherwise.
extern "C" int peclr_augment_warp_crop_mirror_u8(const uint8_t* images, int B, int H, int W, int n_views, const double* params,
                                                 const int* mirror, uint8_t* crops, peclr_stream_t stream) {
    if (!images || !params || !mirror || !crops) return PECLR_ERR_NULL;
    if (H <= 0 || W <= 0 || bad_batch(B, n_views)) return PECLR_ERR_SHAPE;
    return launch_warp(images, UniformSrc{B, H, W, 1, 1}, UniformWin{H, W}, n_views, H, W, params, mirror, crops,
                       static_cast<hipStream_t>(stream));
}

extern "C" int peclr_augment_pre_mirror_u8(const uint8_t* images, int B, int H, int W, int n_views, const int* ext,
                                           const int* coefs, int kx, int ky, const int* mirror, uint8_t* srcs,
                                           uint16_t* blur_tmp, peclr_stream_t stream) {
    if (!images || !ext || !coefs || !mirror || !srcs) return PECLR_ERR_NULL;
    if (H <= 0 || W <= 0 || bad_batch(B, n_views)) return PECLR_ERR_SHAPE;
    if (bad_ksize(kx, ky)) return PECLR_ERR_SHAPE;
    return launch_pre(images, UniformSrc{B, H, W, kx, ky}, n_views, H, W, ext, coefs, mirror, srcs, blur_tmp,
                      static_cast<hipStream_t>(stream));
}

extern "C" int peclr_augment_pre_ragged_mirror_u8(const uint8_t* images, int B, int n_views, const int64_t* geom,
                                                  int64_t total_bytes, int max_h, int max_w, const int* ext, const int* coefs,
                                                  int max_kx, int max_ky, const int* mirror, uint8_t* srcs, uint16_t* blur_tmp,
                                                  peclr_stream_t stream) {
    if (!images || !geom || !ext || !coefs || !mirror || !srcs) return PECLR_ERR_NULL;
    if (max_h <= 0 || max_w <= 0 || total_bytes <= 0 || bad_batch(B, n_views)) return PECLR_ERR_SHAPE;
    if (bad_ksize(max_kx, max_ky)) return PECLR_ERR_SHAPE;
    const RaggedSrc geo{B, reinterpret_cast<const long long*>(geom), (size_t)total_bytes};
    return launch_pre(images, geo, n_views, max_h, max_w, ext, coefs, mirror, srcs, blur_tmp,
                      static_cast<hipStream_t>(stream));
}

extern "C" int peclr_augment_warp_crop_ragged_mirror_u8(const uint8_t* images, int B, int n_views, const int64_t* geom,
                                                        const double* params, const int64_t* wins, int max_cw, int max_ch,
                                                        const int* mirror, uint8_t* crops, peclr_stream_t stream) {
    if (!images || !geom || !params || !wins || !mirror || !crops) return PECLR_ERR_NULL;
    if (max_cw <= 0 || max_ch <= 0 || bad_batch(B, n_views)) return PECLR_ERR_SHAPE;
    const RaggedSrc geo{B, reinterpret_cast<const long long*>(geom), 0};
    return launch_warp(images, geo, RaggedWin{reinterpret_cast<const long long*>(wins)}, n_views, max_ch, max_cw, params,
                       mirror, crops, static_cast<hipStream_t>(stream));
}
