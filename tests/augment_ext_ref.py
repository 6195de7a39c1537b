"""NumPy restatement of the five augmentations TwoViewAugmenter(extended=True) adds -- TEST CODE ONLY.

Composes with oracle/augment_oracle.py (imported, not edited) into the whole per-view pipeline the GPU
kernels run:

    source -> [Sobel] -> [cut-out] -> [Gaussian blur]            stage 0 (csrc/augment.hip pre_* kernels)
           -> [rotate] -> crop -> resize -> [colour jitter]       oracle/augment_oracle.py
           -> [Gaussian noise] -> [colour drop] -> normalise      stage 2

Pixel arithmetic (unpinned, like the oracle's: there is no OpenCV here to pin it against):
  * gray: cvtColor(COLOR_BGR2GRAY) 8U, channel 0 taken as blue, (1868 c0 + 9617 c1 + 4899 c2 + 2^13) >> 14
  * Sobel: cv2.Sobel(gray, CV_64F, 1, 0, 3) + cv2.Sobel(gray, CV_64F, 0, 1, 3), BORDER_REFLECT_101, stored into
    uint8 the way x86 NumPy converts float64 to uint8 (the value modulo 256)
  * Gaussian blur: OpenCV's 8-bit fixed-point separable path, Q8 taps (peclr_amd.augment.gaussian_kernel_q8),
    rows u8 x Q8 exact in 16 bits, columns (sum + 2^15) >> 16, BORDER_REFLECT_101
  * noise: n = clamp(rint(N(0, std)), 0, 255) per channel drawn through an integer CDF table from Philox4x32-10,
    image = (image + n) mod 256 (what `image += cv2.randn(uint8 zeros, 0, std)` does, from another stream)
  * colour drop: gray into all three channels
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from oracle import augment_oracle as A

M32 = np.uint64(0xFFFFFFFF)


def reflect101(i: np.ndarray, n: int) -> np.ndarray:
    """cv::borderInterpolate(BORDER_REFLECT_101) for any offset."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.abs(i) % period
    return np.where(i < n, i, period - i)


def gray_u8(img: np.ndarray) -> np.ndarray:
    c = img.astype(np.int64)
    return (1868 * c[..., 0] + 9617 * c[..., 1] + 4899 * c[..., 2] + 8192) >> 14


def sobel_sum(gray: np.ndarray) -> np.ndarray:
    """dx + dy of the 3x3 Sobel, exact integers (what the reference's two CV_64F Sobel calls hold)."""
    h, w = gray.shape
    ys, xs = reflect101(np.arange(-1, h + 1), h), reflect101(np.arange(-1, w + 1), w)
    g = gray.astype(np.int64)[ys][:, xs]
    dx = (g[:-2, 2:] - g[:-2, :-2]) + 2 * (g[1:-1, 2:] - g[1:-1, :-2]) + (g[2:, 2:] - g[2:, :-2])
    dy = (g[2:, :-2] + 2 * g[2:, 1:-1] + g[2:, 2:]) - (g[:-2, :-2] + 2 * g[:-2, 1:-1] + g[:-2, 2:])
    return dx + dy


def sobel_u8(img: np.ndarray) -> np.ndarray:
    v = (sobel_sum(gray_u8(img)) % 256).astype(np.uint8)
    return np.repeat(v[..., None], 3, axis=2)


def cut_out_u8(img: np.ndarray, rows: Sequence[int], cols: Sequence[int], fill: int) -> np.ndarray:
    out = img.copy()
    out[rows[0]:rows[1], cols[0]:cols[1]] = np.uint8(fill)
    return out


def gaussian_blur_u8(img: np.ndarray, taps_x: Sequence[int], taps_y: Sequence[int]) -> np.ndarray:
    h, w = img.shape[:2]
    rx, ry = len(taps_x) // 2, len(taps_y) // 2
    src = img.astype(np.int64)
    rows = np.zeros_like(src)
    for k, t in enumerate(taps_x):
        rows += t * src[:, reflect101(np.arange(w) - rx + k, w)]
    assert rows.max(initial=0) < 1 << 16  # exact in 16 bits
    acc = np.zeros_like(src)
    for k, t in enumerate(taps_y):
        acc += t * rows[reflect101(np.arange(h) - ry + k, h)]
    return ((acc + (1 << 15)) >> 16).astype(np.uint8)


def philox4x32_10(ctr: np.ndarray, key: Tuple[int, int]) -> np.ndarray:
    """Philox4x32-10 on a [..., 4] uint32 counter array; returns [..., 4] uint32."""
    c = [ctr[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
    return np.stack(c, axis=-1).astype(np.uint32)


def noise_values(table: Sequence[int], u: np.ndarray) -> np.ndarray:
    """n = #{k : table[k] <= u}."""
    return np.searchsorted(np.asarray(table, dtype=np.uint64), u.astype(np.uint64), side="right")


def noise_u8(img: np.ndarray, table: Sequence[int], seed: int, call: int, view: int, sample: int) -> np.ndarray:
    """The stage-2 noise of one (view, sample) output image: counter (pixel, sample, view, call), key = the 64-bit
    seed's low and high words, output word c -> channel c."""
    h, w = img.shape[:2]
    pix = np.arange(h * w, dtype=np.uint64)
    ctr = np.stack([pix, np.full_like(pix, sample), np.full_like(pix, view), np.full_like(pix, call & 0xFFFFFFFF)], axis=1)
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[:, :3].reshape(h, w, 3)
    return ((img.astype(np.int64) + noise_values(table, r)) % 256).astype(np.uint8)


def color_drop_u8(img: np.ndarray) -> np.ndarray:
    return np.repeat(gray_u8(img).astype(np.uint8)[..., None], 3, axis=2)


# ------------------------------------------------------------------ whole pipeline for one view
def pre_view(image: np.ndarray, view: Dict) -> np.ndarray:
    """Stage 0 for a view drawn by TwoViewAugmenter.sample_view (its 'sobel' / 'cut_out' / 'sigma' entries)."""
    from peclr_amd.augment import gaussian_kernel_q8

    img = image
    if view["sobel"]:
        img = sobel_u8(img)
    if view["cut_out"] is not None:
        c = view["cut_out"]
        img = cut_out_u8(img, c["rows"], c["cols"], c["fill"])
    if view["sigma"] is not None:
        kx, ky = view["ksize"]
        img = gaussian_blur_u8(img, gaussian_kernel_q8(kx, view["sigma"]), gaussian_kernel_q8(ky, view["sigma"]))
    return img.copy() if img is image else img


def crop_window(src: np.ndarray, view: Dict) -> np.ndarray:
    """The rotated (warpAffine driven by the already-inverted matrix the product hands the kernel) crop window."""
    x0, y0, cw, ch = view["crop"]
    if view["minv"] is None:
        return src[y0:y0 + ch, x0:x0 + cw]
    orig = A.invert_affine
    try:
        A.invert_affine = lambda m: np.asarray(view["minv"], dtype=np.float64).reshape(2, 3)
        return A.warp_affine_u8(src, np.eye(2, 3), region=(x0, y0, cw, ch))
    finally:
        A.invert_affine = orig


def render_view_ext(image: np.ndarray, view: Dict, resize_wh: Tuple[int, int], noise: Optional[Dict] = None,
                    stages: bool = False):
    """noise: {'table', 'seed', 'call', 'view', 'sample'} -- needed when the view draws noise."""
    out = {"source": pre_view(image, view)}
    out["window"] = crop_window(out["source"], view)
    img = A.resize_area_u8(out["window"], tuple(resize_wh))
    if view["h"] is not None:
        img = A.color_jitter_u8(img, view["h"], view["s"], view["a"], view["b"])
    if view["noise"]:
        img = noise_u8(img, noise["table"], noise["seed"], noise["call"], noise["view"], noise["sample"])
    if view["color_drop"]:
        img = color_drop_u8(img)
    out["final_u8"] = img
    out["tensor"] = A.to_tensor_normalize(img)
    return out if stages else out["tensor"]
