"""NumPy restatements for tests/test_pose_gpu.py: the evaluation crop at any output size (8-bit warpAffine, the
augmenter's fixed-point arithmetic from oracle/augment_oracle.py) and the float64 head of RN_25D_wMLPref."""
import numpy as np

from oracle.augment_oracle import _rint, invert_affine


def warp_affine_u8(img: np.ndarray, T: np.ndarray, size: int) -> np.ndarray:
    """cv.warpAffine(img, T[:2], (size, size)), INTER_LINEAR, BORDER_CONSTANT 0 on u8: [size, size, 3] u8."""
    h, w = img.shape[:2]
    mi = invert_affine(T[:2])
    xs = np.arange(size, dtype=np.float64)
    adelta, bdelta = _rint(mi[0, 0] * xs * 1024.0), _rint(mi[1, 0] * xs * 1024.0)
    xrow = _rint((mi[0, 1] * xs + mi[0, 2]) * 1024.0) + 16
    yrow = _rint((mi[1, 1] * xs + mi[1, 2]) * 1024.0) + 16
    xf = (xrow[:, None] + adelta[None, :]) >> 5
    yf = (yrow[:, None] + bdelta[None, :]) >> 5
    sx, sy, fx, fy = xf >> 5, yf >> 5, xf & 31, yf & 31
    src = img.astype(np.int64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(ok[..., None], src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0)

    acc = (tap(sy, sx) * ((32 - fx) * (32 - fy) * 32)[..., None] + tap(sy, sx + 1) * (fx * (32 - fy) * 32)[..., None]
           + tap(sy + 1, sx) * ((32 - fx) * fy * 32)[..., None] + tap(sy + 1, sx + 1) * (fx * fy * 32)[..., None])
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def crop(img: np.ndarray, T: np.ndarray, size: int, table: np.ndarray) -> np.ndarray:
    """preprocess()'s image for one sample, [size, size, 3] float32 (channels last)."""
    px = warp_affine_u8(img, T, size)
    return np.stack([table[c][px[..., c]] for c in range(3)], axis=-1)


def head_f64(out64: np.ndarray, K: np.ndarray, mlp, bn_eps=(1e-5, 1e-5), eps=1e-8) -> np.ndarray:
    """kp3d [B, 21, 3] in float64 from the fc output [B, 64] (root zrel already zeroed) and K [B or 1, 3, 3]."""
    out = out64.astype(np.float64)
    b = out.shape[0]
    kp25d = out[:, :63].reshape(b, 21, 3).copy()
    kp25d[:, 0, 2] = 0
    uv1 = np.concatenate([kp25d[..., :2], np.ones((b, 21, 1))], axis=2)
    Ki = np.linalg.inv(np.broadcast_to(K.astype(np.float64), (b, 3, 3)))
    ku = np.einsum("bjc,brc->bjr", uv1, Ki)
    z = kp25d[..., 2]
    xm, ym, xn, yn, zm, zn = ku[:, 3, 0], ku[:, 3, 1], ku[:, 8, 0], ku[:, 8, 1], z[:, 3], z[:, 8]
    a = (xn - xm) ** 2 + (yn - ym) ** 2
    bq = 2 * (zn * (xn ** 2 + yn ** 2 - xn * xm - yn * ym) + zm * (xm ** 2 + ym ** 2 - xn * xm - yn * ym))
    c = (xn * zn - xm * zm) ** 2 + (yn * zn - ym * zm) ** 2 + (zn - zm) ** 2 - 1
    d = bq ** 2 - 4 * a * c
    a = np.where(np.isnan(a), a, np.maximum(a, eps))
    d = np.where(np.isnan(d), d, np.maximum(d, eps))
    zr = np.clip((-bq + np.sqrt(d)) / (2 * a), 4.0, 50.0)
    x = np.concatenate([z, ku[..., :2].reshape(b, 42), zr[:, None]], axis=1)
    w0, b0, g1, be1, rm1, rv1, w3, b3, g4, be4, rm4, rv4, w6, b6 = [np.asarray(t, dtype=np.float64) for t in mlp]

    def bn(h, g, be, rm, rv, e):
        return (h - rm) / np.sqrt(rv + e) * g + be

    def leaky(h):
        return np.where(h > 0, h, 0.01 * h)

    h = leaky(bn(x @ w0.T + b0, g1, be1, rm1, rv1, bn_eps[0]))
    h = leaky(bn(h @ w3.T + b3, g4, be4, rm4, rv4, bn_eps[1]))
    zroot = zr + (h @ w6.T + b6)[:, 0]
    return ku * (z + zroot[:, None])[..., None]
