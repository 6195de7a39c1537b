"""Two-view augmentation producing the hybrid2 batch dict on the device.

Mirrors `Data_Set.prepare_hybrid2_sample` (reference src/data_loader/data_set.py:357-384) +
`SampleAugmenter.transform_sample` (src/data_loader/sample_augmenter.py:47-129) + ToTensor/Normalize
(src/data_loader/utils.py:283-293) for the published recipe (README.md: --color_jitter
--random_crop --rotate --crop -resize), split where the hardware wants it split:

  host   the PARAMETER side, per sample and in the reference's draw order from Python's `random`:
         angle, [crop margin], [jitter x, jitter y], [h, s, a, b]; crop box, rotation centre and
         matrix, jitter_x / jitter_y.  A few dozen scalar operations per sample on the very torch ops
         the reference uses (float32 tensor mean / max / pow), so that the drawn parameters equal the
         reference's for the same seed (pinned by tests/golden/g9_augment_params.json).
  device the PIXEL side for the whole batch and both views: csrc/augment.hip (two launches).

With `TwoViewAugmenter(..., device_draws=True)` the parameter side of these recipe flags runs on the device as well: one
launch (csrc/augment_draw.hip) computes the same function of Philox uniforms for the whole batch, the two pixel launches follow
on the `params` it wrote, and a call with device inputs neither synchronises with the host nor reads it (see `__init__`).

The emitted dict is what torch's default collate makes of the reference's per-sample dicts:
`transformed_image{1,2}` float32 [B,3,S,S]; `jitter_{x,y}_{1,2}` int64 [B]; `angle_{1,2}` float64 [B]
(only with rotate); `h/s/a/b_{1,2}` float64 [B] (only with colour jitter); `crop_margin_scale_{1,2}`
float64 [B]; `blur_flag_{1,2}` bool [B].

The other five flags of the reference (sobel_filter, cut_out, gaussian_blur, gaussian_noise,
color_drop) are opt-in: `TwoViewAugmenter(..., extended=True)`.  Without it they raise
NotImplementedError.  With it their draws join the reference's order and their pixels run in two
more device stages (see `TwoViewAugmenter.__init__`).  `resize` is required either way (without it
the reference's crops have per-sample sizes and cannot be collated either).

Left hands: the reference's YouTube-3D-Hands loader turns every left hand into a right one before augmentation
(src/data_loader/youtube_loader.py:151-155: cv2.flip(img, 1) and x <- W - x).  Pass `is_left` and the flagged samples'
images are READ mirrored inside the pixel stages (csrc/augment.hip; no flipped copy on the host or the device) while their
joints follow the loader's rule; a batch mixes left and right hands in the same launches.

The images of one batch may differ in size (the reference concatenates YouTube-3D-Hands frames, of whatever size
the video had, with FreiHAND's 224 x 224, and augments each sample on its own): pass `RaggedImages`, or a list of
HWC arrays, instead of one [B,H,W,3] tensor.  The draws, the launches and the emitted dict are the same; every
sample comes out as it would alone.
"""
from __future__ import annotations

import math
import random as _random
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _capi

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
PARENT_JOINT, CHILD_JOINT = 0, 2  # wrist, index_mcp (reference data_loader/utils.py:15-16)
_UNSUPPORTED = ("sobel_filter", "cut_out", "gaussian_blur", "gaussian_noise", "color_drop")
# per-(view, sample) extension record, include/peclr_hip.h PECLR_AUG_EXT_INTS
EXT_INTS = 8
EXT_SOBEL, EXT_CUT_OUT, EXT_BLUR, EXT_NOISE, EXT_COLOR_DROP = 1, 2, 4, 8, 16
EXT_PRE = EXT_SOBEL | EXT_CUT_OUT | EXT_BLUR
EXT_POST = EXT_NOISE | EXT_COLOR_DROP
MAX_BLUR_KSIZE = 257  # csrc/augment.hip's stage-0 limit: radius 128, enough for images up to 2048 on a side

DEFAULT_PARAMS = {  # reference src/experiments/config/training_config.json
    "crop_margin": 1.25, "crop_margin_range": [0.9, 1.5], "hue_factor_range": [0.01, 1.0], "max_angle": 45,
    "min_angle": -45, "resize_shape": [128, 128], "sat_factor_range": [0.01, 1.0],
    "value_factor_alpha_range": [0.5, 1], "value_factor_beta_range": [5, 20], "crop_box_jitter": [0.0, 15.0],
    "cut_out_fraction": [0.0, 0.16], "sobel_kernel": 3, "noise_std": 25,
}
RECIPE_FLAGS = {"color_jitter": True, "random_crop": True, "rotate": True, "crop": True, "resize": True}


def convert_to_2_5d(k: Tensor, joints3d: Tensor) -> Tuple[Tensor, Tensor]:
    """Pinhole projection + root-relative scaled depth (reference data_loader/utils.py:19-33)."""
    scale = (((joints3d[CHILD_JOINT] - joints3d[PARENT_JOINT]) ** 2).sum()) ** 0.5
    joints25d = ((k @ joints3d.T).T) / joints3d[:, -1:]
    joints25d[:, -1] = (joints3d[:, -1] - joints3d[PARENT_JOINT, -1]) / scale
    return joints25d, scale


def _rotation_matrix(center: Tuple[int, int], angle: float) -> List[List[float]]:
    """OpenCV's getRotationMatrix2D(center, angle, 1.0) (documented formula), float64."""
    a = angle * math.pi / 180.0
    al, be = math.cos(a), math.sin(a)
    return [[al, be, (1 - al) * center[0] - be * center[1]], [-be, al, be * center[0] + (1 - al) * center[1]]]


def _invert_affine(m: List[List[float]]) -> List[float]:
    """Destination -> source map, the way warpAffine derives it from the forward matrix."""
    (m0, m1, m2), (m3, m4, m5) = m
    d = m0 * m4 - m1 * m3
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m4 * d, m0 * d
    m0, m1, m3, m4 = a11, m1 * -d, m3 * -d, a22
    b1 = -m0 * m2 - m1 * m5
    b2 = -m3 * m2 - m4 * m5
    return [m0, m1, b1, m3, m4, b2]


def blur_ksize(image_hw: Tuple[int, int]) -> Tuple[int, int]:
    """gaussian_blur_sample's kernel size from the FULL source shape: int(0.1 * side), made odd.  cv2 reads
    the tuple as (width, height), so the HORIZONTAL length comes from H and the vertical one from W (the
    reference's swap, visible on non-square images).  Returns (horizontal, vertical)."""
    kx, ky = int(image_hw[0] * 0.1), int(image_hw[1] * 0.1)
    return kx + 1 if kx % 2 == 0 else kx, ky + 1 if ky % 2 == 0 else ky


def gaussian_kernel_q8(n: int, sigma: float) -> List[int]:
    """The 8-bit fixed-point Gaussian taps (8 fractional bits, summing to 256) of cv2.GaussianBlur's bit-exact
    8U path.  Restated from memory of OpenCV 4.4's getGaussianKernelBitExact + getGaussianKernelFixedPoint_ED
    (imgproc/src/smooth.dispatch.cpp); no OpenCV source, wheel or cv2 is available to check it, so like the
    warp / resize / HSV restatements it is unpinned.  float64 Gaussian normalised to 1 (OpenCV uses a
    software double, which may differ from libm's exp in the last bit); error-diffused round-half-even from
    the outer taps inwards; the centre tap takes what is left of 256."""
    if n < 1 or n % 2 == 0:
        raise ValueError(f"Gaussian kernel size must be odd and positive, got {n}")
    if n == 1:
        return [256]
    scale2x = -0.125 / (sigma * sigma)
    half = (n - 1) // 2
    values = [math.exp(float((1 - n + 2 * i) ** 2) * scale2x) for i in range(half)]
    total = 0.0
    for t in values:
        total += t
    total = total * 2.0 + 1.0
    mul = 1.0 / total
    taps, err, acc = [0] * n, 0.0, 0
    for i in range(half):
        adj = values[i] * mul * 256.0 + err
        v = round(adj)  # Python's round: half to even, as cvRound
        err = adj - v
        taps[i] = taps[n - 1 - i] = v
        acc += v
    taps[half] = 256 - 2 * acc
    return taps


def noise_cdf_table(std: float) -> List[int]:
    """uint32 thresholds T[k] = round(2^32 * P(n <= k)) of n = clamp(rint(N(0, std)), 0, 255), the per-channel
    value cv2.randn writes into a uint8 matrix; only the entries below 2^32 are kept.  A uniform uint32 u
    maps to n = #{k : T[k] <= u}, so each n has probability (T[n] - T[n-1]) / 2^32, within 2^-32 of the exact
    discrete probability."""
    if not std >= 0:
        raise ValueError(f"noise_std must be >= 0, got {std}")
    table = []
    for k in range(255):
        cdf = 1.0 if std == 0 else 1.0 - 0.5 * math.erfc((k + 0.5) / (std * math.sqrt(2.0)))
        t = int(round(cdf * 2.0 ** 32))
        if t >= 2 ** 32:
            break
        table.append(t)
    return table


def _image_hw(image, i: int) -> Tuple[int, int]:
    """(H, W) of one HWC uint8 image (NumPy array or tensor), or the reason it is not one."""
    if not isinstance(image, (np.ndarray, Tensor)):
        raise TypeError(f"image {i}: expected a NumPy array or a tensor, got {type(image).__name__}")
    if image.dtype not in (np.uint8, torch.uint8):
        raise TypeError(f"image {i}: expected uint8 pixels, got {image.dtype}")
    if len(image.shape) != 3 or image.shape[2] != 3:
        raise ValueError(f"image {i}: expected [H,W,3], got {tuple(image.shape)}")
    h, w = int(image.shape[0]), int(image.shape[1])
    if h < 1 or w < 1:
        raise ValueError(f"image {i}: empty ({h}x{w})")
    return h, w


def check_is_left(is_left, b: int) -> Optional[List[bool]]:
    """`is_left` of a batch of b samples -> a list of b bools (None stays None).  Accepts a sequence, NumPy array or tensor of
    bools or of integers 0 / 1; anything else, or another length, raises.  No native call."""
    if is_left is None:
        return None
    a = is_left.detach().cpu().numpy() if isinstance(is_left, Tensor) else np.asarray(is_left)
    if a.ndim != 1 or a.shape[0] != b:
        raise ValueError(f"is_left: expected {b} entries, one per sample, got shape {tuple(a.shape)}")
    if a.dtype != np.bool_:
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"is_left: expected bools or integers 0 / 1, got {a.dtype}")
        if ((a != 0) & (a != 1)).any():
            raise ValueError("is_left: integer entries must be 0 or 1")
    return [bool(x) for x in a]


def mirror_table(left: Optional[List[bool]], sizes: Sequence[Tuple[int, int]]) -> Optional[Tensor]:
    """include/peclr_hip.h's per-sample table of a batch with left hands: int32 [B] (host), the image's width for a left
    sample and 0 otherwise (the pixel stages read non-zero as "mirrored", the label kernel reads the width).  None when
    no sample is left: such a batch takes the entry points without the table."""
    if left is None or not any(left):
        return None
    return torch.tensor([int(hw[1]) if l else 0 for l, hw in zip(left, sizes)], dtype=torch.int32)


class RaggedImages:
    """A batch of HWC uint8 images of different sizes as ONE packed device buffer, back to back and unpadded (image
    starts need no alignment).  data: 1-D uint8 HIP tensor; sizes: the B (H, W) pairs; offsets: int64 [B] byte offset
    of each image in `data` (host tensor)."""

    def __init__(self, data: Tensor, sizes: Sequence[Tuple[int, int]]):
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        self.offsets, total = self.layout(self.sizes)
        if data.dtype != torch.uint8 or data.dim() != 1 or data.numel() != total:
            raise ValueError(f"RaggedImages: {len(self.sizes)} images of these sizes are {total} bytes, got "
                             f"{data.dtype} {tuple(data.shape)}")
        self.data = data

    def __len__(self) -> int:
        return len(self.sizes)

    @property
    def device(self):
        return self.data.device

    @staticmethod
    def layout(sizes: Sequence[Tuple[int, int]]) -> Tuple[Tensor, int]:
        """[(H, W), ...] -> (int64 [B] byte offsets, total bytes): the running sums of H * W * 3 (Python integers,
        so exact past 2^31 bytes)."""
        offsets, total = [], 0
        for h, w in sizes:
            if h < 1 or w < 1:
                raise ValueError(f"RaggedImages: empty image ({h}x{w})")
            offsets.append(total)
            total += int(h) * int(w) * 3
        return torch.tensor(offsets, dtype=torch.int64), total

    @staticmethod
    def check(images) -> List[Tuple[int, int]]:
        """The sizes of a list of HWC uint8 images; raises on anything else.  No device call."""
        if len(images) == 0:
            raise ValueError("RaggedImages: an empty list of images")
        return [_image_hw(im, i) for i, im in enumerate(images)]

    @classmethod
    def from_list(cls, images, device) -> "RaggedImages":
        """images: HWC uint8 NumPy arrays or host tensors.  Packed into one pinned host buffer, then ONE non-blocking
        copy.  (Tensors already on `device` are concatenated there instead.)"""
        sizes = cls.check(images)
        if all(isinstance(im, Tensor) and im.is_cuda for im in images):
            return cls(torch.cat([im.reshape(-1) for im in images]).to(device), sizes)
        offsets, total = cls.layout(sizes)
        host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        flat = host.numpy()
        for im, off, (h, w) in zip(images, offsets.tolist(), sizes):
            src = im.detach().cpu().numpy() if isinstance(im, Tensor) else im
            flat[off:off + h * w * 3] = np.ascontiguousarray(src).reshape(-1)
        return cls(host.to(device, non_blocking=True), sizes)


class TwoViewAugmenter:
    def __init__(self, flags: Optional[Dict[str, bool]] = None, params: Optional[Dict] = None, rng=None,
                 channels_last: bool = True, extended: bool = False, np_rng=None, noise_seed: Optional[int] = None,
                 device_draws: bool = False, draw_seed: Optional[int] = None):
        """flags / params: the reference's `augmentation_flags` / `augmentation_params` (missing flags
        are off, missing params take training_config.json's values).  rng: object with `.uniform`
        and `.getrandbits` (default: Python's global `random`, the generator the reference draws from).

        extended=True accepts the reference's other five flags (sobel_filter, cut_out, gaussian_blur,
        gaussian_noise, color_drop); their draws are interleaved in the reference's order and cut-out's
        joint index and fill come from `np_rng` (default: the `np.random` module, the global legacy state
        the reference draws them from).  They are opt-in because two of them cannot match the reference
        pixel for pixel by construction:
          * gaussian_noise: the reference draws with cv2.randn from OpenCV's global RNG, a stream this
            project cannot reproduce.  The noise here has the same distribution (a clamped, rounded normal
            of std `noise_std`, added with uint8 wrap-around) from a counter-based Philox4x32-10 generator
            keyed by `noise_seed` (default: torch.initial_seed()) and advanced on every call; it consumes
            nothing from `rng` or `np_rng`.
          * sobel_filter: the reference stores the float64 Sobel sum into uint8, which follows x86 NumPy's
            float-to-uint8 conversion (the value modulo 256); that is what is done here.
        Blur's 8-bit fixed-point path is a restatement of OpenCV's (see `gaussian_kernel_q8`).

        device_draws=True moves the parameter side of the recipe flags to the device: ONE launch (csrc/augment_draw.hip) computes
        for every (view, sample) what `sample_view` computes -- the same function, in the same float32 / float64 arithmetic, of
        uniforms that come from Philox4x32-10 keyed by `draw_seed` (default: torch.initial_seed()) instead of from `rng`; the
        stream is NOT Python's, so a seeded host run and a device run draw different numbers of the same distribution.  The
        call counter lives on the device and advances with every launch, also when a hipGraph replays it.  A dense call with
        device images, device joints and `is_left` None or a device tensor then makes no host synchronisation and can be
        captured with torch.cuda.graph (call once, or `draw_state(device)`, before the capture: the state is allocated on first
        use).  The five `extended` flags and a caller's `rng` / `np_rng` are refused with it; an empty crop window, for which
        the host path raises, is clamped to one pixel and counted (`bad_windows`)."""
        self.flags = dict(RECIPE_FLAGS if flags is None else flags)
        self.params = dict(DEFAULT_PARAMS, **(params or {}))
        self.extended = extended
        self.device_draws = bool(device_draws)
        if device_draws:
            for k in _UNSUPPORTED:
                if self.flags.get(k):
                    raise NotImplementedError(f"augmentation '{k}' is drawn on the host only: device draws cover the recipe "
                                              "flags (rotate, crop, random_crop, resize, color_jitter)")
            if rng is not None or np_rng is not None:
                raise ValueError("device_draws=True draws from Philox keyed by draw_seed: rng / np_rng would be ignored")
        elif draw_seed is not None:
            raise ValueError("draw_seed is the key of the device draws: pass device_draws=True with it")
        self.draw_seed = (torch.initial_seed() if draw_seed is None else int(draw_seed)) & (2 ** 64 - 1)
        self._draw_state: Dict = {}  # device -> (call, counters), _capi.augment_draw_state
        self._blur_false: Dict = {}  # (device, B) -> the all-false blur_flag entry
        if not extended:
            for k in _UNSUPPORTED:
                if self.flags.get(k):
                    raise NotImplementedError(f"augmentation '{k}' is not part of the GPU recipe "
                                              "(rotate, crop, random_crop, resize, color_jitter)")
        elif self.flags.get("sobel_filter") and self.params["sobel_kernel"] != 3:
            raise ValueError(f"sobel_filter supports sobel_kernel=3 only (the reference config's value), "
                             f"got {self.params['sobel_kernel']}")
        if not self.flags.get("resize"):
            raise NotImplementedError("the GPU augmenter needs resize=True: crops have per-sample sizes otherwise")
        self.rng = rng if rng is not None else _random
        self.np_rng = np_rng if np_rng is not None else np.random
        self.channels_last = channels_last
        self.noise_seed = (torch.initial_seed() if noise_seed is None else int(noise_seed)) & (2 ** 64 - 1)
        self.noise_call = 0  # Philox counter word: advances on every __call__
        self._noise_table = None

    # ---- host: parameters of one view (sample_augmenter.py:47-129, parameter side)
    def _crop_size(self, joints: Tensor, jitter: Sequence[int], crop_margin: float) -> Tuple[int, int, int, int, int]:
        center_y, center_x = int(torch.mean(joints[:, 1])), int(torch.mean(joints[:, 0]))
        far = torch.max((joints[:, 1] - center_y) ** 2 + (joints[:, 0] - center_x) ** 2)
        side = int(far ** 0.5 * crop_margin)
        origin_x = max(center_x - side + jitter[0], 0)
        origin_y = max(center_y - side + jitter[1], 0)
        return origin_x, origin_y, int(2 * side), center_x - side - origin_x, center_y - side - origin_y

    def sample_view(self, joints25d: Tensor, image_hw: Tuple[int, int], always_crop: bool = True) -> Dict:
        """always_crop=False is the supervised mode (`transform_sample` without an override jitter): the crop happens only
        with the `crop` flag; without it the window is the whole image and neither the margin nor the jitter is drawn."""
        f, p, rng = self.flags, self.params, self.rng
        h_img, w_img = image_hw
        joints = joints25d.detach().to("cpu", torch.float32).clone()
        view: Dict = {"angle": None, "h": None, "s": None, "a": None, "b": None, "blur_flag": False, "minv": None,
                      "sobel": False, "cut_out": None, "sigma": None, "ksize": None, "noise": False, "color_drop": False,
                      "rot": None}
        # augmentations the reference applies first, each decided by one bit drawn only when its flag is on
        if f.get("sobel_filter") and rng.getrandbits(1):
            view["sobel"] = True
        if f.get("cut_out") and rng.getrandbits(1):
            view["cut_out"] = self._cut_out_box(joints, h_img, w_img)
        if f.get("gaussian_blur") and rng.getrandbits(1):
            view["blur_flag"] = True
            view["sigma"] = rng.uniform(0.1, 2.0)
            view["ksize"] = blur_ksize(image_hw)
        if f.get("rotate"):
            ox, oy, side, _, _ = self._crop_size(joints, (0, 0), 0.0)
            center = (int(ox + side / 2), int(oy + side / 2))
            angle = rng.uniform(p["max_angle"], p["min_angle"]) // 1  # the reference swaps min/max on load
            rot = _rotation_matrix(center, angle)
            hom = joints.double()
            hom[:, -1] = 1.0
            joints[:, :-1] = (hom @ torch.tensor(rot, dtype=torch.float64).T).float()
            view["angle"], view["minv"], view["rot"] = angle, _invert_affine(rot), rot
        if not always_crop and not f.get("crop"):
            return self._finish_view(view, jitter_x=0, jitter_y=0, crop_margin_scale=None, origin=None, crop=(0, 0, w_img, h_img))
        # hybrid2 always crops: with the crop flag off it passes a zero jitter (data_set.py:359-364)
        if f.get("random_crop"):
            margin = rng.uniform(p["crop_margin_range"][0], p["crop_margin_range"][1])
        else:
            margin = p["crop_margin"]
        if f.get("crop"):
            jitter = (int(rng.uniform(0, p["crop_box_jitter"][1])), int(rng.uniform(0, p["crop_box_jitter"][1])))
        else:
            jitter = (0, 0)
        ox, oy, side, jx, jy = self._crop_size(joints, jitter, margin)
        x0, y0 = min(ox, w_img), min(oy, h_img)
        cw, ch = min(ox + side, w_img) - x0, min(oy + side, h_img) - y0
        if cw <= 0 or ch <= 0:
            raise ValueError(f"empty crop window (origin {ox},{oy}, side {side}) for a {w_img}x{h_img} image: "
                             "the reference's cv2.resize fails on it too")
        return self._finish_view(view, jitter_x=jx, jitter_y=jy, crop_margin_scale=margin, origin=(ox, oy), crop=(x0, y0, cw, ch))

    def _finish_view(self, view: Dict, **window) -> Dict:
        """The draws that follow the crop window."""
        f, p, rng = self.flags, self.params, self.rng
        view.update(window)
        if f.get("color_jitter"):
            view["h"] = rng.uniform(*p["hue_factor_range"])
            view["s"] = rng.uniform(*p["sat_factor_range"])
            view["a"] = rng.uniform(*p["value_factor_alpha_range"])
            view["b"] = rng.uniform(*p["value_factor_beta_range"])
        # ... and last
        if f.get("gaussian_noise") and rng.getrandbits(1):
            view["noise"] = True
        if f.get("color_drop") and rng.getrandbits(1):
            view["color_drop"] = True
        return view

    def _cut_out_box(self, joints: Tensor, h_img: int, w_img: int) -> Dict:
        """cut_out_sample + get_random_cut_out_box (sample_augmenter.py:314-373) on the unrotated joints.  The
        reference centres the ROWS on the joint's x and the COLUMNS on its y; kept.  `a` is a float32 tensor,
        as there, and `uniform(a, a)` only consumes a draw."""
        joint = int(self.np_rng.randint(0, 20, 1)[0])  # joint 20 is never picked
        ratio = self.rng.uniform(*self.params["cut_out_fraction"])
        d0, d1 = int(h_img * ratio), int(w_img * ratio)
        a0 = joints[joint, 0] - d0 / 2
        a1 = joints[joint, 1] - d1 / 2
        t0 = int(self.rng.uniform(a0, a0))
        t1 = int(self.rng.uniform(a1, a1))
        fill = int(np.uint8(self.np_rng.randint(0, 255, 1))[0])
        r0, r1 = (int(v) for v in np.clip([t0, t0 + d0], 0, h_img))
        c0, c1 = (int(v) for v in np.clip([t1, t1 + d1], 0, w_img))
        return {"joint": joint, "ratio": ratio, "rows": (r0, r1), "cols": (c0, c1), "fill": fill}

    @staticmethod
    def ext_flags(view: Dict) -> int:
        return ((EXT_SOBEL if view["sobel"] else 0) | (EXT_CUT_OUT if view["cut_out"] is not None else 0)
                | (EXT_BLUR if view["sigma"] is not None else 0) | (EXT_NOISE if view["noise"] else 0)
                | (EXT_COLOR_DROP if view["color_drop"] else 0))

    @classmethod
    def pack_ext(cls, views: List[List[Dict]]):
        """include/peclr_hip.h's `ext` records [V][B][PECLR_AUG_EXT_INTS] and the Q8 blur taps they point at
        (per blurred view: the horizontal taps, then the vertical ones)."""
        recs, coefs = [], []
        for vs in views:
            rows = []
            for w in vs:
                cut = w["cut_out"]
                rec = [cls.ext_flags(w), *(cut["rows"] if cut else (0, 0)), *(cut["cols"] if cut else (0, 0)),
                       cut["fill"] if cut else 0, -1, 0]
                if w["sigma"] is not None:
                    rec[6] = len(coefs)
                    coefs += gaussian_kernel_q8(w["ksize"][0], w["sigma"]) + gaussian_kernel_q8(w["ksize"][1], w["sigma"])
                rows.append(rec)
            recs.append(rows)
        return torch.tensor(recs, dtype=torch.int32), torch.tensor(coefs or [0], dtype=torch.int32)

    def noise_table(self) -> Tuple[Tensor, int]:
        """`noise_cdf_table` as int32 storage of the uint32 thresholds (at least one element) and its length."""
        if self._noise_table is None:
            table = noise_cdf_table(float(self.params["noise_std"]))
            t = np.array(table or [0], dtype=np.uint32).view(np.int32)
            self._noise_table = (torch.from_numpy(t.copy()), len(table))
        return self._noise_table

    @staticmethod
    def pack(view: Dict) -> List[float]:
        """One record of include/peclr_hip.h's `params` layout."""
        rot = view["minv"] is not None
        col = view["h"] is not None
        return ([*(view["minv"] if rot else [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), float(rot), *map(float, view["crop"]),
                 float(col), *((view["h"], view["s"], view["a"], view["b"]) if col else (1.0, 1.0, 1.0, 0.0))])

    def sample_batch(self, joints25d: Tensor, image_hw: Union[Tuple[int, int], Sequence[Tuple[int, int]]], is_left=None):
        """Draws view 1 then view 2 for each sample in turn (the order a dataset iterates).  image_hw: one (H, W)
        for the whole batch, or one per sample.  is_left: per sample; the draws of a left sample read its joints, given in
        the STORED image's coordinates, as x <- W - x in float32 -- the reference loader's rule (W, not W - 1: the mirrored
        image's column of x is W - 1 - x, but the joints only place the crop window here, and drawing the windows the
        reference draws is this project's contract)."""
        views: List[List[Dict]] = [[], []]
        if isinstance(image_hw[0], (int, np.integer)):
            image_hw = [tuple(image_hw)] * len(joints25d)
        elif len(image_hw) != len(joints25d):
            raise ValueError(f"{len(image_hw)} image sizes for {len(joints25d)} samples")
        left = check_is_left(is_left, len(joints25d))
        for i, (j, hw) in enumerate(zip(joints25d, image_hw)):
            if left is not None and left[i]:
                j = j.detach().to("cpu", torch.float32).clone()
                j[:, 0] = int(hw[1]) - j[:, 0]
            for v in (0, 1):
                views[v].append(self.sample_view(j, (int(hw[0]), int(hw[1]))))
        params = torch.tensor([[self.pack(w) for w in views[v]] for v in (0, 1)], dtype=torch.float64)
        return params, views

    @staticmethod
    def collate(views: List[List[Dict]]) -> Dict[str, Tensor]:
        out: Dict[str, Tensor] = {}
        for v in (0, 1):
            for key in ("angle", "jitter_x", "jitter_y", "h", "s", "a", "b", "blur_flag", "crop_margin_scale"):
                vals = [w[key] for w in views[v]]
                if vals[0] is None:
                    continue  # the reference drops None entries (data_set.py:382-383)
                if isinstance(vals[0], bool):
                    t = torch.tensor(vals, dtype=torch.bool)
                elif isinstance(vals[0], int):
                    t = torch.tensor(vals, dtype=torch.int64)
                else:
                    t = torch.tensor(vals, dtype=torch.float64)
                out[f"{key}_{v + 1}"] = t
        return out

    @staticmethod
    def ragged_tables(sizes: Sequence[Tuple[int, int]], offsets: Tensor, views: List[List[Dict]]) -> Tuple[Tensor, Tensor]:
        """include/peclr_hip.h's host tables of a mixed-size batch: geom [B,5] int64 (byte offset, H, W and the
        image's own blur lengths) and wins [V,B,4] int64 (byte offset, row stride, width, height of each crop window
        in the PACKED scratch: window after window, row stride = width)."""
        geom = torch.tensor([[off, h, w, *blur_ksize((h, w))] for off, (h, w) in zip(offsets.tolist(), sizes)],
                            dtype=torch.int64)
        wins, at = [], 0
        for vs in views:
            rows = []
            for w in vs:
                _, _, cw, ch = w["crop"]
                rows.append([at, cw, cw, ch])
                at += cw * ch * 3
            wins.append(rows)
        return geom, torch.tensor(wins, dtype=torch.int64)

    def _check_blur_sizes(self, sizes: Sequence[Tuple[int, int]]):
        if self.extended and self.flags.get("gaussian_blur"):
            for h, w in sizes:
                if max(blur_ksize((h, w))) > MAX_BLUR_KSIZE:
                    raise ValueError(f"gaussian_blur: a {h}x{w} image needs kernels {blur_ksize((h, w))}, "
                                     f"longer than the device's {MAX_BLUR_KSIZE}")

    def _call_ragged(self, images, joints25d: Tensor, is_left=None) -> Dict[str, Tensor]:
        """Everything that can be refused is refused before the first device call."""
        if isinstance(images, RaggedImages):
            sizes = images.sizes
        else:
            sizes = RaggedImages.check(images)
        b = len(sizes)
        if len(joints25d) != b:
            raise ValueError(f"{b} images for {len(joints25d)} samples of joints")
        self._check_blur_sizes(sizes)
        left = check_is_left(is_left, b)
        params, views = self.sample_batch(joints25d, sizes, left)
        if not isinstance(images, RaggedImages):
            dev = next((im.device for im in images if isinstance(im, Tensor) and im.is_cuda), torch.device("cuda"))
            images = RaggedImages.from_list(images, dev)
        dev = images.device
        geom, wins = self.ragged_tables(sizes, images.offsets, views)
        mirror = mirror_table(left, sizes)
        lr = {} if mirror is None else {"mirror": mirror.to(dev, non_blocking=True)}  # no left hand: today's calls as they are
        rw, rh = self.params["resize_shape"]
        call = self.noise_call
        self.noise_call += 1
        ops = 0
        for vs in views:
            for view in vs:
                ops |= self.ext_flags(view)
        if not ops:  # as in __call__: the recipe's two launches
            out = _capi.augment_views_ragged(images.data, geom, wins, params.to(dev, non_blocking=True), (rh, rw),
                                             IMAGENET_MEAN, IMAGENET_STD, self.channels_last, **lr)[0]
        else:
            ext, coefs = self.pack_ext(views)
            table, n_table = self.noise_table()
            out = _capi.augment_views_ragged_ext(images.data, geom, wins, params.to(dev, non_blocking=True),
                                                 ext.to(dev, non_blocking=True), coefs.to(dev, non_blocking=True),
                                                 table.to(dev, non_blocking=True), n_table, self.noise_seed, call, ops,
                                                 (rh, rw), IMAGENET_MEAN, IMAGENET_STD, self.channels_last, **lr)[0]
        batch = {"transformed_images": out, "transformed_image1": out[:b], "transformed_image2": out[b:]}
        batch.update({k: t.to(dev, non_blocking=True) for k, t in self.collate(views).items()})
        if left is not None:
            batch["is_left"] = torch.tensor(left, dtype=torch.bool).to(dev, non_blocking=True)
        return batch

    # ---- device: the parameter side (device_draws=True)
    def draw_flags(self) -> int:
        """The recipe flags as include/peclr_hip.h's PECLR_AUG_DRAW_* bits."""
        f = self.flags
        return ((_capi.AUG_DRAW_ROTATE if f.get("rotate") else 0) | (_capi.AUG_DRAW_CROP if f.get("crop") else 0)
                | (_capi.AUG_DRAW_RANDOM_CROP if f.get("random_crop") else 0) | (_capi.AUG_DRAW_RESIZE if f.get("resize") else 0)
                | (_capi.AUG_DRAW_COLOR_JITTER if f.get("color_jitter") else 0))

    def draw_ranges(self) -> List[float]:
        """include/peclr_hip.h's `ranges`: the arguments of `sample_view`'s uniform(a, b) calls, in its order."""
        p = self.params
        return [float(x) for x in (p["max_angle"], p["min_angle"], *p["crop_margin_range"][:2], p["crop_margin"],
                                   p["crop_box_jitter"][1], *p["hue_factor_range"][:2], *p["sat_factor_range"][:2],
                                   *p["value_factor_alpha_range"][:2], *p["value_factor_beta_range"][:2])]

    def draw_state(self, device) -> Tuple[Tensor, Tensor]:
        """(call, counters) of `device`: the int64 [1] call counter and the int32 [2] (empty windows, ticket) the draw launch
        advances.  Allocated and zeroed on first use, which must not happen inside a graph capture."""
        device = torch.device(device)
        if device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
        if device not in self._draw_state:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TwoViewAugmenter: the device draw state is allocated on first use; call the augmenter (or "
                                   "draw_state(device)) once before capturing it into a graph")
            self._draw_state[device] = _capi.augment_draw_state(device)
        return self._draw_state[device]

    def bad_windows(self) -> int:
        """How many samples of all device-drawn batches so far had an EMPTY crop window in one of their views (the host path
        raises ValueError for such a sample; the device clamps the window to one pixel inside the image).  This is the one
        call here that SYNCHRONISES with the device: ask at the end of an epoch, not every step."""
        return sum(int(counters[0].item()) for _, counters in self._draw_state.values())

    def draw_batch(self, joints: Tensor, image_hw=None, geom: Optional[Tensor] = None, mirror: Optional[Tensor] = None,
                   return_uniforms: bool = False):
        """The ONE launch of the device draws, for both views of a batch: joints [B,21,3] float32 / float64 on the device;
        image_hw = (H, W) of every sample, or geom, the DEVICE [B,5] int64 table of a mixed-size batch; mirror: None or the
        device int32 [B] left-hand table.  Advances this device's call counter.  No host synchronisation.
        -> `_capi.augment_draw_views`'s (params [2,B,16], scalars [2,6,B], jitter [2,2,B], uniforms [2,B,8] or None)."""
        call, counters = self.draw_state(joints.device)
        return _capi.augment_draw_views(joints, image_hw, geom, mirror, self.draw_flags(), self.draw_ranges(), self.draw_seed,
                                        call, counters, 2, return_uniforms)

    @staticmethod
    def _check_device_left(is_left, b: int):
        """is_left of a device-drawn batch, checked on the host: a device tensor (never read here) by shape and dtype, anything
        else by `check_is_left`.  -> (the device tensor or None, the list of bools or None)."""
        if isinstance(is_left, Tensor) and is_left.is_cuda:
            if is_left.dim() != 1 or is_left.shape[0] != b:
                raise ValueError(f"is_left: expected {b} entries, one per sample, got shape {tuple(is_left.shape)}")
            if is_left.dtype.is_floating_point or is_left.dtype.is_complex:
                raise TypeError(f"is_left: expected bools or integers 0 / 1, got {is_left.dtype}")
            return is_left, None
        return None, check_is_left(is_left, b)

    @staticmethod
    def _device_left(on_device: Optional[Tensor], left: Optional[List[bool]], sizes: Sequence[Tuple[int, int]], dev):
        """`_check_device_left`'s result -> (mirror int32 [B] on the device or None, the dict's bool [B] entry or None)."""
        if on_device is not None:
            flag = on_device if on_device.dtype == torch.bool else on_device != 0
            return flag.to(torch.int32), flag
        if left is None:
            return None, None
        mirror = mirror_table(left, sizes)
        return (None if mirror is None else mirror.to(dev, non_blocking=True),
                torch.tensor(left, dtype=torch.bool).to(dev, non_blocking=True))

    def _call_device(self, images, joints25d, is_left, return_uniforms: bool) -> Dict[str, Tensor]:
        """`__call__` with the draws on the device.  Everything that can be refused is refused before the first device call."""
        ragged = not isinstance(images, Tensor)
        if ragged:
            sizes = images.sizes if isinstance(images, RaggedImages) else RaggedImages.check(images)
            b = len(sizes)
        else:
            if not images.is_cuda or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
                raise _capi.PeclrHipError(f"augment: images must be a [B,H,W,3] uint8 HIP tensor, got {images.dtype} "
                                          f"{tuple(images.shape)} on {images.device} (peclr_amd has no CPU path)")
            b, h, w, _ = images.shape
            sizes = [(h, w)] * b
        joints = joints25d if isinstance(joints25d, Tensor) else torch.as_tensor(np.asarray(joints25d))
        if joints.dim() != 3 or tuple(joints.shape[1:]) != (21, 3) or joints.shape[0] != b:
            raise ValueError(f"joints25d: expected [{b},21,3] for {b} images, got {tuple(joints.shape)}")
        if joints.dtype not in (torch.float32, torch.float64):
            joints = joints.to(torch.float32)
        left_checked = self._check_device_left(is_left, b)
        if ragged and not isinstance(images, RaggedImages):
            dev = next((im.device for im in images if isinstance(im, Tensor) and im.is_cuda), torch.device("cuda"))
            images = RaggedImages.from_list(images, dev)
        dev = images.device
        self.draw_state(dev)
        mirror, left = self._device_left(*left_checked, sizes, dev)
        lr = {} if mirror is None else {"mirror": mirror}
        joints = joints.detach().to(dev, non_blocking=True).contiguous()
        rw, rh = self.params["resize_shape"]
        if not ragged:
            params, scalars, jitter, uniforms = self.draw_batch(joints, (h, w), None, mirror, return_uniforms)
            out, _ = _capi.augment_views(images, params, (rh, rw), IMAGENET_MEAN, IMAGENET_STD, self.channels_last, **lr)
        else:
            geom, wins = self.ragged_slot_tables(sizes, images.offsets, int(images.data.numel()))
            params, scalars, jitter, uniforms = self.draw_batch(joints, None, geom.to(dev, non_blocking=True), mirror,
                                                                return_uniforms)
            out = _capi.augment_views_ragged(images.data, geom, wins, params, (rh, rw), IMAGENET_MEAN, IMAGENET_STD,
                                             self.channels_last, **lr)[0]
        batch = {"transformed_images": out, "transformed_image1": out[:b], "transformed_image2": out[b:]}
        if (dev, b) not in self._blur_false:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TwoViewAugmenter: call once with this batch size before capturing it into a graph")
            self._blur_false[(dev, b)] = torch.zeros(b, device=dev, dtype=torch.bool)
        f = self.flags
        for v in (0, 1):
            entries = {"angle": scalars[v, 0] if f.get("rotate") else None, "jitter_x": jitter[v, 0], "jitter_y": jitter[v, 1]}
            if f.get("color_jitter"):
                entries.update(h=scalars[v, 2], s=scalars[v, 3], a=scalars[v, 4], b=scalars[v, 5])
            entries.update(blur_flag=self._blur_false[(dev, b)], crop_margin_scale=scalars[v, 1])
            batch.update({f"{k}_{v + 1}": t for k, t in entries.items() if t is not None})  # `collate` drops them too
        if left is not None:
            batch["is_left"] = left
        if uniforms is not None:  # what makes the draws checkable: the uniforms and the records the pixel stages read
            batch["params"], batch["uniforms"] = params, uniforms
        return batch

    @staticmethod
    def ragged_slot_tables(sizes: Sequence[Tuple[int, int]], offsets: Tensor, total: int) -> Tuple[Tensor, Tensor]:
        """`ragged_tables` when the windows are not known on the host (device draws): view v of sample i gets a slot the size
        of its whole image at byte v * total + offset_i, row stride W_i -- so the tables depend on the sizes alone and the
        window, wherever the draw puts it, fits.  The scratch is V * total bytes, the warp's grid the largest image's."""
        geom = torch.tensor([[off, h, w, *blur_ksize((h, w))] for off, (h, w) in zip(offsets.tolist(), sizes)],
                            dtype=torch.int64)
        wins = torch.tensor([[[v * total + off, w, w, h] for off, (h, w) in zip(offsets.tolist(), sizes)] for v in (0, 1)],
                            dtype=torch.int64)
        return geom, wins

    # ---- device: the batch
    def __call__(self, images: Union[Tensor, RaggedImages, Sequence], joints25d: Tensor, is_left=None,
                 return_uniforms: bool = False) -> Dict[str, Tensor]:
        """images: [B,H,W,3] uint8 on the HIP device (the reference's RGB HWC arrays, one size per
        batch), or -- for a batch whose images differ in size -- a `RaggedImages`, or a list / tuple of HWC uint8
        arrays (packed and copied here); joints25d: [B,21,3] (any device; the parameter logic runs on the host).
        is_left: None, or B bools (or integers 0 / 1): a flagged sample comes out as the reference loader's
        (cv2.flip(img, 1), x <- W - x) would -- its image as stored, read mirrored on the device, its joints in the stored
        image's coordinates (`sample_batch` has the rule).  The dict then also holds `is_left` (bool [B], device).  None or
        all false launches exactly what a call without it launches.
        With device_draws=True the joints are read on the device (a CPU tensor is uploaded), `is_left` may be a device bool /
        integer [B] tensor, which is then never read on the host; with return_uniforms=True the dict also holds `uniforms`
        (float64 [2,B,8]: angle, margin, jitter x, jitter y, h, s, a, b) and `params` (float64 [2,B,16], the records the
        pixel stages read)."""
        if self.device_draws:
            return self._call_device(images, joints25d, is_left, return_uniforms)
        if return_uniforms:
            raise ValueError("return_uniforms needs device_draws=True: the host draws come from rng")
        if not isinstance(images, Tensor):
            return self._call_ragged(images, joints25d, is_left)
        b, h, w, _ = images.shape
        left = check_is_left(is_left, b)
        params, views = self.sample_batch(joints25d, (h, w), left)
        mirror = mirror_table(left, [(h, w)] * b)
        lr = {} if mirror is None else {"mirror": mirror.to(images.device, non_blocking=True)}
        rw, rh = self.params["resize_shape"]
        call = self.noise_call
        self.noise_call += 1
        ops = 0
        for vs in views:
            for view in vs:
                ops |= self.ext_flags(view)
        if not ops:  # none of the five drawn anywhere in the batch: exactly the recipe's two launches
            out, _ = _capi.augment_views(images, params.to(images.device, non_blocking=True), (rh, rw), IMAGENET_MEAN,
                                         IMAGENET_STD, self.channels_last, **lr)
        else:
            if ops & EXT_BLUR and max(blur_ksize((h, w))) > MAX_BLUR_KSIZE:
                raise ValueError(f"gaussian_blur: a {h}x{w} image needs kernels {blur_ksize((h, w))}, "
                                 f"longer than the device's {MAX_BLUR_KSIZE}")
            ext, coefs = self.pack_ext(views)
            table, n_table = self.noise_table()
            dev = images.device
            out = _capi.augment_views_ext(images, params.to(dev, non_blocking=True), ext.to(dev, non_blocking=True),
                                          coefs.to(dev, non_blocking=True), blur_ksize((h, w)),
                                          table.to(dev, non_blocking=True), n_table, self.noise_seed, call, ops,
                                          (rh, rw), IMAGENET_MEAN, IMAGENET_STD, self.channels_last, **lr)[0]
        # both views are the halves of ONE buffer; `transformed_images` lets the model skip its cat(view1, view2)
        # (hybrid2_model.py:30-32) -- an extra "image" entry, which the reference's consumers of the dict ignore
        batch = {"transformed_images": out, "transformed_image1": out[:b], "transformed_image2": out[b:]}
        batch.update({k: t.to(images.device, non_blocking=True) for k, t in self.collate(views).items()})
        if left is not None:
            batch["is_left"] = torch.tensor(left, dtype=torch.bool).to(images.device, non_blocking=True)
        return batch
