"""Supervised samples on the device: one augmented view together with the labels that went through the same transformation.

Mirrors `Data_Set.prepare_supervised_sample` (reference src/data_loader/data_set.py:278-329) for a batch -- the sample that
`evaluation_utils.evaluate()` and any fine-tuning consume -- split as peclr_amd/augment.py splits the two-view sample:

  host    the PARAMETER side of one view per sample, drawn by `TwoViewAugmenter.sample_view(..., always_crop=False)` in the
          reference's draw order (the supervised mode crops only with the `crop` flag), and the 3 x 3 matrix `T` of
          `SampleAugmenter.transform_sample`, built in float64 in the reference's order: [rot; 0 0 1], minus the crop
          origin, rows times the resize factors.
  device  the PIXEL side: the launches of csrc/augment.hip with one view;
          the LABEL side: ONE launch of csrc/labels.hip (`peclr_supervised_labels`) for the 2.5D joints under `T`, the camera
          matrix `T @ K`, the bone scale, the 3D joints re-created from the 2.5D ones, and `T` as float32.

The conversions themselves are also here as batched functions of HIP tensors: `joints3d_to_25d` (convert_to_2_5D),
`joints25d_to_3d` (convert_2_5D_to_3D) and `root_depth` (get_root_depth), one launch each.  Each stage is evaluated in
float64 from float32 inputs and rounded once (csrc/labels.hip).

Left hands (`is_left`): a left sample is BY DEFINITION the sample (img[:, ::-1], float32(F K M), joints3d with X negated,
joints_raw with X negated) put through the path above -- the right hand that the mirrored camera sees in the mirrored scene,
`HandPosePredictor(is_left=...)`'s convention, so that a model trained on such batches and the predictor agree on what a left
hand looks like.  `mirror_camera` forms those values on the host (the draws read them); on the device the image is read
mirrored in place and the label kernel forms the same values itself (`peclr_supervised_labels_mirror`).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _capi
from .augment import IMAGENET_MEAN, IMAGENET_STD, RaggedImages, TwoViewAugmenter, blur_ksize, check_is_left, convert_to_2_5d, \
    mirror_table

NUM_JOINTS = 21


def joints3d_to_25d(K: Tensor, joints3d: Tensor) -> Tuple[Tensor, Tensor]:
    """The batched convert_to_2_5D: K [B,3,3], joints3d [B,21,3] float32 HIP tensors -> (joints25d [B,21,3], scale [B]).
    One launch, no host synchronisation.  A CPU tensor raises PeclrHipError."""
    return _capi.joints3d_to_25d(K, joints3d)


def joints25d_to_3d(joints25d: Tensor, scale: Tensor, K: Tensor, z_root_calc: Optional[Tensor] = None) -> Tensor:
    """The batched convert_2_5D_to_3D(joints25d, scale, K, is_batch=True, Z_root_calc=z_root_calc): float32 HIP tensors
    [B,21,3], [B], [B,3,3] (and [B]) -> joints3d [B,21,3].  One launch, no host synchronisation."""
    return _capi.joints25d_to_3d(joints25d, scale, K, z_root_calc)[0]


def root_depth(joints25d: Tensor, K: Tensor) -> Tensor:
    """The batched get_root_depth: the scale-normalised root depth [B] of arXiv:1804.09534 eq. 6-7, with the reference's two
    clamp(min=1e-6).  (The conversion launch with a unit scale: its 3D output is dropped.)"""
    b = _capi._label_batch(joints25d, "root_depth")
    return _capi.joints25d_to_3d(joints25d, torch.ones((b,), device=joints25d.device, dtype=torch.float32), K)[1]


def mirror_camera(K, joints3d, width) -> Tuple[Tensor, Tensor]:
    """The labels of a left hand as the right hand of the mirrored image: K [...,3,3], joints3d [...,21,3] (tensors or arrays,
    read as float32) and the image width (one integer, or one per leading index) -> (float32(F K M), joints3d with X negated),
    float32 host tensors.  F: u -> (W - 1) - u, M = diag(-1, 1, 1); by the rule of csrc/predict.hip and csrc/labels.hip: row 0
    <- (W - 1) row 2 - row 0, then column 0 negated, in float64 (the product is exact: an integer below 2^24 times a 24-bit
    significand), rounded to float32 once.  Any [...,21,3] tensor (joints_raw) mirrors the same way."""
    k = torch.as_tensor(K).detach().to("cpu", torch.float32).to(torch.float64)
    j = torch.as_tensor(joints3d).detach().to("cpu", torch.float32).clone()
    w1 = torch.as_tensor(width).to("cpu", torch.float64) - 1.0
    kf = k.clone()
    kf[..., 0, :] = w1[..., None] * k[..., 2, :] - k[..., 0, :]
    kf[..., :, 0] = -kf[..., :, 0]
    j[..., 0] = -j[..., 0]
    return kf.to(torch.float32), j


def transformation_matrix(view: Dict, resize_shape: Sequence[int]) -> List[List[float]]:
    """`transform_sample`'s 3 x 3 matrix of one drawn view, float64, in the reference's order of operations (so that it is
    the same matrix to the last bit): [rot; 0 0 1] or the identity, the shift by the crop origin, the rows times the resize
    factors (resize_shape[0] / window width, resize_shape[1] / window height)."""
    rot = view["rot"]
    t = [list(map(float, rot[0])), list(map(float, rot[1])), [0.0, 0.0, 1.0]] if rot is not None else \
        [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    if view["origin"] is not None:
        t[0][2] -= view["origin"][0]
        t[1][2] -= view["origin"][1]
    _, _, cw, ch = view["crop"]
    fw, fh = resize_shape[0] / cw, resize_shape[1] / ch
    t[0] = [v * fw for v in t[0]]
    t[1] = [v * fh for v in t[1]]
    return t


class SupervisedAugmenter:
    def __init__(self, flags: Optional[Dict[str, bool]] = None, params: Optional[Dict] = None, use_palm: bool = False, rng=None,
                 np_rng=None, extended: bool = False, channels_last: bool = True, noise_seed: Optional[int] = None):
        """flags / params / rng / np_rng / extended / noise_seed: as `TwoViewAugmenter`, whose drawing logic this reuses.
        use_palm: the reference's `config.use_palm` -- the wrist becomes the mean of wrist and index MCP, and `joints` and
        `scale` are recomputed from the moved joints with the new camera matrix."""
        self.views = TwoViewAugmenter(flags, params, rng=rng, channels_last=channels_last, extended=extended, np_rng=np_rng,
                                      noise_seed=noise_seed)
        self.flags, self.params = self.views.flags, self.views.params
        self.use_palm = bool(use_palm)
        self.channels_last = channels_last
        self.last_views: Optional[List[Dict]] = None     # the drawn views of the last batch
        self.last_params: Optional[Tensor] = None        # their packed records [1,B,16] float64 (device)
        self.last_T: Optional[Tensor] = None             # their matrices [B,3,3] float64 (host)

    # ---- host
    def sample_batch(self, K: Tensor, joints3d: Tensor, sizes: Sequence[Tuple[int, int]], is_left=None):
        """One view per sample, in the order a dataset iterates -> (params [1,B,16] float64, views, T [B,3,3] float64), host.
        The joints the draws read are the reference's: convert_to_2_5D on the float32 host tensors -- for a left sample on
        `mirror_camera`'s float32 values, so that its draws are those of the flipped sample."""
        k, j = K.detach().to("cpu", torch.float32), joints3d.detach().to("cpu", torch.float32)
        left = check_is_left(is_left, len(sizes))
        views = []
        for i, hw in enumerate(sizes):
            ki, ji = mirror_camera(k[i], j[i], int(hw[1])) if left is not None and left[i] else (k[i], j[i])
            joints25d, _ = convert_to_2_5d(ki, ji)
            views.append(self.views.sample_view(joints25d, (int(hw[0]), int(hw[1])), always_crop=False))
        params = torch.tensor([[self.views.pack(w) for w in views]], dtype=torch.float64)
        T = torch.tensor([transformation_matrix(w, self.params["resize_shape"]) for w in views], dtype=torch.float64)
        return params, views, T

    # ---- device
    def __call__(self, images: Union[Tensor, RaggedImages, Sequence], K: Tensor, joints3d: Tensor,
                 joints_valid: Optional[Tensor] = None, joints_raw: Optional[Tensor] = None, is_left=None) -> Dict[str, Tensor]:
        """images: [B,H,W,3] uint8 on the HIP device, or a `RaggedImages` / a list of HWC uint8 arrays for a batch whose
        images differ in size.  K [B,3,3], joints3d [B,21,3] (and joints_raw [B,21,3], joints_valid [B,21,1]): host tensors
        as a dataset yields them (uploaded here without blocking), or device tensors (the draws then read a host copy,
        which synchronises).  Returns what torch's default collate makes of the reference's per-sample dicts: `image`
        float32 [B,3,S,S], `joints`, `joints3D`, `joints3D_recreated`, `joints_raw` float32 [B,21,3], `K`, `T` float32
        [B,3,3], `scale` float32 [B], `joints_valid` as given or ones [B,21,1] -- all on the device.  One label launch plus
        the pixel launches; everything that can be refused is refused before the first device call.
        is_left: None, or B bools (or integers 0 / 1).  A flagged sample is given as STORED (a left hand, its own K and
        joints) and comes out as the sample (img[:, ::-1], `mirror_camera(K, joints3d, W)`, joints_raw with X negated)
        comes out without the flag, bit for bit: the image is read mirrored on the device, nothing is flipped on the host.
        The dict then also holds `is_left` (bool [B]).  None or all false launches exactly what a call without it launches."""
        ragged = not isinstance(images, Tensor)
        if not ragged:
            if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8:
                raise ValueError(f"images: expected [B,H,W,3] uint8, got {images.dtype} {tuple(images.shape)}")
            if not images.is_cuda:
                raise _capi.PeclrHipError(f"images: expected a HIP device tensor, got {images.device} (peclr_amd has no CPU path)")
            sizes = [(int(images.shape[1]), int(images.shape[2]))] * images.shape[0]
        elif isinstance(images, RaggedImages):
            sizes = images.sizes
        else:
            sizes = RaggedImages.check(images)
        b = len(sizes)
        for t, shape, what in ((K, (b, 3, 3), "K"), (joints3d, (b, NUM_JOINTS, 3), "joints3d"),
                               (joints_raw, (b, NUM_JOINTS, 3), "joints_raw")):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError(f"{what}: expected {list(shape)} for {b} images, got {tuple(t.shape)}")
        if joints_valid is not None and len(joints_valid) != b:
            raise ValueError(f"joints_valid: {len(joints_valid)} entries for {b} images")
        self.views._check_blur_sizes(sizes)
        left = check_is_left(is_left, b)
        params, views, T = self.sample_batch(K, joints3d, sizes, left)     # raises on an empty crop window

        if ragged and not isinstance(images, RaggedImages):
            dev = next((im.device for im in images if isinstance(im, Tensor) and im.is_cuda), torch.device("cuda"))
            images = RaggedImages.from_list(images, dev)
        dev = images.device
        up = lambda t: t.to(dev, torch.float32, non_blocking=True).contiguous()  # noqa: E731
        params_d = params.to(dev, non_blocking=True)
        mirror = mirror_table(left, sizes)     # one table for the label kernel (the widths) and the pixel stages (non-zero)
        lr = {} if mirror is None else {"mirror": mirror.to(dev, non_blocking=True)}  # no left hand: today's calls as they are
        labels = _capi.supervised_labels(up(K), up(joints3d), T.to(dev, non_blocking=True), self.use_palm,
                                         None if joints_raw is None else up(joints_raw),
                                         **({"mirror_w": lr["mirror"]} if lr else {}))
        image = self._pixels(images, sizes, params_d, views, lr)
        self.last_views, self.last_params, self.last_T = views, params_d, T
        if joints_valid is None:
            joints_valid = torch.ones((b, NUM_JOINTS, 1), device=dev)
        return {"image": image, "joints": labels["joints"], "joints3D": labels["joints3D"], "K": labels["K"],
                "scale": labels["scale"], "joints3D_recreated": labels["joints3D_recreated"],
                "joints_valid": joints_valid.to(dev, non_blocking=True), "joints_raw": labels["joints_raw"], "T": labels["T"],
                **({} if left is None else {"is_left": torch.tensor(left, dtype=torch.bool).to(dev, non_blocking=True)})}

    def _pixels(self, images, sizes, params_d: Tensor, views: List[Dict], lr: Optional[Dict] = None) -> Tensor:
        """The existing pixel launches with one view (as `TwoViewAugmenter.__call__` / `_call_ragged` make them).  lr: the
        `mirror=` keyword of a batch with left hands, or empty."""
        tv = self.views
        rw, rh = self.params["resize_shape"]
        dev = params_d.device
        call = tv.noise_call
        tv.noise_call += 1
        ops = 0
        for view in views:
            ops |= tv.ext_flags(view)
        tail = ((rh, rw), IMAGENET_MEAN, IMAGENET_STD, self.channels_last)
        lr = lr or {}
        if ops:
            ext, coefs = tv.pack_ext([views])
            table, n_table = tv.noise_table()
            ext_args = (ext.to(dev, non_blocking=True), coefs.to(dev, non_blocking=True))
            noise_args = (table.to(dev, non_blocking=True), n_table, tv.noise_seed, call, ops)
        if isinstance(images, RaggedImages):
            geom, wins = tv.ragged_tables(sizes, images.offsets, [views])
            if not ops:
                return _capi.augment_views_ragged(images.data, geom, wins, params_d, *tail, **lr)[0]
            return _capi.augment_views_ragged_ext(images.data, geom, wins, params_d, *ext_args, *noise_args, *tail, **lr)[0]
        if not ops:
            return _capi.augment_views(images, params_d, *tail, **lr)[0]
        return _capi.augment_views_ext(images, params_d, *ext_args, blur_ksize(sizes[0]), *noise_args, *tail, **lr)[0]
