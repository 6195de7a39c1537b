"""Two-pass hand-pose prediction on images of any size, with a hand box and a left-hand flag per sample.

`pose.FreiHANDPredictor` is FreiHAND-shaped: one [B,H,W,3] tensor, the fixed centred box of pred_fh.py, right hands, FreiHAND
joints out.  `HandPosePredictor` runs the same two passes (crop -> backbone -> head with the re-crop in its epilogue -> crop ->
backbone -> head) for

- images that differ in size within one batch (a `RaggedImages`, a list of HWC uint8 arrays, or a dense [B,H,W,3] tensor --
  the uniform case of the same kernel), as YouTube-3D-Hands frames or a user's own frames come;
- a hand box per sample in source pixels (a detector's, or the dataset's), instead of the centred default;
- left hands, which the reference mirrors into right hands before the network sees them: the crop kernel reads the image
  mirrored (no flipped copy is made), the camera becomes that of the mirrored image looking at the mirrored scene, and one
  launch after pass 2 takes everything back into the sample's own frame;

and returns the 3D joints in the sample's camera frame and the 2D keypoints in source-image pixels (what
`PoseEvaluator.update_2d` scores).  No host round trip between the passes, one status read at the end, one hipGraph
(`capture` / `replay`).  Kernels: csrc/predict.hip.  The augmenters read left hands the same way (`is_left`; supervised.mirror_camera is `flip_camera`, rounded).

Everything that can be refused is refused on the host before the first device call (`plan`), naming the sample.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _capi
from .augment import RaggedImages
from .pose import BBOX_SCALE, CROP_SIZE, K_DEFAULT, FreiHANDPredictor, RN25DwMLPref, _dev, create_affine_transform_from_bbox, \
    modify_bbox


# ------------------------------------------------------------------ host geometry (float64 NumPy, no device call)
def mirror_box(box, width: int) -> np.ndarray:
    """(x1, y1, x2, y2) in an image of `width` columns -> the same box in img[:, ::-1]: (x1, x2) <- (W-1-x2, W-1-x1)."""
    x1, y1, x2, y2 = (float(v) for v in box)
    return np.array([(width - 1) - x2, y1, (width - 1) - x1, y2], dtype=np.float64)


def flip_camera(K, width: int) -> np.ndarray:
    """Kf = F K M, the camera of the mirrored image looking at the mirrored scene (F: u -> W-1-u, M = diag(-1, 1, 1)), by the
    rule the crop kernel follows: float64, one product and one difference per entry."""
    K = np.asarray(K, dtype=np.float64)
    r = [np.float64(width - 1) * K[2][c] - K[0][c] for c in range(3)]
    return np.array([[-r[0], r[1], r[2]], [-K[1][0], K[1][1], K[1][2]], [-K[2][0], K[2][1], K[2][2]]], dtype=np.float64)


def box_transform(box, crop_size: int = CROP_SIZE, box_scale: float = 1.0) -> np.ndarray:
    """The pass-1 matrix of one sample from its hand box: pose.py's two functions, float64."""
    return create_affine_transform_from_bbox(modify_bbox(np.array(box, dtype=np.float64), box_scale), crop_size)


def default_transform(h: int, w: int, crop_size: int = CROP_SIZE, bbox_scale: float = BBOX_SCALE) -> np.ndarray:
    """Without a box: the centred box of `initial_transform`, on the image's own size (float32 box, as there)."""
    return create_affine_transform_from_bbox(modify_bbox(np.array([0, 0, w, h], dtype=np.float32), bbox_scale), crop_size)


class Plan(NamedTuple):
    """One call's host side: what the device gets, checked."""
    sizes: List[Tuple[int, int]]
    total_bytes: int
    geom: np.ndarray           # int64 [B,4]: byte offset, H, W, flip
    T1: np.ndarray             # float64 [B,3,3], on mirrored-source coordinates for left samples
    K: object                  # float64 [B,3,3] array / tensor, or None (the model's default)
    scale: object              # float64 [B] array / tensor, or None (1.0)


def _host_array(x, what: str) -> np.ndarray:
    if isinstance(x, Tensor):
        if x.is_cuda:
            raise TypeError(f"{what} must be on the host (it decides the crop geometry before any device call), got a tensor on {x.device}")
        x = x.detach().numpy()
    return np.asarray(x)


def _image_sizes(images) -> Tuple[List[Tuple[int, int]], List[int], int]:
    """(sizes, byte offsets, bytes of the buffer the offsets index) of any accepted `images`."""
    if isinstance(images, RaggedImages):
        sizes, offsets, have = images.sizes, [int(o) for o in images.offsets.tolist()], int(images.data.numel())
        if len(sizes) == 0:
            raise ValueError("images: an empty RaggedImages")
    elif isinstance(images, (list, tuple)):
        sizes = RaggedImages.check(images)
        offsets, have = RaggedImages.layout(sizes)
        offsets = offsets.tolist()
    elif isinstance(images, (Tensor, np.ndarray)):
        dtype_ok = images.dtype == (torch.uint8 if isinstance(images, Tensor) else np.uint8)
        if not dtype_ok:
            raise TypeError(f"images: expected uint8 pixels, got {images.dtype}")
        shape = tuple(images.shape)
        if len(shape) != 4 or shape[3] != 3 or min(shape[:3]) < 1:
            raise ValueError(f"images: expected a non-empty [B,H,W,3] tensor, got {shape}")
        b, h, w, _ = shape
        sizes, offsets, have = [(h, w)] * b, [i * h * w * 3 for i in range(b)], b * h * w * 3
    else:
        raise TypeError(f"images: expected a [B,H,W,3] uint8 tensor, a RaggedImages or a list of HWC uint8 arrays, got {type(images).__name__}")
    for i, ((h, w), off) in enumerate(zip(sizes, offsets)):
        if off < 0 or off + h * w * 3 > have:
            raise ValueError(f"sample {i}: image of {h}x{w} at byte {off} ends past the packed buffer of {have} bytes")
    return list(sizes), offsets, have


def _per_sample(x, b: int, tail: Tuple[int, ...], what: str):
    """A [B, *tail] floating array or tensor (host or device) as it is; raises on any other dtype or shape.  No device call."""
    if not isinstance(x, Tensor):
        x = np.asarray(x)
        floating = x.dtype.kind == "f"
    else:
        floating = x.dtype.is_floating_point
    if not floating:
        raise TypeError(f"{what}: expected floating point values, got {x.dtype}")
    if tuple(x.shape) != (b, *tail):
        raise ValueError(f"{what}: expected {[b, *tail]} for {b} images, got {list(x.shape)}")
    return x


def plan(images, K=None, scale=None, boxes=None, is_left=None, crop_size: int = CROP_SIZE, bbox_scale: float = BBOX_SCALE,
         box_scale: float = 1.0) -> Plan:
    """Check one call's arguments and lay out its geometry, on the host alone.  Raises TypeError / ValueError naming the
    sample: wrong dtypes or shapes, lengths that disagree, a non-finite or empty box, an image that ends past its buffer."""
    sizes, offsets, total = _image_sizes(images)
    b = len(sizes)
    if K is not None:
        K = _per_sample(K, b, (3, 3), "K")
    if scale is not None:
        scale = _per_sample(scale, b, (), "scale")
    left = np.zeros(b, dtype=bool)
    if is_left is not None:
        left = _host_array(is_left, "is_left")
        if left.dtype != np.bool_:
            raise TypeError(f"is_left: expected bool, got {left.dtype}")
        if left.shape != (b,):
            raise ValueError(f"is_left: expected [{b}] for {b} images, got {list(left.shape)}")
    if boxes is not None:
        boxes = _host_array(boxes, "boxes")
        if boxes.dtype.kind not in "fiu":
            raise TypeError(f"boxes: expected real numbers (x1, y1, x2, y2), got {boxes.dtype}")
        if boxes.shape != (b, 4):
            raise ValueError(f"boxes: expected [{b}, 4] for {b} images, got {list(boxes.shape)}")
        boxes = boxes.astype(np.float64)
        for i, (x1, y1, x2, y2) in enumerate(boxes):
            if not np.isfinite(boxes[i]).all():
                raise ValueError(f"sample {i}: box {boxes[i].tolist()} is not finite")
            if x2 <= x1 or y2 <= y1:
                raise ValueError(f"sample {i}: box {boxes[i].tolist()} is empty (x2 <= x1 or y2 <= y1)")
    T1 = np.empty((b, 3, 3), dtype=np.float64)
    centred = {}                # size -> matrix: a batch of one size pays for one (the host is on the critical path of a call)
    for i, (h, w) in enumerate(sizes):
        if boxes is None:       # (the centred box is its own mirror image)
            if (h, w) not in centred:
                centred[(h, w)] = default_transform(h, w, crop_size, bbox_scale)
            T1[i] = centred[(h, w)]
        else:
            T1[i] = box_transform(mirror_box(boxes[i], w) if left[i] else boxes[i], crop_size, box_scale)
    geom = np.array([[off, h, w, int(f)] for off, (h, w), f in zip(offsets, sizes, left)], dtype=np.int64).reshape(b, 4)
    return Plan(sizes, total, geom, T1, K, scale)


def check_replay(p: Plan, batch: int, max_bytes: int) -> None:
    """What a captured graph cannot take: another batch length, or images that need more than its static buffer."""
    if len(p.sizes) != batch:
        raise ValueError(f"replay: captured for {batch} images, got {len(p.sizes)}")
    if p.total_bytes > max_bytes:
        raise ValueError(f"replay: captured for images of at most {max_bytes} bytes in all, these need {p.total_bytes}")


class _Batch(NamedTuple):
    """One call's device side."""
    data: Tensor      # 1-D uint8: the images back to back
    geom: Tensor      # int64 [B,4]
    T1: Tensor        # float64 [B,3,3]


# ------------------------------------------------------------------ the predictor
class HandPosePredictor(FreiHANDPredictor):
    """predict(images, K=None, scale=None, boxes=None, is_left=None) -> {"xyz": float64 [B,21,3] FreiHAND joint order, times
    `scale` (scale-normalised without one), "kp3d": float32 [B,21,3] model joint order, both in the sample's own camera frame;
    "kp2d": float64 [B,21,2] model joint order, source-image pixels}, HIP tensors.

    images: [B,H,W,3] uint8 tensor, `RaggedImages`, or a list / tuple of HWC uint8 arrays (packed by `RaggedImages.from_list`).
    K: [B,3,3] or None (the model's `K_default`); scale: [B] or None (1.0); is_left: [B] bool or None; boxes: [B,4] (x1, y1, x2,
    y2) in ORIGINAL source pixels or None (the centred box of `initial_transform` on each image's own size).  A left sample's
    box is mirrored on the host, its image read mirrored by the crop kernel; T1 / T2 of such a sample act on mirrored-source
    coordinates.  `last` keeps pass1, pass2, T1, T2, K1, K2, geom of the latest call.
    precision / fold_bn: as `FreiHANDPredictor` (this class runs its `_passes`)."""

    def __init__(self, model: RN25DwMLPref, crop_size: int = CROP_SIZE, bbox_scale: float = BBOX_SCALE, box_scale: float = 1.0,
                 precision="fp32", fold_bn=None):
        super().__init__(model, crop_size, bbox_scale, precision, fold_bn)
        self.bbox_scale, self.box_scale = bbox_scale, box_scale
        self._max_bytes = 0

    def plan(self, images, K=None, scale=None, boxes=None, is_left=None) -> Plan:
        return plan(images, K, scale, boxes, is_left, self.size, self.bbox_scale, self.box_scale)

    # ---- device side
    def _two_passes(self, batch: _Batch, K: Tensor, scale: Tensor):
        m = self.model
        if m.training or not m.backend_model.bn1.hip:
            raise _capi.PeclrHipError("HandPosePredictor: the model must be in eval mode with the HIP kernels on (enable_hip())")
        data, geom, T1 = batch
        b = geom.shape[0]
        with torch.no_grad():
            x1, k1 = _capi.pose_crop_ragged(data, geom, T1, K, self._table, self.size)
            out1, T2, _, status = m._head_hip(m.features(x1), k1, T1=T1, size=self.size)
            x2, k2 = _capi.pose_crop_ragged(data, geom, T2, K, self._table, self.size)
            out2, _, fh, status = m._head_hip(m.features(x2), k2, scale=scale, status=status)
            out64 = out2["kp25d"].as_strided((b, 64), (64, 1))     # the head's [B,64] output: kp25d views its first 63 columns
            kp2d, kp3d, xyz = _capi.pose_unmap(out64, T2, geom, out2["kp3d"], fh)
        self.last = {"pass1": out1, "pass2": out2, "T1": T1, "T2": T2, "K1": k1, "K2": k2, "geom": geom}
        return {"xyz": xyz, "kp3d": kp3d, "kp2d": kp2d}, status

    def _data(self, images) -> Tensor:
        if isinstance(images, (list, tuple)):
            images = RaggedImages.from_list(images, self.device)
        if isinstance(images, RaggedImages):
            return images.data if images.data.device == self.device else images.data.to(self.device, non_blocking=True)
        return _dev(images, self.device, torch.uint8).reshape(-1)

    def _camera(self, p: Plan):
        b = len(p.sizes)
        K = (self.model.K_default.to(torch.float64).expand(b, 3, 3).contiguous() if p.K is None
             else _dev(p.K, self.device, torch.float64))
        scale = (torch.ones((b,), dtype=torch.float64, device=self.device) if p.scale is None
                 else _dev(p.scale, self.device, torch.float64))
        return K, scale

    def predict(self, images, K=None, scale=None, boxes=None, is_left=None) -> Dict[str, Tensor]:
        p = self.plan(images, K, scale, boxes, is_left)            # every refusal: before the first device call
        batch = _Batch(self._data(images), _dev(p.geom, self.device, torch.int64), _dev(p.T1, self.device, torch.float64))
        out, status = self._passes(batch, *self._camera(p))
        self._raise_on_status(status)
        return out

    # ---- one hipGraph
    def capture(self, batch: int, max_bytes: int) -> "HandPosePredictor":
        """Record the whole call for `batch` images of at most `max_bytes` in all as one hipGraph over static buffers -- the packed
        image buffer, geom, T1, K, scale (after one eager call, which creates the weight planes and warms the allocator).  The
        kernels find every image through geom, so the unused tail of the image buffer is never read."""
        batch, max_bytes = int(batch), int(max_bytes)
        if batch < 1 or max_bytes < 3 * batch:
            raise ValueError(f"capture: needs batch >= 1 and max_bytes >= 3 * batch, got {batch} and {max_bytes}")
        dev = self.device
        geom = np.array([[3 * i, 1, 1, 0] for i in range(batch)], dtype=np.int64)      # until the first replay: 1 x 1 images
        T1 = np.stack([default_transform(1, 1, self.size, self.bbox_scale)] * batch)
        self._static = (_Batch(torch.zeros((max_bytes,), dtype=torch.uint8, device=dev), torch.from_numpy(geom).to(dev),
                               torch.from_numpy(T1).to(dev)),
                        torch.from_numpy(np.array(K_DEFAULT)).expand(batch, 3, 3).contiguous().to(dev),
                        torch.ones((batch,), dtype=torch.float64, device=dev))
        self._passes(*self._static)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._static_out = self._passes(*self._static)
        self._graph_last = self.last
        self._graph, self._batch, self._max_bytes = g, batch, max_bytes
        return self

    def replay(self, images, K=None, scale=None, boxes=None, is_left=None) -> Dict[str, Tensor]:
        if self._graph is None:
            raise RuntimeError("HandPosePredictor.replay: call capture(batch, max_bytes) first")
        p = self.plan(images, K, scale, boxes, is_left)
        check_replay(p, self._batch, self._max_bytes)              # ... and these two: before any device call as well
        data = self._data(images)
        sb, sk, ss = self._static
        sb.data[:data.numel()].copy_(data, non_blocking=True)
        sb.geom.copy_(_dev(p.geom, self.device, torch.int64), non_blocking=True)
        sb.T1.copy_(_dev(p.T1, self.device, torch.float64), non_blocking=True)
        K, scale = self._camera(p)
        sk.copy_(K)
        ss.copy_(scale)
        self._graph.replay()
        self.last = self._graph_last
        out, status = self._static_out
        self._raise_on_status(status)
        return {k: v.clone() for k, v in out.items()}
