"""The fine-tuned 2.5D hand-pose model and batched FreiHAND prediction.

Restates the reference's downstream half: `RN_25D_wMLPref` / `ZrootMLP_ref` (src/models/rn_25D_wMLPref.py), the
helpers of testing/fh_utils.py and the two-pass crop -> predict -> re-crop loop of testing/pred_fh.py.  The state_dict
is the reference's, key for key and in its order (`backend_model.<torchvision keys>`, then `zroot_ref.zroot_ref.*`), so
the published `rn{50,152}_peclr_yt3d-fh_pt_fh_ft.pth` files load unchanged.

Three paths:
- stock (CPU, HIP BatchNorm off, train mode or grad enabled): plain torch ops in the reference's order;
- HIP training (train mode after `enable_hip_training()`, a HIP tensor, HIP BatchNorm on): the backbone on the in-tree
  kernels and the head, forward and backward, on `peclr_pose_head_train_{fwd,bwd}_f32` (`PoseHeadTrain`);
- HIP (eval, a HIP tensor, `enable_hip()` / `enable_hip_batchnorm(model.backend_model)`, no grad): the backbone's last
  BatchNorm also average-pools, and one `peclr_pose_head_f32` launch takes the pooled features to every output.

`FreiHANDPredictor` runs both passes for a whole batch on the device (crop kernel, backbone, head with the re-crop in
its epilogue, crop, backbone, head with the submission joints in its epilogue) without a host synchronisation before
the single status check at the end, and can record them as one hipGraph.
"""
from __future__ import annotations

import json
import os
import zipfile
from typing import Dict, Optional

import numpy as np
import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

import contextlib

from . import _capi
from . import bn2d as _bn2d
from . import resnet as _resnet
from .bn2d import FusedBatchNormAct2d, enable_hip_batchnorm
from .encoder import TailAvgPool

NUM_JOINTS = 21
CROP_SIZE = 224
BBOX_SCALE = 0.33
IMAGE_MEAN = (0.485, 0.456, 0.406)
IMAGE_STD = (0.229, 0.224, 0.225)
# the reference's default camera (rn_25D_wMLPref.py): used when forward() gets no K
K_DEFAULT = ((388.9018310596544, 0.0, 112.0), (0.0, 388.71231836584275, 112.0), (0.0, 0.0, 1.0))
# fh_utils.convert_order: FreiHAND joint i is model joint FH_ORDER[i] (model order: wrist, the five MCPs, PIPs, DIPs, tips)
FH_ORDER = (0, 1, 6, 11, 16, 2, 7, 12, 17, 3, 8, 13, 18, 4, 9, 14, 19, 5, 10, 15, 20)


class ZrootMLPRef(nn.Module):
    """Closed-form scale-normalised root depth (arXiv:1804.09534 Eq. 6/7) refined by an MLP (arXiv:2003.09282)."""

    norm_bone_idx = (3, 8)
    eps_value = 1e-8   # the `eps` buffer's value, for the HIP head (read without a device round trip)

    def __init__(self):
        super().__init__()
        self.zroot_ref = nn.Sequential(nn.Linear(64, 128), nn.BatchNorm1d(128), nn.LeakyReLU(),
                                       nn.Linear(128, 128), nn.BatchNorm1d(128), nn.LeakyReLU(), nn.Linear(128, 1))
        self.register_buffer("eps", torch.tensor(self.eps_value), persistent=False)

    def forward(self, kp3d_unnorm: Tensor, zrel: Tensor, K: Optional[Tensor] = None) -> Tensor:
        m, n = self.norm_bone_idx
        xm, ym = kp3d_unnorm[:, m:m + 1, 0:1], kp3d_unnorm[:, m:m + 1, 1:2]
        xn, yn = kp3d_unnorm[:, n:n + 1, 0:1], kp3d_unnorm[:, n:n + 1, 1:2]
        zm, zn = zrel[:, m:m + 1], zrel[:, n:n + 1]
        a = (xn - xm) ** 2 + (yn - ym) ** 2
        b = 2 * (zn * (xn ** 2 + yn ** 2 - xn * xm - yn * ym) + zm * (xm ** 2 + ym ** 2 - xn * xm - yn * ym))
        c = (xn * zn - xm * zm) ** 2 + (yn * zn - ym * zm) ** 2 + (zn - zm) ** 2 - 1
        d = b ** 2 - 4 * a * c
        a = torch.max(self.eps, a)       # (NaN propagates)
        d = torch.max(self.eps, d)
        zroot = ((-b + torch.sqrt(d)) / (2 * a)).detach()
        zroot = torch.clamp(zroot, 4.0, 50.0)
        mlp_in = torch.cat((zrel.reshape(-1, 21), kp3d_unnorm[..., :2].reshape(-1, 42), zroot.reshape(-1, 1)), dim=1)
        return zroot + self.zroot_ref(mlp_in).reshape(zroot.shape)


class PoseHeadTrain(torch.autograd.Function):
    """The head in train mode on the HIP kernels (csrc/pose_train.hip): four launches forward, six backward (five when the
    features need no gradient), every reduction in a fixed order.

    apply(feat [B,2048], K [B or 1,3,3], fc_w, fc_b, *the 14 MLP tensors of `peclr_pose_head_f32`, nbt1, nbt2, bn_eps (2),
    momentum (2), eps) -> (out64 [B,64], kp3d [B,21,3], zroot [B]); kp25d = out64[:, :63].  The running statistics and the two
    num_batches_tracked are updated in place.  Differentiable once with respect to the features, fc and the ten MLP
    parameters; K gets no gradient."""

    @staticmethod
    def forward(ctx, feat, K, fc_w, fc_b, *rest):
        mlp, (nbt1, nbt2, bn_eps, momentum, eps) = list(rest[:_capi.POSE_MLP_TENSORS]), rest[_capi.POSE_MLP_TENSORS:]
        feat, K = feat.contiguous(), K.float().contiguous()
        out64, kp3d, zroot, save = _capi.pose_head_train_fwd(feat, fc_w, fc_b, mlp, bn_eps, momentum, (nbt1, nbt2), K, eps)
        ctx.save_for_backward(feat, K, fc_w, out64, zroot, save, *mlp)
        ctx.set_materialize_grads(False)
        return out64, kp3d, zroot

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out64, g_kp3d, g_zroot):
        feat, K, fc_w, out64, zroot, save, *mlp = ctx.saved_tensors
        g_out64, g_kp3d, g_zroot = (None if g is None else g.float().contiguous() for g in (g_out64, g_kp3d, g_zroot))
        d_feat, d_fc_w, d_fc_b, d_mlp, _ = _capi.pose_head_train_bwd(feat, fc_w, mlp, K, out64, zroot, save, g_kp3d, g_out64, g_zroot,
                                                                     want_d_feat=ctx.needs_input_grad[0])
        grads = [None] * _capi.POSE_MLP_TENSORS
        for i, g in zip(_capi._POSE_MLP_GRAD_OF, d_mlp):
            grads[i] = g
        return (d_feat, None, d_fc_w, d_fc_b, *grads, None, None, None, None, None)


def _backbone(name: str) -> _resnet.ResNet:
    model = {"rn50": _resnet.resnet50, "rn152": _resnet.resnet152}[name](norm_layer=FusedBatchNormAct2d)
    model.fc = nn.Linear(model.fc.in_features, 3 * NUM_JOINTS + 1)   # 2D + zrel for 21 joints (+1 unused)
    # In HIP mode the stem BatchNorm also does the ReLU + max pool, and the last block's final BatchNorm the average pool
    # (fp32 [N, C] out, as encoder.ResNetModel arranges it); the modules they replace have no parameters: keys unchanged.
    model.bn1.default_pool = True
    model.maxpool = nn.Identity()
    model.layer4[-1].bn3.tail_avgpool = True
    model.avgpool = TailAvgPool()
    return model


class RN25DwMLPref(nn.Module):
    """ResNet-50 / 152 predicting 2D keypoints and relative depth of 21 joints, lifted to 3D with the camera matrix."""

    def __init__(self, backend_model: str = "rn50"):
        super().__init__()
        if backend_model not in ("rn50", "rn152"):
            raise ValueError(f"Unknown backend_model: {backend_model}")
        self.backend_type = backend_model
        self.backend_model = _backbone(backend_model)
        self.zroot_ref = ZrootMLPRef()
        self.register_buffer("K_default", torch.tensor(K_DEFAULT, dtype=torch.float32).reshape(1, 3, 3), persistent=False)
        self.hip_training = False

    # ---- paths
    def enable_hip(self, enabled: bool = True) -> "RN25DwMLPref":
        """channels_last backbone weights and the HIP BatchNorm / convolution kernels (call after .to(device))."""
        if enabled:
            self.backend_model.to(memory_format=torch.channels_last)
        enable_hip_batchnorm(self.backend_model, enabled)
        return self

    def enable_hip_training(self, enabled: bool = True) -> "RN25DwMLPref":
        """Opt in: in train mode, on a HIP tensor and with the HIP BatchNorm on, `head()` and `forward()` run the head on the
        training kernels (`PoseHeadTrain`) and return `zroot` [B], the refined root depth, next to the four usual keys.
        Without it train mode stays on stock torch ops.  Call after .to(device)."""
        if enabled:
            if not self.backend_model.fc.weight.is_cuda:
                raise _capi.PeclrHipError("enable_hip_training: the model must be on a HIP device (peclr_amd has no CPU path)")
            self._check_hip_training()
        self.hip_training = bool(enabled)
        return self

    def _check_hip_training(self):
        for bn in (self.zroot_ref.zroot_ref[1], self.zroot_ref.zroot_ref[4]):
            if bn.momentum is None or not bn.track_running_stats:
                raise _capi.PeclrHipError("the HIP training head needs BatchNorm1d with a numeric momentum and "
                                          "track_running_stats=True (momentum=None and track_running_stats=False are not supported)")

    def hip_train_path(self, x: Tensor) -> bool:
        return self.hip_training and self.training and x.is_cuda and self.backend_model.bn1.hip

    def hip_path(self, x: Tensor) -> bool:
        return (not self.training and x.is_cuda and not torch.is_grad_enabled() and self.backend_model.bn1.hip
                and self.backend_model.fc.weight.is_cuda)

    def features(self, img: Tensor) -> Tensor:
        """The backbone up to the pooled [B, 2048] features (everything but `fc`).  Under bf16 / fp16 autocast, in eval mode and
        with `bn2d.ROUTING.fold_eval_bn` on, the bottleneck blocks apply their BatchNorm layers in the convolution epilogues
        (`bn2d.fold_plan`): one launch writes all their tables first, once per call."""
        bb = self.backend_model
        if bb.bn1.hip:
            img = img.contiguous(memory_format=torch.channels_last)
        if _bn2d.fold_applies(bb, img):
            with _bn2d.folded_eval_bn(bb):
                return self._features(bb, img)
        return self._features(bb, img)

    @staticmethod
    def _features(bb, img: Tensor) -> Tensor:
        x = _resnet._bn(bb.bn1, _resnet._conv(bb.conv1, img, bb.bn1), relu=True)
        x = bb.layer4(bb.layer3(bb.layer2(bb.layer1(bb.maxpool(x)))))
        return torch.flatten(bb.avgpool(x), 1)

    def _mlp_tensors(self):
        s = self.zroot_ref.zroot_ref
        return [s[0].weight, s[0].bias, s[1].weight, s[1].bias, s[1].running_mean, s[1].running_var,
                s[3].weight, s[3].bias, s[4].weight, s[4].bias, s[4].running_mean, s[4].running_var, s[6].weight, s[6].bias]

    def _head_hip(self, feat: Tensor, K: Tensor, T1=None, size=0, scale=None, status=None):
        s = self.zroot_ref.zroot_ref
        fc = self.backend_model.fc
        K = K.float().contiguous()
        out64, kp3d, T2, fh, status = _capi.pose_head(feat.contiguous(), fc.weight, fc.bias, self._mlp_tensors(), (s[1].eps, s[4].eps),
                                                      K, self.zroot_ref.eps_value, T1=T1, size=size, scale=scale, status=status)
        kp25d = out64[:, :-1].view(-1, NUM_JOINTS, 3)
        out = {"kp3d": kp3d, "zrel": kp25d[..., 2:3], "kp2d": kp25d[..., :2], "kp25d": kp25d}
        return out, T2, fh, status

    def _head_train(self, feat: Tensor, K: Tensor) -> Dict[str, Tensor]:
        self._check_hip_training()
        s = self.zroot_ref.zroot_ref
        fc = self.backend_model.fc
        out64, kp3d, zroot = PoseHeadTrain.apply(feat, K, fc.weight, fc.bias, *self._mlp_tensors(), s[1].num_batches_tracked,
                                                 s[4].num_batches_tracked, (s[1].eps, s[4].eps), (s[1].momentum, s[4].momentum),
                                                 self.zroot_ref.eps_value)
        kp25d = out64[:, :-1].contiguous().view(-1, NUM_JOINTS, 3)      # a copy: `PoseLoss` takes a contiguous prediction
        return {"kp3d": kp3d, "zrel": kp25d[..., 2:3], "kp2d": kp25d[..., :2], "kp25d": kp25d, "zroot": zroot}

    def _head_stock(self, out: Tensor, K: Tensor) -> Dict[str, Tensor]:
        kp25d = out[:, :-1].view(-1, NUM_JOINTS, 3)
        kp2d, zrel = kp25d[..., :2], kp25d[..., 2:3]
        zrel[:, 0] = 0                    # in place: visible in kp25d
        kp2d_h = torch.cat((kp2d, torch.ones((kp2d.shape[0], NUM_JOINTS, 1), device=K.device)), dim=2)
        kp3d_unnorm = torch.matmul(kp2d_h, K.inverse().transpose(1, 2))
        zroot = self.zroot_ref(kp3d_unnorm, zrel, K)
        return {"kp3d": kp3d_unnorm * (zrel + zroot), "zrel": zrel, "kp2d": kp2d, "kp25d": kp25d}

    def head(self, features: Tensor, K: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """Pooled [B, 2048] features -> {"kp3d", "zrel", "kp2d", "kp25d"}."""
        K = self.K_default if K is None else K
        if self.hip_train_path(features):
            return self._head_train(features, K)
        if self.hip_path(features):
            return self._head_hip(features, K)[0]
        return self._head_stock(self.backend_model.fc(features), K)

    def forward(self, img: Tensor, K: Optional[Tensor] = None) -> Dict[str, Tensor]:
        K = self.K_default if K is None else K
        if self.hip_train_path(img):
            return self._head_train(self.features(img), K)
        if self.hip_path(img):
            return self._head_hip(self.features(img), K)[0]
        return self._head_stock(self.backend_model(img), K)


# ------------------------------------------------------------------ testing/fh_utils.py, restated (float64 NumPy)
def modify_bbox(bbox: np.ndarray, scale: float) -> np.ndarray:
    """Square box of side max(w, h) * scale around the box's centre, written into `bbox` (its dtype) and returned."""
    cx, cy = (bbox[0] + bbox[2]) / 2, (bbox[1] + bbox[3]) / 2
    w, h = bbox[2] - bbox[0], bbox[3] - bbox[1]
    w *= scale
    h *= scale
    side = max(h, w)
    bbox[0], bbox[1] = cx - side / 2, cy - side / 2
    bbox[2], bbox[3] = cx + side / 2, cy + side / 2
    return bbox


def create_affine_transform_from_bbox(bbox, crop_size: int) -> np.ndarray:
    """Forward matrix that scales the box's longer side to 0.7 crop_size and moves its centre to the crop's centre."""
    side = float(max(bbox[3] - bbox[1], bbox[2] - bbox[0]))
    s = 0.7 * crop_size / side
    cx, cy = (bbox[0] + bbox[2]) / 2, (bbox[1] + bbox[3]) / 2
    scale = np.identity(3)
    scale[0][0] = scale[1][1] = s
    to_origin, to_centre = np.identity(3), np.identity(3)
    to_origin[0][2], to_origin[1][2] = -cx, -cy
    to_centre[0][2], to_centre[1][2] = crop_size / 2, crop_size / 2
    return np.matmul(to_centre, np.matmul(scale, to_origin))


def get_bbox_from_pose(pose: np.ndarray) -> np.ndarray:
    """[x1, y1, x2, y2] of the non-NaN coordinates, each truncated toward zero by int()."""
    x, y = pose[:, 0], pose[:, 1]
    x, y = x[~np.isnan(x)], y[~np.isnan(y)]
    if len(x) == 0 or len(y) == 0:
        raise ValueError("get_bbox_from_pose: every x or every y is NaN")
    return np.array([int(np.min(x)), int(np.min(y)), int(np.max(x)), int(np.max(y))])


def recrop_transform(kp2d: np.ndarray, T: np.ndarray, crop_size: int = CROP_SIZE) -> np.ndarray:
    """pred()'s step between the two passes: the box of the pass-1 keypoints mapped back through inv(T) -> T2."""
    box = get_bbox_from_pose(kp2d)
    corners = np.concatenate((box.reshape(2, 2).T, np.ones((1, 2))), axis=0)
    corners = np.matmul(np.linalg.inv(T)[:2], corners)
    return create_affine_transform_from_bbox(corners.T.reshape(4), crop_size)


def move_palm_to_wrist(kp3d: np.ndarray) -> np.ndarray:
    kp3d[0] = 2 * kp3d[0] - kp3d[3]
    return kp3d


def convert_order(kp3d: np.ndarray) -> np.ndarray:
    return kp3d[list(FH_ORDER)].copy()


def to_freihand(kp3d: np.ndarray, scale: float) -> np.ndarray:
    """One sample's [21, 3] model-order kp3d -> FreiHAND order and metres (pred()'s tail), float64."""
    kp = move_palm_to_wrist(np.asarray(kp3d, dtype=np.float32).astype(np.float64))
    return convert_order(kp) * scale


def normalisation_table() -> np.ndarray:
    """[3, 256] float32: preprocess()'s u8 -> float32 chain, float32(u) / 255, minus the float64 mean, over the float64
    std, then float32."""
    u = np.arange(256, dtype=np.uint8).astype(np.float32) / 255
    t = (u[None, :] - np.array(IMAGE_MEAN)[:, None]) / np.array(IMAGE_STD)[:, None]
    return t.astype(np.float32)


def initial_transform(crop_size: int = CROP_SIZE, bbox_scale: float = BBOX_SCALE) -> np.ndarray:
    """pred_fh.py's pass-1 matrix: modify_bbox([0, 0, S, S], 0.33) on the crop size (not the image size)."""
    box = modify_bbox(np.array([0, 0, crop_size, crop_size], dtype=np.float32), bbox_scale)
    return create_affine_transform_from_bbox(box, crop_size)


# ------------------------------------------------------------------ batched prediction
def _dev(x, device, dtype) -> Tensor:
    t = torch.as_tensor(x)
    if t.device != device:
        t = (t.pin_memory() if not t.is_cuda else t).to(device, non_blocking=True)
    return t.to(dtype).contiguous()


class FreiHANDPredictor:
    """pred_fh.py's two-pass prediction for a whole batch on the device.

    predict(images_u8 [B,H,W,3], K [B,3,3], scale [B]) -> float64 [B,21,3] HIP tensor, FreiHAND joint order, metres.
    `last` keeps the pass-1 / pass-2 output dicts and T1 / T2 of the latest call (tests).
    precision: "fp32" / 32 (the reference's, the default), or "bf16" / "fp16" / 16 (= fp16): both passes run under
    `torch.autocast("cuda", dtype)` -- the backbone on the 16-bit convolution kernels, crops, head and lifting in fp32 / fp64 as
    before.  fold_bn (16-bit only): the eval-mode BatchNorm layers of the bottleneck blocks in the convolution epilogues
    (`bn2d.fold_plan`); None = the default for the precision, `FOLD_BN_DEFAULT`."""

    PRECISIONS = {"fp32": None, 32: None, "bf16": torch.bfloat16, "fp16": torch.float16, 16: torch.float16}
    FOLD_BN_DEFAULT = True        # what fold_bn=None means for a 16-bit precision

    def __init__(self, model: RN25DwMLPref, crop_size: int = CROP_SIZE, bbox_scale: float = BBOX_SCALE, precision="fp32", fold_bn=None):
        if isinstance(precision, bool) or not isinstance(precision, (str, int)) or precision not in self.PRECISIONS:
            raise ValueError(f"{type(self).__name__}: precision must be one of 'fp32', 32, 'bf16', 'fp16', 16 -- got {precision!r}")
        self.autocast_dtype = self.PRECISIONS[precision]
        self.fold_bn = self.autocast_dtype is not None and (self.FOLD_BN_DEFAULT if fold_bn is None else bool(fold_bn))
        self.model, self.size = model, crop_size
        self.T1 = initial_transform(crop_size, bbox_scale)
        self.device = model.backend_model.fc.weight.device
        if self.device.type != "cuda":
            raise _capi.PeclrHipError(f"{type(self).__name__}: the model must be on a HIP device (peclr_amd has no CPU path)")
        self._table = torch.from_numpy(normalisation_table()).to(self.device)
        self._T1 = torch.from_numpy(self.T1).reshape(1, 3, 3).to(self.device)
        self.last = None
        self._graph = None

    def _passes(self, images: Tensor, K: Tensor, scale: Tensor):
        if self.autocast_dtype is None:                   # fp32: exactly the launches of before (whatever the switches say)
            return self._two_passes(images, K, scale)
        with torch.autocast("cuda", dtype=self.autocast_dtype), _bn2d.routing(fold_eval_bn=self.fold_bn):
            return self._two_passes(images, K, scale)

    def _two_passes(self, images: Tensor, K: Tensor, scale: Tensor):
        m = self.model
        if m.training or not m.backend_model.bn1.hip:
            raise _capi.PeclrHipError("FreiHANDPredictor: the model must be in eval mode with the HIP kernels on (enable_hip())")
        b = images.shape[0]
        T1 = self._T1.expand(b, 3, 3).contiguous()
        with torch.no_grad():
            x1, k1 = _capi.pose_crop(images, T1, K, self._table, self.size)
            out1, T2, _, status = m._head_hip(m.features(x1), k1, T1=T1, size=self.size)
            x2, k2 = _capi.pose_crop(images, T2, K, self._table, self.size)
            out2, _, fh, status = m._head_hip(m.features(x2), k2, scale=scale, status=status)
        self.last = {"pass1": out1, "pass2": out2, "T1": T1, "T2": T2, "K1": k1, "K2": k2}
        return fh, status

    def _inputs(self, images, K, scale):
        images = _dev(images, self.device, torch.uint8)
        K = _dev(K, self.device, torch.float64).reshape(-1, 3, 3)
        scale = _dev(scale, self.device, torch.float64).reshape(-1)
        return images, K, scale

    @staticmethod
    def _raise_on_status(status: Tensor):
        """The one host synchronisation: the status words through pinned memory and an event."""
        host = torch.empty(status.shape, dtype=status.dtype, pin_memory=True)
        host.copy_(status, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        bad = np.flatnonzero(host.numpy())
        if len(bad):
            what = "no keypoint coordinate to box" if host.numpy()[bad[0]] & _capi.POSE_STATUS_NO_BBOX else "NaN detected"
            raise FloatingPointError(f"FreiHAND prediction failed for sample(s) {bad.tolist()}: {what}")

    def predict(self, images_u8, K, scale) -> Tensor:
        fh, status = self._passes(*self._inputs(images_u8, K, scale))
        self._raise_on_status(status)
        return fh

    def capture(self, batch: int, image_hw=(224, 224)) -> "FreiHANDPredictor":
        """Record both passes for `batch` images of `image_hw` as one hipGraph over static input buffers (after one eager call,
        which creates the weight planes and warms the allocator); `replay` then runs it."""
        h, w = image_hw
        self._static = (torch.zeros((batch, h, w, 3), dtype=torch.uint8, device=self.device),
                        torch.from_numpy(np.array(K_DEFAULT)).expand(batch, 3, 3).contiguous().to(self.device),
                        torch.ones((batch,), dtype=torch.float64, device=self.device))
        self._passes(*self._static)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._static_out = self._passes(*self._static)
        self._graph_last = self.last
        self._graph = g
        return self

    def replay(self, images_u8, K, scale) -> Tensor:
        if self._graph is None:
            raise RuntimeError("FreiHANDPredictor.replay: call capture(batch) first")
        images, K, scale = self._inputs(images_u8, K, scale)
        si, sk, ss = self._static
        if images.shape != si.shape:
            raise ValueError(f"replay: captured for images {tuple(si.shape)}, got {tuple(images.shape)}")
        si.copy_(images)
        sk.copy_(K)
        ss.copy_(scale)
        self._graph.replay()
        self.last = self._graph_last
        fh, status = self._static_out
        self._raise_on_status(status)
        return fh.clone()


def write_freihand_submission(path: str, kp3d) -> str:
    """pred_fh.py's dump(): `<path>.json` = [xyz_list, verts_list] (verts: zeros [778, 3] per sample, the reference does not
    predict them) and `<path>.zip` holding that file under its base name.  Returns the json path."""
    base = path[:-5] if path.endswith(".json") else path
    kp = np.asarray(kp3d.detach().cpu() if isinstance(kp3d, Tensor) else kp3d, dtype=np.float64)
    verts = np.zeros((778, 3)).tolist()
    d = os.path.dirname(base)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(base + ".json", "w") as f:
        json.dump([[k.tolist() for k in kp], [verts for _ in range(len(kp))]], f)
    with zipfile.ZipFile(base + ".zip", "w", zipfile.ZIP_DEFLATED) as z:
        z.write(base + ".json", arcname=os.path.basename(base) + ".json")
    return base + ".json"
