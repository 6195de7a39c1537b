"""The metrics a supervised step logs, on the device: `calculate_metrics` (reference src/models/utils.py:53-73).

    calculate_metrics(y_pred, y_true, step="train") -> {"EPE_mean_train": ..., "EPE_median_train": ...}

The Euclidean distance of every joint of the batch, then their mean and `torch.median`'s lower median (element (n - 1) // 2
of the ascending order, n = 21 B).  One launch of `peclr_pose_step_metrics_f32` (csrc/pose_metrics.hip) per call -- for one pair
or, as the fine-tuning step uses it, for the 2.5D and the 3D pair at once (`step_metrics`): float64 distances rounded once, a
fixed-order float64 sum, an exact radix select; no atomics, no host synchronisation, capturable into a hipGraph.  A NaN
distance makes both values of its pair NaN.  The results carry no gradient (the reference logs them, nothing more).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor

from . import _capi

NUM_JOINTS = 21
MAX_BATCH = _capi.POSE_METRICS_MAX_BATCH


def _check_pair(pred, truth, what: str):
    """Everything that can be refused is refused here, before any device call."""
    for t, name in ((pred, "y_pred"), (truth, "y_true")):
        if not isinstance(t, Tensor):
            raise TypeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
        if t.dim() != 3 or tuple(t.shape[1:]) != (NUM_JOINTS, 3):
            raise ValueError(f"{what}: {name} must be [B,{NUM_JOINTS},3], got {tuple(t.shape)}")
    if pred.shape != truth.shape:
        raise ValueError(f"{what}: y_pred {tuple(pred.shape)} and y_true {tuple(truth.shape)} differ in shape")
    if not 1 <= pred.shape[0] <= MAX_BATCH:
        raise ValueError(f"{what}: 1 <= B <= {MAX_BATCH} samples per call, got {pred.shape[0]}")


def _check_device(tensors, what: str):
    for t in tensors:
        if not t.is_cuda:
            raise _capi.PeclrHipError(f"{what}: expected HIP device tensors, got one on {t.device} (peclr_amd has no CPU path)")


def _f32(t: Tensor) -> Tensor:
    return t.detach().to(torch.float32).contiguous()


def step_metrics(pred: Tensor, truth: Tensor, pred2: Optional[Tensor] = None, truth2: Optional[Tensor] = None,
                 out: Optional[Tensor] = None) -> Tensor:
    """[mean, median] of |pred - truth|_2 over all joints, then the same of the second pair when there is one -> float32 [4] on
    the device (`out`, when given, is written in place; its last two entries stay as they are without a second pair).  All
    tensors [B,21,3], 1 <= B <= 1024, on a HIP device.  One launch for contiguous float32 inputs, which is what the fine-tuning
    step passes; any other dtype or layout costs a torch copy per tensor first."""
    _check_pair(pred, truth, "step_metrics")
    tensors = [pred, truth]
    if (pred2 is None) != (truth2 is None):
        raise ValueError("step_metrics: the second pair needs both its prediction and its truth")
    if pred2 is not None:
        _check_pair(pred2, truth2, "step_metrics (second pair)")
        if pred2.shape != pred.shape:
            raise ValueError(f"step_metrics: both pairs must hold the same number of samples, got {pred.shape[0]} and {pred2.shape[0]}")
        tensors += [pred2, truth2]
    _check_device(tensors, "step_metrics")
    if pred2 is not None:
        pred2, truth2 = _f32(pred2), _f32(truth2)
    return _capi.pose_step_metrics(_f32(pred), _f32(truth), pred2, truth2, out=out)


def calculate_metrics(y_pred: Tensor, y_true: Tensor, step: str = "train") -> Dict[str, Tensor]:
    """The reference's signature and keys: {"EPE_mean_<step>", "EPE_median_<step>"}, 0-dim float32 device tensors."""
    m = step_metrics(y_pred, y_true)
    return {f"EPE_mean_{step}": m[0], f"EPE_median_{step}": m[1]}
