"""The supervised losses of the 2.5D pose model on the device, with their gradients.

Mirrors `cal_l1_loss` and `cal_3d_loss` (reference src/models/utils.py:20-50, :76-104) for a batch as `SupervisedAugmenter`
yields it: the L1 loss of the 2D joints, of the root-relative depth with and without the bone scale, and of the 3D joints that
`convert_2_5D_to_3D` lifts from the prediction -- each weighted by `joints_valid / joints_valid.sum()`.

    losses = pose_losses(pred, batch["joints"], batch["joints3D"], batch["scale"], batch["K"], batch["joints_valid"])
    (losses["loss_2d"] + losses["loss_z"] + losses["loss_3d"]).backward()

One forward launch pair (per-sample partial sums and per-element gradients; a fixed-order fold) and one backward launch
(csrc/pose_loss.hip): float64 arithmetic from float32 tensors, every emitted tensor rounded once, no atomics, no host
synchronisation -- forward and backward capture into a hipGraph.  The gradient goes to `pred` and to `z_root_calc`; the labels
get none.  The workspaces between forward and backward (about 1 KB per sample) come from torch's allocator, per call.
"""
from __future__ import annotations

from typing import Dict, Mapping, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import _capi

NUM_JOINTS = 21
LOSS_NAMES = ("loss_2d", "loss_z", "loss_z_unscaled", "loss_3d")


def _check_shapes(pred, joints, joints3d, scale, K, joints_valid, z_root_calc, optional=("joints_valid", "z_root_calc")):
    """ValueError for anything that is not a tensor of the expected shape -- before any device call."""
    if not isinstance(pred, Tensor) or pred.dim() != 3 or tuple(pred.shape[1:]) != (NUM_JOINTS, 3) or pred.shape[0] < 1:
        got = tuple(pred.shape) if isinstance(pred, Tensor) else type(pred).__name__
        raise ValueError(f"pred: expected [B,{NUM_JOINTS},3] with B >= 1, got {got}")
    b = pred.shape[0]
    for t, shape, what in ((joints, (b, NUM_JOINTS, 3), "joints"), (joints3d, (b, NUM_JOINTS, 3), "joints3d"), (scale, (b,), "scale"),
                           (K, (b, 3, 3), "K"), (joints_valid, (b, NUM_JOINTS, 1), "joints_valid"), (z_root_calc, (b,), "z_root_calc")):
        if t is None and what in optional:
            continue
        if not isinstance(t, Tensor) or tuple(t.shape) != shape:
            got = tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__
            raise ValueError(f"{what}: expected {list(shape)} for a prediction of {b} samples, got {got}")


class _PoseLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, z_root_calc, joints, joints3d, scale, K, joints_valid):
        losses, g_l1, g_3d, g_zroot, inv_valid = _capi.pose_loss(pred, joints, joints3d, scale, K, joints_valid, z_root_calc)
        ctx.save_for_backward(g_l1, g_3d, g_zroot, scale, inv_valid)
        ctx.want_z_root = z_root_calc is not None and ctx.needs_input_grad[1]
        return tuple(losses.unbind(0))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        g_l1, g_3d, g_zroot, scale, inv_valid = ctx.saved_tensors
        up = torch.stack([g.to(torch.float32) for g in grads])           # [4] on the device: the launch reads it there
        grad_pred, grad_z = _capi.pose_loss_bwd(up, g_l1, g_3d, g_zroot, scale, inv_valid, ctx.want_z_root)
        return grad_pred, grad_z, None, None, None, None, None


def pose_losses(pred: Tensor, joints: Tensor, joints3d: Tensor, scale: Tensor, K: Tensor, joints_valid: Optional[Tensor] = None,
                z_root_calc: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """pred, joints [B,21,3] 2.5D; joints3d [B,21,3]; scale [B]; K [B,3,3]; joints_valid [B,21,1] or None (ones); z_root_calc
    [B] or None (the closed-form root depth of pred's wrist and index MCP) -- contiguous float32 HIP tensors -> the four
    losses as 0-dim float32 device tensors: `loss_2d`, `loss_z`, `loss_z_unscaled` (cal_l1_loss's tuple) and `loss_3d`
    (cal_3d_loss).  Differentiable once with respect to `pred` and `z_root_calc`.  A wrong shape raises ValueError, a CPU
    tensor PeclrHipError, both before the first device call."""
    _check_shapes(pred, joints, joints3d, scale, K, joints_valid, z_root_calc)
    return dict(zip(LOSS_NAMES, _PoseLosses.apply(pred, z_root_calc, joints, joints3d, scale, K, joints_valid)))


def l1_loss(pred: Tensor, joints: Tensor, scale: Tensor, joints_valid: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """cal_l1_loss(pred, joints, scale, joints_valid) -> (loss_2d, loss_z, loss_z_unscaled): the same launches as
    `pose_losses` without the 3D term (no camera matrix is read, no root depth computed)."""
    _check_shapes(pred, joints, None, scale, None, joints_valid, None, optional=("joints3d", "K", "joints_valid", "z_root_calc"))
    return _PoseLosses.apply(pred, None, joints, None, scale, None, joints_valid)[:3]


def loss_3d(pred: Tensor, joints3d: Tensor, scale: Tensor, K: Tensor, joints_valid: Optional[Tensor] = None,
            z_root_calc: Optional[Tensor] = None) -> Tensor:
    """cal_3d_loss(pred, joints3d, scale, K, joints_valid, z_root_calc): the same launches as `pose_losses` without the L1
    terms."""
    _check_shapes(pred, None, joints3d, scale, K, joints_valid, z_root_calc, optional=("joints", "joints_valid", "z_root_calc"))
    return _PoseLosses.apply(pred, z_root_calc, None, joints3d, scale, K, joints_valid)[3]


class PoseLoss(nn.Module):
    """The weighted sum of the four losses on a `SupervisedAugmenter` batch.

    weights: a mapping from `loss_2d` / `loss_z` / `loss_z_unscaled` / `loss_3d` to a number (a missing name is 0), or four
    numbers in that order.  `forward(pred, batch, z_root_calc=None)` reads `joints`, `joints3D`, `scale`, `K` and
    `joints_valid` (optional) of the dict and returns (total, the dict of the four losses)."""

    def __init__(self, weights: Union[Mapping[str, float], Sequence[float]] = (1.0, 1.0, 0.0, 1.0)):
        super().__init__()
        if isinstance(weights, Mapping):
            unknown = set(weights) - set(LOSS_NAMES)
            if unknown:
                raise ValueError(f"weights: unknown loss names {sorted(unknown)}; expected some of {list(LOSS_NAMES)}")
            weights = [float(weights.get(n, 0.0)) for n in LOSS_NAMES]
        weights = [float(w) for w in weights]
        if len(weights) != len(LOSS_NAMES):
            raise ValueError(f"weights: expected {len(LOSS_NAMES)} numbers ({', '.join(LOSS_NAMES)}), got {len(weights)}")
        self.weights = dict(zip(LOSS_NAMES, weights))

    def forward(self, pred: Tensor, batch: Mapping[str, Tensor], z_root_calc: Optional[Tensor] = None):
        losses = pose_losses(pred, batch["joints"], batch["joints3D"], batch["scale"], batch["K"], batch.get("joints_valid"),
                             z_root_calc)
        total = None
        for name, w in self.weights.items():
            if w != 0.0:
                total = losses[name] * w if total is None else total + losses[name] * w
        if total is None:
            total = losses["loss_2d"] * 0.0
        return total, losses
