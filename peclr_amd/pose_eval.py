"""Scoring pose predictions on the device: end-point error, PCK curves / AUC and the same after a Procrustes alignment.

Restates the reference's src/experiments/evaluation_utils.py (calculate_epe_statistics, calc_procrustes_transform,
get_pck_curves, cal_auc_joints, get_procrustes_statistics and the metric dict of evaluate()) on one HIP kernel,
`peclr_pose_eval` (csrc/pose_eval.hip): per batch ONE launch writes the per-joint distances, aligns every prediction onto its
ground truth in float64 (a 3 x 3 Jacobi SVD per sample, no LAPACK call, no host round trip) and adds the PCK counts of all
thresholds into an integer table.  Nothing here synchronises with the host except where a docstring says so, so scoring can
sit in the same hipGraph as `FreiHANDPredictor`'s two passes.

What stays on the host is what the reference also does in NumPy: the trapezoid rule over the (at most a few hundred)
thresholds, with its roundings -- the per-joint fraction is float32(count) / float32(n), the thresholds are float64.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _capi

NUM_JOINTS = 21
_NP = {torch.float32: np.float32, torch.float64: np.float64}
_trapz = getattr(np, "trapezoid", None) or np.trapz


def _thresholds(threshold_min: float, threshold_max: float, step: float) -> np.ndarray:
    return np.arange(threshold_min, threshold_max, step)


def _need_hip(t: Tensor, what: str):
    if not isinstance(t, Tensor) or not t.is_cuda:
        where = t.device if isinstance(t, Tensor) else type(t).__name__
        raise _capi.PeclrHipError(f"{what}: expected a HIP device tensor, got {where} (peclr_amd has no CPU path)")


def _pair(pred: Tensor, gt: Tensor, what: str):
    _need_hip(pred, what)
    _need_hip(gt, what)
    if pred.dtype not in _NP:
        raise _capi.PeclrHipError(f"{what}: float32 or float64 expected, got {pred.dtype}")
    return pred.contiguous(), gt.to(pred.dtype).contiguous()


def _lower_median(flat_sorted: Tensor, n: Tensor) -> Tensor:
    """torch.median of the first n elements of an ascending vector whose tail is padding: element (n - 1) // 2."""
    idx = ((n - 1).clamp(min=0) // 2).to(torch.int64).reshape(1)
    return flat_sorted.gather(0, idx)[0]


# ------------------------------------------------------------------ the reference's functions
def epe_statistics(pred: Tensor, gt: Tensor, dim: int = 3) -> Dict[str, Tensor]:
    """calculate_epe_statistics: {"eucledian_dist" [B,21], "mean", "median", "min", "max"} (the reference's spelling), device
    tensors of the inputs' dtype.  dim = 2: only x and y count.  The distances come from the kernel (float64 arithmetic, one
    rounding), the mean is reduced in float64, the median is torch's lower median.  No host synchronisation."""
    if dim not in (2, 3):
        dim = 3                      # the reference: "Coordinates treated as 3D"
    pred, gt = _pair(pred, gt, "epe_statistics")
    dist = _capi.pose_eval(pred, gt, dim=dim, procrustes=False)["dist"]
    return {"eucledian_dist": dist, "mean": dist.double().mean().to(dist.dtype), "median": torch.median(dist),
            "min": torch.min(dist), "max": torch.max(dist)}


def procrustes_transform(X: Tensor, Y: Tensor) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor], Optional[Tensor]]:
    """calc_procrustes_transform: the similarity transform of Y [B,21,3] that best matches X, per sample ->
    (y_transform [B,21,3], rot_mat [B,3,3], scale [B,1,1], translation [B,1,3]).

    The reference's early exit is kept here, and only here: when X or Y is all zeros (FreiHAND's evaluation split has no
    labels) nothing is computed.  That test reads a device value, so THIS CALL MAY SYNCHRONISE with the host (the
    streaming `PoseEvaluator` never does).  The reference then returns the malformed `(Y, (tensor([]),) * 3)`, a 2-tuple;
    this returns `(Y, None, None, None)`, which unpacks like the regular result.

    A sample whose centred X or Y has norm 0 (or holds a NaN) gets NaN outputs, as the reference's 0 / 0 gives."""
    Y, X = _pair(Y, X, "procrustes_transform")
    if bool(torch.all(X == 0)) or bool(torch.all(Y == 0)):
        return Y, None, None, None
    out = _capi.pose_eval(Y, X, dim=3, procrustes=True)
    b = Y.shape[0]
    return out["aligned"], out["rot"], out["scale"].view(b, 1, 1), out["trans"].view(b, 1, 3)


def _counts_of(dist: Tensor, thr: np.ndarray) -> Tensor:
    """[21, T] int64 counts of dist[:, j] < thr[k] from the kernel: a distance d enters as the point (d, 0, 0) against the
    origin with dim = 2, and sqrt(d * d) == d exactly in IEEE arithmetic, so the kernel compares d itself -- the same
    comparison, in dist's dtype, that fills `PoseEvaluator`'s table."""
    _need_hip(dist, "pck_curves")
    if dist.dim() != 2 or dist.shape[1] != NUM_JOINTS or dist.dtype not in _NP:
        raise _capi.PeclrHipError(f"pck_curves: distances must be [B,21] float32 / float64, got {dist.dtype} {tuple(dist.shape)}")
    pts = torch.zeros(dist.shape + (3,), dtype=dist.dtype, device=dist.device)
    pts[..., 0] = dist
    t = torch.from_numpy(thr.astype(_NP[dist.dtype])).to(dist.device)
    counts = torch.zeros((2, NUM_JOINTS, len(thr)), dtype=torch.int64, device=dist.device)
    _capi.pose_eval(pts, torch.zeros_like(pts), dim=2, procrustes=False, thr=t, counts=counts)
    return counts[0]


def curve_from_counts(counts, n: int, per_joint: bool = True) -> np.ndarray:
    """The reference's float32 `torch.mean((dist < theta) * 1.0)`: count / n, one float32 rounding.  counts [21, T] integers."""
    counts = np.asarray(counts)
    if per_joint:
        return np.float32(counts) / np.float32(n)
    return np.float32(counts.sum(0)) / np.float32(n * counts.shape[0])


def auc_from_counts(counts, n: int, thresholds, per_joint: bool = True):
    """cal_auc_joints from integer PCK counts [21, T] of n samples: trapezoid rule over the float64 thresholds on the float32
    per-joint fractions, over the area under a curve of ones."""
    thresholds = np.asarray(thresholds, dtype=np.float64)
    curve = curve_from_counts(counts, n)
    norm = _trapz(y=np.ones(len(thresholds)), x=thresholds)
    auc = np.array([_trapz(y=curve[j], x=thresholds) / norm for j in range(curve.shape[0])])
    return auc if per_joint else np.mean(auc)


def pck_curves(dist: Tensor, threshold_min: float = 0.0, threshold_max: float = 0.5, step: float = 0.005,
               per_joint: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """get_pck_curves: the share of keypoints under each threshold of np.arange(threshold_min, threshold_max, step) ->
    (curve [T] or [21, T] float32, thresholds [T] float64).  One launch and ONE copy to the host (the reference: one
    reduction and one .cpu() per threshold); returning NumPy arrays, it synchronises."""
    thr = _thresholds(threshold_min, threshold_max, step)
    counts = _counts_of(dist, thr).cpu().numpy()
    return curve_from_counts(counts, dist.shape[0], per_joint), thr


def auc_joints(dist: Tensor, per_joint: bool = True):
    """cal_auc_joints: area under the per-joint PCK curves over thresholds 0 .. 0.5 step 0.005, per joint or their mean."""
    thr = _thresholds(0.0, 0.5, 0.005)
    return auc_from_counts(_counts_of(dist, thr).cpu().numpy(), dist.shape[0], thr, per_joint)


# ------------------------------------------------------------------ streaming
class PoseEvaluator:
    """The metric dict of the reference's evaluate(), accumulated batch by batch on the device.

        ev = PoseEvaluator(capacity=len(dataset))
        for ...: ev.update(pred_xyz, gt_xyz)        # one launch, no host synchronisation
        metrics = ev.compute()                      # the single synchronisation

    update(pred, gt) appends the batch's [B,21] raw and Procrustes-aligned distances to preallocated [capacity,21]
    buffers and adds its PCK counts to one int64 [2,21,T] table.  update_2d(kp2d_pred, kp2d_gt) is an optional second
    stream for Mean_EPE_2D / Median_EPE_2D ([B,21,2], or [B,21,3] whose z is ignored).

    Where the rows go.  The fill position lives in a DEVICE integer that the launch reads and itself advances, so an
    update() recorded in a hipGraph appends on every replay instead of overwriting the rows of the capture.  The host
    keeps its own count of the rows its update() calls have asked for -- it is what lets update() refuse a batch beyond
    `capacity` without a synchronisation -- but it cannot see replays; compute() therefore takes the number of samples
    from the device integer.  Replays that run past `capacity` write nothing (the kernel checks) and make compute() raise.
    The launch that advances the integer assumes it is alone with it: every update() (and every replay of a graph that
    holds one) of one evaluator must be ordered on ONE stream.  Two updates in flight on different streams would fill the
    same rows.

    compute() returns exactly the reference's keys -- Mean_EPE_3D, Median_EPE_3D, AUC, Mean_EPE_3D_procrustes,
    Median_EPE_3D_procrustes, auc_procrustes (and Mean_EPE_2D, Median_EPE_2D when update_2d was fed) -- plus `pck` and
    `pck_procrustes` ([21, T] float32 per-joint curves) and `thresholds`.  Means are reduced in float64 on the device
    and returned in the evaluator's dtype; medians are torch's lower median."""

    def __init__(self, capacity: int, dtype: torch.dtype = torch.float64, thresholds=(0.0, 0.5, 0.005), device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise _capi.PeclrHipError(f"PoseEvaluator: expected a HIP device, got {device} (peclr_amd has no CPU path)")
        if dtype not in _NP:
            raise _capi.PeclrHipError(f"PoseEvaluator: float32 or float64 expected, got {dtype}")
        if capacity <= 0:
            raise ValueError("PoseEvaluator: capacity must be positive")
        self.capacity, self.dtype, self.device = int(capacity), dtype, device
        self.thresholds = _thresholds(*thresholds)
        self._thr = torch.from_numpy(self.thresholds.astype(_NP[dtype])).to(device)
        z = dict(device=device)
        self._dist = torch.zeros((capacity, NUM_JOINTS), dtype=dtype, **z)
        self._dist_al = torch.zeros((capacity, NUM_JOINTS), dtype=dtype, **z)
        self._dist_2d = None                      # allocated by the first update_2d
        self._status = torch.zeros((2, capacity), dtype=torch.int32, **z)      # 3D stream, 2D stream
        self._cursor = torch.zeros((2, 2), dtype=torch.int32, **z)            # per stream {rows filled, ticket}
        self._counts = torch.zeros((2, NUM_JOINTS, len(self.thresholds)), dtype=torch.int64, **z)
        self._asked = [0, 0]
        self._lifted = {}                         # update_25d's 3D predictions and root depths, per batch size

    def reset(self) -> "PoseEvaluator":
        """Forget everything fed so far (stream-ordered fills, no synchronisation)."""
        self._status.zero_()
        self._cursor.zero_()
        self._counts.zero_()
        self._asked = [0, 0]
        return self

    def _room(self, stream: int, b: int):
        if self._asked[stream] + b > self.capacity:
            raise ValueError(f"PoseEvaluator: {self._asked[stream]} + {b} samples exceed the capacity of {self.capacity}")

    def update(self, pred: Tensor, gt: Tensor) -> None:
        """Score one batch: pred, gt [B,21,3] HIP tensors (cast to the evaluator's dtype).  One kernel launch on the current
        stream, no host synchronisation, capturable into a hipGraph.  Raises ValueError when the host-side count says the
        batch does not fit `capacity`, PeclrHipError for CPU tensors or wrong shapes; a call that raises leaves the
        evaluator as it was.  All update() calls of one evaluator must be ordered on one stream (see the class docstring)."""
        pred, gt = _pair(pred, gt, "PoseEvaluator.update")
        self._room(0, pred.shape[0])
        _capi.pose_eval(pred.to(self.dtype), gt.to(self.dtype), dim=3, procrustes=True, thr=self._thr, counts=self._counts,
                        status=self._status[0], dist=self._dist, dist_aligned=self._dist_al, cursor=self._cursor[0],
                        want_transform=False)
        self._asked[0] += pred.shape[0]          # only once the launch is enqueued: a refused call asks for nothing

    def update_25d(self, pred25d: Tensor, scale: Tensor, K: Tensor, gt3d: Tensor) -> None:
        """Score one batch of 2.5D predictions, as the reference's evaluate() does: pred25d [B,21,3], scale [B], K [B,3,3]
        float32 HIP tensors are lifted with convert_2_5D_to_3D (`peclr_joints25d_to_3d`: one launch into a buffer this
        evaluator owns, one per batch size) and the result is scored against gt3d [B,21,3] by update()'s launch.  Same
        guarantees and exceptions as update(): no host synchronisation, capturable into a hipGraph, a refused call leaves
        the evaluator as it was."""
        for t, what in ((pred25d, "pred25d"), (scale, "scale"), (K, "K"), (gt3d, "gt3d")):
            _need_hip(t, f"PoseEvaluator.update_25d {what}")
        b = pred25d.shape[0]
        self._room(0, b)
        if b not in self._lifted:
            self._lifted[b] = (torch.empty((b, NUM_JOINTS, 3), dtype=torch.float32, device=self.device),
                               torch.empty((b,), dtype=torch.float32, device=self.device))
        out, z_root = self._lifted[b]
        _capi.joints25d_to_3d(pred25d, scale, K, out=out, z_root=z_root)
        self.update(out, gt3d)

    def update_2d(self, kp2d_pred: Tensor, kp2d_gt: Tensor) -> None:
        """The optional 2D stream: kp2d_pred, kp2d_gt [B,21,2] (or [B,21,3], z ignored) feed Mean_EPE_2D / Median_EPE_2D through
        the same kernel with dim = 2.  Same guarantees and exceptions as update(); its rows are counted apart from update()'s."""
        pred, gt = _pair(kp2d_pred, kp2d_gt, "PoseEvaluator.update_2d")
        if pred.shape[-1] == 2:
            pred, gt = torch.nn.functional.pad(pred, (0, 1)), torch.nn.functional.pad(gt, (0, 1))
        self._room(1, pred.shape[0])
        if self._dist_2d is None:
            self._dist_2d = torch.zeros((self.capacity, NUM_JOINTS), dtype=self.dtype, device=self.device)
        _capi.pose_eval(pred.to(self.dtype), gt.to(self.dtype), dim=2, procrustes=False, status=self._status[1],
                        dist=self._dist_2d, cursor=self._cursor[1])
        self._asked[1] += pred.shape[0]

    def _mean_median(self, dist: Tensor, n: Tensor) -> Tensor:
        """[mean, median] (float64) of the first n rows; n is a device scalar."""
        valid = (torch.arange(self.capacity, device=self.device) < n)[:, None]
        count = (n * NUM_JOINTS).clamp(min=1)
        d = dist.double()
        mean = torch.where(valid, d, torch.zeros_like(d)).sum() / count
        flat = torch.where(valid, d, torch.full_like(d, float("inf"))).reshape(-1).sort().values
        median = _lower_median(flat, n * NUM_JOINTS)
        has_nan = torch.isnan(torch.where(valid, d, torch.zeros_like(d))).any()       # torch.median: NaN wins
        return torch.stack([mean, torch.where(has_nan, torch.full_like(median, float("nan")), median)])

    def compute(self, allow_nan: bool = False) -> dict:
        """The metrics of everything fed so far.  The ONE host synchronisation: every reduction is enqueued first, the
        results travel through pinned memory behind one event.  Raises FloatingPointError naming the samples whose
        status is set (a NaN coordinate; a cloud whose centred norm is 0 or not finite) unless allow_nan=True, in which
        case the affected metrics are the NaNs the reference would report."""
        n3, n2 = (self._cursor[s, 0].clamp(max=self.capacity) for s in (0, 1))
        parts = [self._mean_median(self._dist, n3), self._mean_median(self._dist_al, n3)]
        if self._dist_2d is not None:
            parts.append(self._mean_median(self._dist_2d, n2))
        dev = [torch.cat(parts), self._counts.reshape(-1), torch.cat([self._cursor.reshape(-1), self._status.reshape(-1)])]
        host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in dev]
        for h, t in zip(host, dev):
            h.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        stats, counts, ints = (h.numpy() for h in host)
        filled = [int(ints[0]), int(ints[2])]
        for s, what in ((0, "update"), (1, "update_2d")):
            if filled[s] > self.capacity:
                raise RuntimeError(f"PoseEvaluator: {what} launches asked for {filled[s]} rows, capacity is {self.capacity}; "
                                   "the launches that did not fit wrote nothing")
        status = ints[4:].reshape(2, self.capacity)
        if not allow_nan:
            for s, what in ((0, "sample(s)"), (1, "2D sample(s)")):
                bad = np.flatnonzero(status[s, :filled[s]])
                if len(bad):
                    bits = int(np.bitwise_or.reduce(status[s, bad]))
                    why = [w for bit, w in ((_capi.POSE_STATUS_NAN, "NaN detected"),
                                            (_capi.POSE_EVAL_DEGENERATE, "degenerate cloud (centred norm 0 or not finite)"))
                           if bits & bit]
                    raise FloatingPointError(f"pose evaluation failed for {what} {bad.tolist()}: {', '.join(why)}")
        n = filled[0]
        if n == 0 and not filled[1]:
            raise RuntimeError("PoseEvaluator.compute: no samples")
        cast = _NP[self.dtype]
        out = {}
        if n:                                            # (a 2D-only protocol, YouTube-3D-Hands', feeds update_2d alone)
            counts = counts.reshape(2, NUM_JOINTS, -1)
            out = {"Mean_EPE_3D": cast(stats[0]), "Median_EPE_3D": cast(stats[1]),
                   "AUC": float(np.mean(auc_from_counts(counts[0], n, self.thresholds))),
                   "Mean_EPE_3D_procrustes": cast(stats[2]), "Median_EPE_3D_procrustes": cast(stats[3]),
                   "auc_procrustes": float(np.mean(auc_from_counts(counts[1], n, self.thresholds)))}
        if self._dist_2d is not None and filled[1]:
            out["Mean_EPE_2D"], out["Median_EPE_2D"] = cast(stats[4]), cast(stats[5])
        if n:
            out["pck"], out["pck_procrustes"] = curve_from_counts(counts[0], n), curve_from_counts(counts[1], n)
        out["thresholds"] = self.thresholds.copy()
        return out

    def distances(self, n: int) -> Tuple[Tensor, Tensor]:
        """Views of the first n rows of the raw and the aligned distance buffers (n: a count the caller knows)."""
        return self._dist[:n], self._dist_al[:n]
