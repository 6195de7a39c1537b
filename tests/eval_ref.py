"""float64 NumPy restatement of the reference's scoring functions (src/experiments/evaluation_utils.py), test-side like
tests/pose_ref.py: calculate_epe_statistics, calc_procrustes_transform (np.linalg.svd), get_pck_curves, cal_auc_joints.
tests/test_pose_eval_host.py holds it against the recorded outputs of the reference itself (tests/golden/g12_pose_eval.*)."""
import numpy as np

_trapz = getattr(np, "trapezoid", None) or np.trapz


def epe_statistics(pred, gt, dim=3):
    pred, gt = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    if dim == 2:
        pred, gt = pred[:, :, :2], gt[:, :, :2]
    dist = np.sqrt(((pred - gt) ** 2).sum(2))
    flat = np.sort(dist.reshape(-1))
    return {"eucledian_dist": dist, "mean": dist.mean(), "median": flat[(len(flat) - 1) // 2],   # torch's lower median
            "min": dist.min(), "max": dist.max()}


def procrustes_transform(X, Y):
    """(y_transform, rot_mat, scale [B,1,1], translation [B,1,3], normX [B], normY [B]) of Y aligned onto X."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    muX, muY = X.mean(1, keepdims=True), Y.mean(1, keepdims=True)
    X0, Y0 = X - muX, Y - muY
    normX = np.sqrt((X0 ** 2).sum((1, 2), keepdims=True))
    normY = np.sqrt((Y0 ** 2).sum((1, 2), keepdims=True))
    X0, Y0 = X0 / normX, Y0 / normY
    A = np.matmul(X0.transpose(0, 2, 1), Y0)
    U, s, Vt = np.linalg.svd(A)
    V = Vt.transpose(0, 2, 1).copy()
    s = s.copy()
    sign = np.sign(np.linalg.det(np.matmul(V, U.transpose(0, 2, 1))))
    V[:, :, -1] *= sign[:, None]
    s[:, -1] *= sign
    rot = np.matmul(V, U.transpose(0, 2, 1))
    ratio = s.sum(1).reshape(-1, 1, 1)
    scale = ratio * normX / normY
    trans = muX - scale * np.matmul(muY, rot)
    y_transform = normX * ratio * np.matmul(Y0, rot) + muX
    return y_transform, rot, scale, trans, normX.reshape(-1), normY.reshape(-1)


def thresholds(threshold_min=0.0, threshold_max=0.5, step=0.005):
    return np.arange(threshold_min, threshold_max, step)


def pck_counts(dist, thr):
    """[21, T] integer counts of dist[:, j] < thr[k]; the comparison in dist's dtype, as torch compares a tensor with a scalar."""
    dist = np.asarray(dist)
    thr = np.asarray(thr).astype(dist.dtype)
    return (dist[:, :, None] < thr[None, None, :]).sum(0).astype(np.int64)


def pck_curve(dist, thr):
    """get_pck_curves(per_joint=True): the float32 mean of a 0/1 tensor, count / n rounded once."""
    return np.float32(pck_counts(dist, thr)) / np.float32(len(dist))


def auc_from_curve(curve, thr):
    thr = np.asarray(thr, dtype=np.float64)
    norm = _trapz(y=np.ones(len(thr)), x=thr)
    return np.array([_trapz(y=curve[j], x=thr) / norm for j in range(curve.shape[0])])
