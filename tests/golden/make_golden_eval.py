"""Golden vectors for scoring pose predictions, from the reference's own code (src/experiments/evaluation_utils.py).

Needs a checkout of the reference (REFERENCE_ROOT in _ref_import.py); not run by the tests:

    python tests/golden/make_golden_eval.py

Stubs on top of `_ref_import.install_stubs()`: `tqdm`, `src.data_loader.data_set` and `src.data_loader.utils` (the module
imports names from them that the recorded functions never call).  torch.svd runs on the CPU.

Recorded (g12_pose_eval.npz, g12_pose_eval.json), for B in {1, 7, 130}, the inputs once in float64 (values float32 holds exactly) and the reference's outputs
for float64 inputs and for the same inputs cast to float32:
- calc_procrustes_transform(X = gt, Y = pred): y_transform, rot_mat, scale, translation
- calculate_epe_statistics (dist, mean, median, min, max) on the raw and on the aligned cloud, and with dim = 2
- get_pck_curves(per_joint=True) and cal_auc_joints of both distance sets, get_pck_curves(per_joint=False) of the raw set;
  get_procrustes_statistics
- e_ref32 per case: the largest |float32 run - float64 run| of y_transform, rot_mat and scale
- e_np64: the largest difference of tests/eval_ref.py (float64 NumPy) from the float64 run, in the units of the tests' bars
- gap_min: the smallest relative distance of any reference distance to any non-zero threshold (asserted >= 1e-5: PCK counts
  can then be compared exactly)
The B = 7 batch: row 0 mirrored prediction, 1 pred == gt, 2 both clouds planar, 3 prediction x1000 and far away, 4.. noisy.
Apart from the cases (their means would not be finite): a row with a NaN and a row whose prediction is all zeros.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402

_ref_import.install_stubs()
_ref_import._mod("tqdm", tqdm=lambda it, *a, **k: it)
_ref_import._mod("src.data_loader.data_set", Data_Set=object)
_ref_import._mod("src.data_loader.utils", convert_2_5D_to_3D=None)

from src.experiments import evaluation_utils as ev  # noqa: E402

import eval_ref  # noqa: E402

SEED = 14   # (12 and 13 put a distance within 1e-5 of a threshold)
GAP_BAR = 1e-5
rng = np.random.default_rng(SEED)
SPECIAL = {"mirrored": 0, "identity": 1, "planar": 2, "scaled": 3, "noisy": 4}


def _rotation():
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _hand():
    """A hand-sized cloud (metres): 21 joints spread over ~0.1 around a point in front of the camera."""
    return rng.standard_normal((21, 3)) * np.array([0.04, 0.05, 0.02]) + np.array([0.05, -0.03, 0.6])


def _noisy(gt):
    """A rotated, rescaled, shifted copy plus per-joint errors: lengths spread over 0 .. 0.6 times the row's quality."""
    c = gt.mean(0)
    moved = (gt - c) @ _rotation().T * rng.uniform(0.8, 1.25) + c + rng.standard_normal(3) * 0.02
    dirs = rng.standard_normal((21, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return moved + dirs * rng.uniform(0.0, 0.6, (21, 1)) * rng.uniform(0.02, 1.0)


def _batch(b, special):
    gt = np.stack([_hand() for _ in range(b)])
    pred = np.stack([_noisy(g) for g in gt])
    if special:
        i = SPECIAL["mirrored"]
        c = gt[i].mean(0)
        pred[i] = ((gt[i] - c) * np.array([-1.0, 1.0, 1.0])) @ _rotation().T * 1.1 + c + rng.standard_normal((21, 3)) * 0.002
        i = SPECIAL["identity"]
        pred[i] = gt[i]
        i = SPECIAL["planar"]
        gt[i, :, 2] = 0.6
        pred[i] = gt[i] + np.concatenate([rng.standard_normal((21, 2)) * 0.01, np.zeros((21, 1))], axis=1)
        pred[i, :, 2] = 0.55
        i = SPECIAL["scaled"]
        c = gt[i].mean(0)
        pred[i] = ((gt[i] - c) @ _rotation().T + rng.standard_normal((21, 3)) * 0.003) * 1000.0 + np.array([2.5e4, -1.2e4, 6.0e5])
    return _f32_exact(gt), _f32_exact(pred)


def _f32_exact(a):
    """Inputs are float64 numbers that float32 holds exactly: the float32 and the float64 run of the reference then see the SAME
    clouds, and e_ref32 measures float32 arithmetic alone -- not the rounding of the inputs, which any float32 implementation
    shares with the reference and which would otherwise dominate it (the x1000 row: 6e5 has a float32 ulp of 1/16)."""
    return a.astype(np.float32).astype(np.float64)


def _t(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def _stats(d):
    return {k: float(d[k]) for k in ("mean", "median", "min", "max")}


out, meta = {}, {"seed": SEED, "special_rows": SPECIAL, "cases": {}}
thr = np.arange(0.0, 0.5, 0.005)
out["thresholds"] = thr
gap_min = np.inf
e_np64 = 0.0

for b, special in ((1, False), (7, True), (130, False)):
    gt, pred = _batch(b, special)
    out[f"in/{b}/gt"], out[f"in/{b}/pred"] = gt, pred
    case = {}
    runs = {}
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        X, Y = _t(gt, dtype), _t(pred, dtype)
        yt, rot, scale, trans = ev.calc_procrustes_transform(X, Y)
        assert yt.dtype == dtype
        raw = ev.calculate_epe_statistics(Y, X, dim=3)
        raw2d = ev.calculate_epe_statistics(Y, X, dim=2)
        al = ev.calculate_epe_statistics(yt, X, dim=3)
        pck, thr_ref = ev.get_pck_curves(raw["eucledian_dist"], per_joint=True)
        pck_al, _ = ev.get_pck_curves(al["eucledian_dist"], per_joint=True)
        assert np.array_equal(thr_ref, thr) and pck.dtype == np.float32 and pck.shape == (21, len(thr))
        auc, auc_al = ev.cal_auc_joints(raw["eucledian_dist"]), ev.cal_auc_joints(al["eucledian_dist"])
        pstats = ev.get_procrustes_statistics({"predictions": Y, "joints_raw": X, "predictions_3d": Y})
        p = f"{name}/{b}/"
        out[p + "aligned"], out[p + "rot"], out[p + "scale"], out[p + "trans"] = (t.numpy() for t in (yt, rot, scale, trans))
        out[p + "dist"], out[p + "dist_2d"] = raw["eucledian_dist"].numpy(), raw2d["eucledian_dist"].numpy()
        out[p + "dist_aligned"] = al["eucledian_dist"].numpy()
        out[p + "pck"], out[p + "pck_aligned"], out[p + "auc"], out[p + "auc_aligned"] = pck, pck_al, auc, auc_al
        overall, _ = ev.get_pck_curves(raw["eucledian_dist"])          # per_joint=False: one float32 mean over all joints
        assert overall.dtype == np.float32 and overall.shape == (len(thr),)
        out[p + "pck_overall"] = overall
        case[name] = {"raw": _stats(raw), "raw_2d": _stats(raw2d), "aligned": _stats(al),
                      "procrustes_statistics": {k: float(v) for k, v in pstats.items()}}
        assert abs(case[name]["procrustes_statistics"]["Mean_EPE_3D_procrustes"] - case[name]["aligned"]["mean"]) == 0.0
        runs[name] = (yt.double().numpy(), rot.double().numpy(), scale.double().numpy())
        th = thr.astype(np.float32 if name == "f32" else np.float64).astype(np.float64)[1:]
        for d in (raw["eucledian_dist"], al["eucledian_dist"]):
            d = d.double().numpy().reshape(-1, 1)
            gap_min = min(gap_min, float((np.abs(d - th[None, :]) / th[None, :]).min()))
    case["e_ref32"] = {k: float(np.abs(runs["f32"][i] - runs["f64"][i]).max()) for i, k in enumerate(("aligned", "rot", "scale"))}

    # the float64 NumPy restatement against the float64 run, in the units of the tests' bars
    yt, rot, scale, trans, normX, normY = eval_ref.procrustes_transform(gt, pred)
    p = f"f64/{b}/"
    nx = normX.reshape(-1, 1, 1)
    e = max(float((np.abs(yt - out[p + "aligned"]) / nx).max()), float((np.abs(trans - out[p + "trans"]) / nx).max()),
            float(np.abs(rot - out[p + "rot"]).max()),
            float((np.abs(scale - out[p + "scale"]) / (normX / normY).reshape(-1, 1, 1)).max()))
    case["e_np64"] = e
    e_np64 = max(e_np64, e)
    meta["cases"][str(b)] = case

# rows that make a batch's means non-finite: inputs only
g = _hand()
bad = _noisy(g)
bad[7, 1] = np.nan
out["in/nan_row/gt"], out["in/nan_row/pred"] = _f32_exact(g[None]), _f32_exact(bad[None])
g = _hand()
out["in/zero_row/gt"], out["in/zero_row/pred"] = _f32_exact(g[None]), np.zeros((1, 21, 3))

assert gap_min >= GAP_BAR, f"a reference distance lies within {gap_min:.2e} (relative) of a threshold: change SEED"
meta["gap_min"], meta["gap_bar"], meta["e_np64"] = gap_min, GAP_BAR, e_np64

np.savez_compressed(os.path.join(HERE, "g12_pose_eval.npz"), **out)
with open(os.path.join(HERE, "g12_pose_eval.json"), "w") as f:
    json.dump(meta, f, indent=1)
print("wrote g12_pose_eval.npz / g12_pose_eval.json; gap_min %.3e, e_np64 %.3e" % (gap_min, e_np64))
print({b: c["e_ref32"] for b, c in meta["cases"].items()})
