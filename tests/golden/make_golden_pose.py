"""Golden vectors for the fine-tuned 2.5D hand-pose model and the FreiHAND prediction helpers, from the reference's own
code (src/models/rn_25D_wMLPref.py, testing/fh_utils.py, testing/pred_fh.py).

Needs a checkout of the reference (REFERENCE_ROOT in _ref_import.py); not run by the tests:

    python tests/golden/make_golden_pose.py

Stubs on top of `_ref_import.install_stubs()`: `torchvision.models.resnet50 / resnet152` return a backend whose forward
is its `fc` on a 2048-wide feature vector (so the recorded forward is the model's head on given pooled features),
`skimage.io`, `tqdm` and `cv2.warpAffine` (identity: the warp's pixel arithmetic stays unpinned, OpenCV is not available;
what preprocess() does around it -- the normalisation chain and K' = T @ K -- is recorded exactly).

Recorded (g11_pose.npz, g11_pose.json):
- the model's forward in eval mode on pooled features, B in {1, 7, 64}, default and per-sample K, with fc and MLP weights
  and non-trivial BatchNorm running statistics; rows that hit d < eps, both clamp ends and a NaN
- the state_dict keys of the head (fc, zroot_ref) in order
- modify_bbox, create_affine_transform_from_bbox, get_bbox_from_pose (NaN and negative coordinates)
- pred() itself on a stub model: T1, the pass-1 keypoints, T2, the pass-2 kp3d and the submitted joints
- preprocess() on a 1 x 256 ramp image (normalisation table) and its K'
"""
import json
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

_ref_import.install_stubs()


class _StubBackend(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(2048, 1000)

    def forward(self, x):
        return self.fc(x.flatten(1))


tvm = sys.modules["torchvision.models"]
tvm.resnet50 = tvm.resnet152 = _StubBackend
sk = _ref_import._mod("skimage")
sk.io = _ref_import._mod("skimage.io", imread=lambda p: None)
_ref_import._mod("tqdm", tqdm=lambda it, *a, **k: it)
cv2 = sys.modules["cv2"]
cv2.BORDER_CONSTANT = 0
WARPS = []


def _warp_affine(img, M, dsize, borderMode=None, borderValue=None):
    WARPS.append(np.array(M, dtype=np.float64))
    return img


cv2.warpAffine = _warp_affine

from src.models.rn_25D_wMLPref import RN_25D_wMLPref  # noqa: E402
from testing import fh_utils  # noqa: E402
from testing import pred_fh  # noqa: E402

rng = np.random.default_rng(11)
torch.manual_seed(11)
out = {}
meta = {}

# ---- the model's forward on pooled features
model = RN_25D_wMLPref("rn50")
W = (rng.standard_normal((64, 2048)) * 1e-3).astype(np.float16)
W[np.arange(64), np.arange(64)] += np.float16(1.0)      # columns 0..63 of the features steer the 64 outputs
bias = (rng.standard_normal(64) * 0.01).astype(np.float16)
with torch.no_grad():
    model.backend_model.fc.weight.copy_(torch.from_numpy(W.astype(np.float32)))
    model.backend_model.fc.bias.copy_(torch.from_numpy(bias.astype(np.float32)))
    for m in model.zroot_ref.zroot_ref:
        if isinstance(m, nn.Linear):
            m.weight.copy_(torch.randn_like(m.weight) / np.sqrt(m.in_features))
            m.bias.copy_(torch.randn_like(m.bias) * 0.1)
        elif isinstance(m, nn.BatchNorm1d):
            m.weight.copy_(1 + 0.2 * torch.randn_like(m.weight))
            m.bias.copy_(0.1 * torch.randn_like(m.bias))
            m.running_mean.copy_(0.3 * torch.randn_like(m.running_mean))
            m.running_var.copy_(0.5 + torch.rand_like(m.running_var))
model.eval()
sd = model.state_dict()
meta["head_keys"] = list(sd)
for k, v in sd.items():
    out["w/" + k] = v.numpy()
out["w/backend_model.fc.weight"] = W          # exact float16 values: half the bytes
out["w/backend_model.fc.bias"] = bias
meta["K_default"] = model.K_default.numpy().tolist()


def _features(b, special):
    f = rng.standard_normal((b, 2048)).astype(np.float16)
    tgt = np.zeros((b, 21, 3))
    tgt[..., 0] = rng.uniform(40, 184, (b, 21))
    tgt[..., 1] = rng.uniform(40, 184, (b, 21))
    tgt[..., 2] = rng.uniform(-0.25, 0.25, (b, 21))
    if special:
        # row 1: d < eps (large depth difference of bones 3 and 8, close in 2D); row 2: clamp at 50 (close, equal depth);
        # row 3: clamp at 4 (far apart); row 4: a NaN feature
        tgt[1, 3, :] = (110, 110, -0.9)
        tgt[1, 8, :] = (118, 112, 0.9)
        tgt[2, 3, :] = (110, 110, 0.05)
        tgt[2, 8, :] = (111.5, 110.5, 0.05)
        tgt[3, 3, :] = (40, 40, 0.0)
        tgt[3, 8, :] = (190, 180, 0.0)
    f[:, :63] = (tgt.reshape(b, 63) - bias[:63].astype(np.float64)).astype(np.float16)
    if special:
        f[4, 100] = np.nan
    return f


def _k_per_sample(b):
    k = np.zeros((b, 3, 3), dtype=np.float32)
    k[:, 0, 0] = rng.uniform(250, 600, b)
    k[:, 1, 1] = k[:, 0, 0] * rng.uniform(0.98, 1.02, b)
    k[:, 0, 2] = rng.uniform(90, 134, b)
    k[:, 1, 2] = rng.uniform(90, 134, b)
    k[:, 2, 2] = 1
    return k


cases = []
for b, special in ((1, False), (7, True), (64, True)):
    f = _features(b, special)
    out[f"feat_{b}"] = f
    kps = _k_per_sample(b)
    out[f"K_{b}"] = kps
    for kname, K in (("default", None), ("per_sample", torch.from_numpy(kps))):
        with torch.no_grad():
            o = model(torch.from_numpy(f.astype(np.float32)), K)
        name = f"fwd_{b}_{kname}"
        for key in ("kp3d", "zrel", "kp2d", "kp25d"):
            out[f"{name}/{key}"] = o[key].numpy()
        cases.append(name)
meta["forward_cases"] = cases

# which rows hit the special branches (float64 restatement of the closed form on the recorded outputs)
flags = {}
for name in cases:
    kp25d = out[f"{name}/kp25d"].astype(np.float64)
    b = kp25d.shape[0]
    K = (np.array(meta["K_default"]).reshape(1, 3, 3).repeat(b, 0) if name.endswith("default")
         else out[f"K_{b}"].astype(np.float64))
    uv1 = np.concatenate([kp25d[..., :2], np.ones((b, 21, 1))], axis=2)
    ku = np.einsum("bjc,brc->bjr", uv1, np.linalg.inv(K))
    z = kp25d[..., 2]
    xm, ym, xn, yn, zm, zn = ku[:, 3, 0], ku[:, 3, 1], ku[:, 8, 0], ku[:, 8, 1], z[:, 3], z[:, 8]
    a = (xn - xm) ** 2 + (yn - ym) ** 2
    bq = 2 * (zn * (xn ** 2 + yn ** 2 - xn * xm - yn * ym) + zm * (xm ** 2 + ym ** 2 - xn * xm - yn * ym))
    c = (xn * zn - xm * zm) ** 2 + (yn * zn - ym * zm) ** 2 + (zn - zm) ** 2 - 1
    d = bq ** 2 - 4 * a * c
    zr = (-bq + np.sqrt(np.maximum(d, 1e-8))) / (2 * np.maximum(a, 1e-8))
    flags[name] = {"d_below_eps": np.flatnonzero(d < 1e-8).tolist(), "clamp_low": np.flatnonzero(zr < 4).tolist(),
                   "clamp_high": np.flatnonzero(zr > 50).tolist(), "nan": np.flatnonzero(np.isnan(d)).tolist()}
meta["forward_flags"] = flags
for key in ("d_below_eps", "clamp_low", "clamp_high", "nan"):
    assert flags["fwd_7_default"][key], (key, flags["fwd_7_default"])

# ---- fh_utils helpers
boxes = [np.array([0, 0, 224, 224], dtype=np.float32), np.array([10.5, 20.25, 130.0, 90.0]),
         np.array([-30.0, 5.0, 40.0, 200.0]), np.array([3, 7, 100, 60], dtype=np.float32)]
meta["modify_bbox"] = []
for i, bx in enumerate(boxes):
    for s in (0.33, 1.0, 1.7):
        res = fh_utils.modify_bbox(bx.copy(), s)
        meta["modify_bbox"].append({"box": bx.tolist(), "dtype": str(bx.dtype), "scale": s, "out": res.astype(np.float64).tolist()})
meta["affine_from_bbox"] = []
for bx in [np.array([10.5, 20.25, 130.0, 90.0]), np.array([-30.0, 5.0, 40.0, 200.0]),
           fh_utils.modify_bbox(np.array([0, 0, 224, 224], dtype=np.float32), 0.33), np.array([100.0, 100.0, 101.0, 180.0])]:
    for size in (224, 128):
        T = fh_utils.create_affine_transform_from_bbox(bx, size)
        meta["affine_from_bbox"].append({"box": bx.astype(np.float64).tolist(), "dtype": str(bx.dtype), "size": size,
                                         "T": T.tolist()})
poses = []
p = rng.uniform(-40, 260, (21, 2)).astype(np.float32)
poses.append(p)
p = p.copy()
p[[2, 5], 0] = np.nan
p[7, 1] = np.nan
p[0] = (-3.7, -0.4)
poses.append(p)
p = rng.uniform(-5, 5, (21, 2)).astype(np.float32)
poses.append(p)
meta["bbox_from_pose"] = [{"pose": np.where(np.isnan(q), None, q).tolist(), "box": [int(v) for v in fh_utils.get_bbox_from_pose(q)]}
                          for q in poses]

# ---- pred() on a stub model: the two passes' T, the re-crop and the submission joints
pred_fh.dev = torch.device("cpu")
T1 = fh_utils.create_affine_transform_from_bbox(
    fh_utils.modify_bbox(np.array([0, 0, pred_fh.CROP_SIZE, pred_fh.CROP_SIZE], dtype=np.float32), pred_fh.BBOX_SCALE),
    pred_fh.CROP_SIZE)
meta["T1"] = T1.tolist()
pred_cases = []
for i in range(6):
    img = np.zeros((224, 224, 3), dtype=np.uint8)
    K = np.array([[rng.uniform(300, 500), 0, rng.uniform(100, 124)], [0, rng.uniform(300, 500), rng.uniform(100, 124)], [0, 0, 1]])
    scale = float(rng.uniform(0.02, 0.05))
    kp25d_1 = np.concatenate([rng.uniform(-20, 240, (1, 21, 2)), rng.uniform(-0.2, 0.2, (1, 21, 1))], 2).astype(np.float32)
    if i == 1:
        kp25d_1[0, 4, 0] = np.nan
    kp3d_2 = rng.uniform(-0.5, 0.5, (1, 21, 3)).astype(np.float32)
    kp3d_2[..., 2] += 8
    outs = iter([{"kp25d": torch.from_numpy(kp25d_1), "kp3d": torch.zeros(1, 21, 3)},
                 {"kp25d": torch.zeros(1, 21, 3), "kp3d": torch.from_numpy(kp3d_2)}])
    feeds = []

    def _model(feed):
        feeds.append({k: v.numpy() for k, v in feed.items()})
        return next(outs)

    WARPS.clear()
    xyz, verts = pred_fh.pred(img, K, scale, _model, T1)
    pred_cases.append({"K": K.tolist(), "scale": scale, "kp2d_1": np.where(np.isnan(kp25d_1[0, :, :2]), None, kp25d_1[0, :, :2]).tolist(),
                       "kp3d_2": kp3d_2[0].tolist(), "T_pass1": WARPS[0][:2].tolist(), "T_pass2": WARPS[1][:2].tolist(),
                       "K_pass1": feeds[0]["K"][0].tolist(), "K_pass2": feeds[1]["K"][0].tolist(), "xyz": xyz.tolist(),
                       "verts_shape": list(verts.shape)})
meta["pred"] = pred_cases

# ---- preprocess() on a 1 x 256 ramp (identity warp): the normalisation table and K'
ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
Kp = np.array([[412.5, 0.0, 101.25], [0.0, 409.75, 117.5], [0.0, 0.0, 1.0]])
img_t, K_t = fh_utils.preprocess(ramp, Kp, T1, 16)
out["norm_table"] = img_t.float().reshape(3, 256).numpy()
out["preprocess_K"] = K_t.float().numpy()[0]
meta["preprocess_K_in"] = Kp.tolist()

np.savez_compressed(os.path.join(HERE, "g11_pose.npz"), **out)
with open(os.path.join(HERE, "g11_pose.json"), "w") as f:
    json.dump(meta, f, indent=1)
print("wrote g11_pose.npz / g11_pose.json;", {k: v for k, v in flags["fwd_7_default"].items()})
