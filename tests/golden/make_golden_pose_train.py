"""Golden vectors for the 2.5D pose head in TRAIN mode, forward and backward, from the reference's own RN_25D_wMLPref
(src/models/rn_25D_wMLPref.py) under the stubs of make_golden_pose.py: a backend whose forward is its `fc` on pooled features.

Needs a checkout of the reference (REFERENCE_ROOT in _ref_import.py); not run by the tests:

    python tests/golden/make_golden_pose_train.py

The fc and MLP weights are g11's (read from g11_pose.npz, not stored again); the initial running statistics are g11's too.
Cases: B in {2, 5, 37, 67}, each with the default K and a per-sample K, features built as in make_golden_pose.py (kp2d in
40..184 px, zrel in +-0.25; in B = 5 rows 1..3 are g11's special rows: d < eps, clamp at 50, clamp at 4).  The reference runs
twice per case, as model.double() (gold64) and in float32 (gold32), on seeded upstream gradients G3 (kp3d), G25 (the fc
output after the root's zrel is zeroed) and Gz (zroot).  Seeds are rejected until every LeakyReLU input of the float64 run
has |y| >= 1e-4 in both K variants (a unit whose sign flips in fp32 would move every gradient); the margin is recorded.

Recorded (g15_pose_head_train.npz / .json), to stay below the largest fixture of the tree:
- inputs: features as float16 steering columns [B,64] and int8 multiples of 1/32 for the other 1984; K; G3, G25, Gz as int8
  multiples of 1/64;
- gold64 as float64: kp25d, kp3d, zroot, do (the gradient at the fc output, by retain_grad), the gradients of the eight
  vector-shaped MLP parameters, the updated running statistics, num_batches_tracked;
- of the two matrix gradients (0.weight, 3.weight: 192 KB per case in float64) two-sided probes U dW and dW V with the fixed
  vectors of `probes()`; of the LeakyReLU inputs their sign bits and the margin.  dWfc, dbfc, dfeat are not recorded: plain
  linear algebra on `do`;
- gold32 as the figure the tests need: e_ref = max|gold32 - gold64| / max|gold64| per tensor (json), for every tensor
  above and for the full 0.weight, 3.weight, dWfc, dbfc, dfeat.
"""
import copy
import json
import os
import sys

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
        self.fc_out = self.fc(x.flatten(1))
        self.fc_out.retain_grad()            # the gradient at the fc output, before the model zeroes the root's zrel in place
        return self.fc_out.clone()


tvm = sys.modules["torchvision.models"]
tvm.resnet50 = tvm.resnet152 = _StubBackend

from src.models.rn_25D_wMLPref import RN_25D_wMLPref  # noqa: E402

MLP_KEYS = ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias", "6.weight", "6.bias")
MARGIN = 1e-4


def probes(n_out, n_in):
    """Fixed probe vectors U [2, n_out], V [n_in, 2] for the two matrix gradients."""
    U = np.stack([np.cos(0.37 * (k + 1) * np.arange(n_out) + k) for k in range(2)])
    V = np.stack([np.sin(0.53 * (k + 1) * np.arange(n_in) + 2 * k) for k in range(2)], axis=1)
    return U, V


g11 = np.load(os.path.join(HERE, "g11_pose.npz"))
base = RN_25D_wMLPref("rn50")
sd = {k[2:]: torch.from_numpy(np.asarray(g11[k], dtype=np.float32 if g11[k].dtype.kind == "f" else g11[k].dtype))
      for k in g11.files if k.startswith("w/")}
base.load_state_dict(sd)
bias = g11["w/backend_model.fc.bias"].astype(np.float64)


def _features(rng, b, special):
    tgt = np.zeros((b, 21, 3))
    tgt[..., 0] = rng.uniform(40, 184, (b, 21))
    tgt[..., 1] = rng.uniform(40, 184, (b, 21))
    tgt[..., 2] = rng.uniform(-0.25, 0.25, (b, 21))
    if special:      # rows of make_golden_pose.py: d < eps; clamp at 50; clamp at 4
        tgt[1, 3, :], tgt[1, 8, :] = (110, 110, -0.9), (118, 112, 0.9)
        tgt[2, 3, :], tgt[2, 8, :] = (110, 110, 0.05), (111.5, 110.5, 0.05)
        tgt[3, 3, :], tgt[3, 8, :] = (40, 40, 0.0), (190, 180, 0.0)
    steer = rng.standard_normal((b, 64)).astype(np.float16)
    steer[:, :63] = (tgt.reshape(b, 63) - bias[:63]).astype(np.float16)
    # the other columns like pooled post-ReLU features: non-negative, mostly zero, multiples of 1/32
    rest = np.where(rng.random((b, 1984)) < 0.7, 0, rng.integers(1, 64, (b, 1984))).astype(np.int8)
    return steer, rest


def _k_per_sample(rng, b):
    k = np.zeros((b, 3, 3), dtype=np.float32)
    k[:, 0, 0] = rng.uniform(250, 600, b)
    k[:, 1, 1] = k[:, 0, 0] * rng.uniform(0.98, 1.02, b)
    k[:, 0, 2] = rng.uniform(90, 134, b)
    k[:, 1, 2] = rng.uniform(90, 134, b)
    k[:, 2, 2] = 1
    return k


def run(dtype, feat, K, G3, G25, Gz):
    """One train-mode forward and backward of the reference in `dtype` -> dict of float64 arrays."""
    m = copy.deepcopy(base).to(dtype).train()
    seq = m.zroot_ref.zroot_ref
    grabbed = {}

    def _grab(key, keep_grad=False):
        def hook(mod, inputs, o):            # (returns None: the output stays the module's own)
            if keep_grad:
                o.retain_grad()
            grabbed[key] = o if keep_grad else o.detach()
        return hook

    hooks = [seq[1].register_forward_hook(_grab("y1")), seq[4].register_forward_hook(_grab("y2")),
             m.zroot_ref.register_forward_hook(_grab("zroot", keep_grad=True))]
    x = torch.from_numpy(feat).to(dtype).requires_grad_(True)
    out = m(x, None if K is None else torch.from_numpy(K).to(dtype))
    fc_out = m.backend_model.fc_out
    g3, g25, gz = (torch.from_numpy(g).to(dtype) for g in (G3, G25, Gz))
    loss = ((out["kp3d"] * g3).sum() + (out["kp25d"].reshape(-1, 63) * g25[:, :63]).sum() + (fc_out[:, 63] * g25[:, 63]).sum()
            + (grabbed["zroot"].reshape(-1) * gz).sum())
    loss.backward()
    for h in hooks:
        h.remove()
    r = {k: out[k].detach() for k in ("kp3d", "kp25d", "kp2d", "zrel")}
    r.update(zroot=grabbed["zroot"].detach().reshape(-1), y1=grabbed["y1"], y2=grabbed["y2"], do=fc_out.grad, dfeat=x.grad,
             dWfc=m.backend_model.fc.weight.grad, dbfc=m.backend_model.fc.bias.grad)
    for k in MLP_KEYS:
        r[k] = dict(seq.named_parameters())[k].grad
    for i in (1, 4):
        r[f"{i}.running_mean"], r[f"{i}.running_var"] = seq[i].running_mean, seq[i].running_var
        r[f"{i}.num_batches_tracked"] = seq[i].num_batches_tracked
    return {k: v.detach().double().numpy() if v.dtype.is_floating_point else v.numpy() for k, v in r.items()}


out = {"K_default": base.K_default.numpy()}
meta = {"cases": [], "margin": {}, "seed": {}, "e_ref": {}, "tries": {},
                 "momentum": [base.zroot_ref.zroot_ref[1].momentum, base.zroot_ref.zroot_ref[4].momentum]}
for b in (2, 5, 37, 67):
    for seed in range(15 * b, 15 * b + 200):
        rng = np.random.default_rng(seed)
        steer, rest = _features(rng, b, b == 5)
        feat = np.concatenate([steer.astype(np.float64), rest.astype(np.float64) / 32], axis=1)
        kps = _k_per_sample(rng, b)
        G = {"G3": rng.integers(-64, 65, (b, 21, 3)).astype(np.int8), "G25": rng.integers(-64, 65, (b, 64)).astype(np.int8),
             "Gz": rng.integers(-64, 65, (b,)).astype(np.int8)}
        Gf = {k: v.astype(np.float64) / 64 for k, v in G.items()}
        runs = {kname: run(torch.float64, feat, K, Gf["G3"], Gf["G25"], Gf["Gz"]) for kname, K in (("default", None), ("per_sample", kps))}
        margin = min(float(np.abs(r[y]).min()) for r in runs.values() for y in ("y1", "y2"))
        if margin >= MARGIN and not any(np.isnan(v).any() for r in runs.values() for v in r.values()):
            break
    else:
        raise SystemExit(f"no seed with margin >= {MARGIN} at B = {b}")
    meta["seed"][str(b)], meta["tries"][str(b)] = seed, seed - 15 * b + 1
    out[f"steer_{b}"], out[f"rest_{b}"], out[f"K_{b}"] = steer, rest, kps
    for k, v in G.items():
        out[f"{k}_{b}"] = v
    for kname, K in (("default", None), ("per_sample", kps)):
        name = f"train_{b}_{kname}"
        g64 = runs[kname]
        g32 = run(torch.float32, feat, K, Gf["G3"], Gf["G25"], Gf["Gz"])
        meta["cases"].append(name)
        meta["margin"][name] = min(float(np.abs(g64[y]).min()) for y in ("y1", "y2"))
        meta["e_ref"][name] = {k: float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max())
                               for k in g64 if g64[k].dtype.kind == "f" and k not in ("y1", "y2") and np.abs(g64[k]).max() > 0}
        assert (g32["1.num_batches_tracked"], g32["4.num_batches_tracked"]) == (g64["1.num_batches_tracked"], g64["4.num_batches_tracked"])
        for k in ("kp25d", "kp3d", "zroot", "do", "0.bias", "1.weight", "1.bias", "3.bias", "4.weight", "4.bias", "6.weight", "6.bias",
                  "1.running_mean", "1.running_var", "4.running_mean", "4.running_var", "1.num_batches_tracked", "4.num_batches_tracked"):
            out[f"{name}/{k}"] = g64[k]
        for k in ("0.weight", "3.weight"):
            U, V = probes(*g64[k].shape)
            out[f"{name}/{k}/left"], out[f"{name}/{k}/right"] = U @ g64[k], g64[k] @ V
            meta.setdefault("max_abs", {}).setdefault(name, {})[k] = float(np.abs(g64[k]).max())
        for y in ("y1", "y2"):
            out[f"{name}/{y}_positive"] = np.packbits(g64[y] > 0, axis=1)

path = os.path.join(HERE, "g15_pose_head_train.npz")
np.savez_compressed(path, **out)
with open(os.path.join(HERE, "g15_pose_head_train.json"), "w") as f:
    json.dump(meta, f, indent=1)
print("wrote g15_pose_head_train.npz:", os.path.getsize(path), "bytes; margins", meta["margin"], "tries", meta["tries"])
