"""Float64 restatement of the supervised pose losses (peclr_amd/pose_loss.py, csrc/pose_loss.hip) with torch autograd on the CPU:
cal_l1_loss and cal_3d_loss over convert_2_5D_to_3D / get_root_depth, written out from their formulas.  The repository's own
text; tests/test_pose_loss_host.py holds it to the reference's float64 results (g14_pose_losses.json, gold64) at 1e-12 of each
tensor's largest magnitude, the GPU tests then use it where the fixture has no entry (B = 261).

Everything is evaluated in float64 from whatever it is given.  The gradients are autograd's: torch.clamp's backward passes the
gradient where the input is >= the minimum, L1's is sign() with sign(0) = 0.
"""
import base64
import json
import os

import numpy as np
import torch

PARENT, CHILD = 0, 2  # wrist, index MCP
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_pose_losses.json")
LOSS_NAMES = ("loss_2d", "loss_z", "loss_z_unscaled", "loss_3d")


def dec(entry):
    """One array of the fixture: {"f32" | "f64": base64 of little-endian bytes, "shape": [...]} (as g13_supervised.json)."""
    kind = "f32" if "f32" in entry else "f64"
    a = np.frombuffer(base64.b64decode(entry[kind]), dtype="<f4" if kind == "f32" else "<f8")
    return a.reshape(entry["shape"]).copy()


def load_fixture():
    with open(GOLDEN) as f:
        return json.load(f)


def case_inputs(case):
    """The float32 inputs of a fixture case as NumPy arrays; `joints_valid` / `z_root_calc` are None where the case has none."""
    out = {k: dec(case[k]) for k in ("pred", "joints", "joints3D", "scale", "K")}
    out["joints_valid"] = dec(case["joints_valid"]) if "joints_valid" in case else None
    out["z_root_calc"] = dec(case["z_root_calc"]) if "z_root_calc" in case else None
    return out


def inverse3(k):
    """[B,3,3] -> its inverse, adjugate over determinant."""
    c = torch.stack([
        torch.stack([k[:, 1, 1] * k[:, 2, 2] - k[:, 1, 2] * k[:, 2, 1], k[:, 0, 2] * k[:, 2, 1] - k[:, 0, 1] * k[:, 2, 2],
                     k[:, 0, 1] * k[:, 1, 2] - k[:, 0, 2] * k[:, 1, 1]], 1),
        torch.stack([k[:, 1, 2] * k[:, 2, 0] - k[:, 1, 0] * k[:, 2, 2], k[:, 0, 0] * k[:, 2, 2] - k[:, 0, 2] * k[:, 2, 0],
                     k[:, 0, 2] * k[:, 1, 0] - k[:, 0, 0] * k[:, 1, 2]], 1),
        torch.stack([k[:, 1, 0] * k[:, 2, 1] - k[:, 1, 1] * k[:, 2, 0], k[:, 0, 1] * k[:, 2, 0] - k[:, 0, 0] * k[:, 2, 1],
                     k[:, 0, 0] * k[:, 1, 1] - k[:, 0, 1] * k[:, 1, 0]], 1)], 1)
    det = k[:, 0, 0] * c[:, 0, 0] + k[:, 0, 1] * c[:, 1, 0] + k[:, 0, 2] * c[:, 2, 0]
    return c / det.view(-1, 1, 1)


def root_depth(pred, inv):
    """get_root_depth on [B,21,3] joints with the inverse camera matrices [B,3,3] -> [B]; both clamp(min=1e-6)."""
    def ray(j):
        return inv[:, 0, 0] * pred[:, j, 0] + inv[:, 0, 1] * pred[:, j, 1] + inv[:, 0, 2], \
            inv[:, 1, 0] * pred[:, j, 0] + inv[:, 1, 1] * pred[:, j, 1] + inv[:, 1, 2]

    (xn, yn), (xm, ym) = ray(PARENT), ray(CHILD)
    zn, zm = pred[:, PARENT, 2], pred[:, CHILD, 2]
    a = (xn - xm) ** 2 + (yn - ym) ** 2
    b = 2 * (zn * (xn ** 2 + yn ** 2 - xn * xm - yn * ym) + zm * (xm ** 2 + ym ** 2 - xn * xm - yn * ym))
    c = (xn * zn - xm * zm) ** 2 + (yn * zn - ym * zm) ** 2 + (zn - zm) ** 2 - 1
    return 0.5 * (-b + torch.clamp(b ** 2 - 4 * a * c, min=1e-6) ** 0.5) / torch.clamp(a, min=1e-6)


def lift(pred, scale, k, z_root_calc=None):
    """convert_2_5D_to_3D(pred, scale, K, is_batch=True, Z_root_calc) -> [B,21,3]."""
    inv = inverse3(k)
    z_root = root_depth(pred, inv) if z_root_calc is None else z_root_calc
    depth = (pred[:, :, 2:] + z_root.view(-1, 1, 1)) * scale.view(-1, 1, 1)
    hom = torch.cat((pred[:, :, :2], torch.ones_like(pred[:, :, 2:])), 2)
    return torch.bmm(hom, inv.transpose(1, 2)) * depth


def losses(pred, joints, joints3d, scale, k, joints_valid=None, z_root_calc=None):
    """The four losses as a [4] tensor: cal_l1_loss's three, then cal_3d_loss."""
    valid = torch.ones_like(joints[..., -1:]) if joints_valid is None else joints_valid
    weight = valid / valid.sum()
    loss_2d = ((pred[..., :2] - joints[..., :2]).abs() * weight).sum() / 2
    loss_z = (pred[..., 2:] - joints[..., 2:]).abs() * weight
    loss_zu = (loss_z * scale.view(-1, 1, 1)).sum()
    loss_3 = ((lift(pred, scale, k, z_root_calc) - joints3d).abs() * weight).sum() / 3
    return torch.stack((loss_2d, loss_z.sum(), loss_zu, loss_3))


def losses_and_grads(inputs, weights):
    """inputs: the dict of `case_inputs` (any float arrays) -> (losses [4], d(w . losses)/d pred [B,21,3], d/d z_root_calc [B] or
    None), float64 NumPy arrays."""
    t = {k: None if v is None else torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in inputs.items()}
    pred = t["pred"].clone().requires_grad_(True)
    zc = None if t["z_root_calc"] is None else t["z_root_calc"].clone().requires_grad_(True)
    out = losses(pred, t["joints"], t["joints3D"], t["scale"], t["K"], t["joints_valid"], zc)
    (out * torch.tensor(weights, dtype=torch.float64)).sum().backward()
    return out.detach().numpy(), pred.grad.numpy(), None if zc is None else zc.grad.numpy()
