"""Golden vectors for the supervised pose losses (peclr_amd/pose_loss.py, csrc/pose_loss.hip).

Run where the reference checkout is present (tests/golden/_ref_import.py names its place):

    python tests/golden/make_golden_losses.py

Calls the reference's own `cal_l1_loss` and `cal_3d_loss` (src/models/utils.py) and differentiates them with autograd.

Fixture: g14_pose_losses.json.  Arrays are base64 of little-endian float32 / float64 bytes ({"f32": ...} / {"f64": ...}, with
"shape"), as in g13_supervised.json.  `weights`: the two weight vectors w over (loss_2d, loss_z, loss_z_unscaled, loss_3d).
Per case:

  inputs   pred, joints, joints3D [B,21,3], scale [B], K [B,3,3] float32; joints_valid [B,21,1] and z_root_calc [B] where used
  gold64   the reference on .double() copies of those tensors: losses [4]; grad_pred [2,B,21,3] = d(w . losses)/d pred for
           either w; grad_z_root_calc [2,B] where z_root_calc is used
  gold32   the same from the float32 tensors themselves

Inputs: synthetic hands as `hands()` of tests/test_supervised_gpu.py makes them (focal 480, 224 x 224), truth from the
reference's `convert_to_2_5D`, pred = truth + normal noise of 4 px in u and v and 0.15 in z, joints_valid random 0 / 1 with
about 20 % zeros (None in one case).  The noise of a joint is drawn again, and a case's seed advanced, until the case satisfies
what is asserted below, which is part of the fixture's contract:

  * outside the tied joint of "ties", every difference a sign is taken of (pred - joints in uv and in z, the lifted pred -
    joints3D) exceeds 1e-3 of the largest such difference of its tensor in that sample (per sample: the clamped root depth of
    "clamps" puts one sample's 3D differences four orders above the others'), in float64 and in float32: no sign hangs on a
    last bit;
  * outside "clamps", the leading coefficient `a` and the discriminant of get_root_depth exceed 1e-3 in both precisions.
"""
import base64
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

_ref_import.install_stubs()
from src.data_loader.utils import (convert_2_5D_to_3D, convert_to_2_5D, get_root_depth,  # noqa: E402
                                   get_zroot_constraint_terms)
from src.models.utils import cal_3d_loss, cal_l1_loss  # noqa: E402

WEIGHTS = [[1.0, 1.0, 0.0, 1.0], [0.5, 2.0, 3.0, 0.25]]
MARGIN = 1e-3


def enc(t):
    a = t.detach().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = np.ascontiguousarray(a)
    kind = {np.dtype("float32"): "f32", np.dtype("float64"): "f64"}[a.dtype]
    return {kind: base64.b64encode(a.astype(a.dtype.newbyteorder("<")).tobytes()).decode(), "shape": list(a.shape)}


def hands(n, seed, hw=(224, 224), focal=480.0):
    """n synthetic hands -> (K [n,3,3], joints3D [n,21,3]) float32 NumPy arrays (tests/test_supervised_gpu.py: hands)."""
    g = np.random.default_rng(seed)
    k = np.array([[focal, 0, hw[1] / 2], [0, focal, hw[0] / 2], [0, 0, 1]], dtype=np.float32)
    out = []
    for _ in range(n):
        z = 0.6 + 0.05 * g.standard_normal(21)
        u = g.uniform(0.35, 0.65) * hw[1] + min(hw) / 9 * g.standard_normal(21)
        v = g.uniform(0.35, 0.65) * hw[0] + min(hw) / 9 * g.standard_normal(21)
        out.append(np.stack([(u - k[0, 2]) * z / focal, (v - k[1, 2]) * z / focal, z], axis=1))
    return np.repeat(k[None], n, 0), np.array(out, dtype=np.float32)


def quadratic(pred, k):
    """(a, b^2 - 4ac) of get_root_depth for a batch, in the dtype given."""
    x_n, y_n, z_n, x_m, y_m, z_m, c_ = get_zroot_constraint_terms(pred, torch.inverse(k), True)
    a = (x_n - x_m) ** 2 + (y_n - y_m) ** 2
    b = 2 * (z_n * (x_n ** 2 + y_n ** 2 - x_n * x_m - y_n * y_m) + z_m * (x_m ** 2 + y_m ** 2 - x_n * x_m - y_n * y_m))
    c = (x_n * z_n - x_m * z_m) ** 2 + (y_n * z_n - y_m * z_m) ** 2 + (z_n - z_m) ** 2 - c_
    return a, b ** 2 - 4 * a * c


def evaluate(t, weights):
    """The reference's losses and the gradients of w . losses, in the dtype of the tensors of `t`."""
    pred = t["pred"].clone().requires_grad_(True)
    zc = None if t["z_root_calc"] is None else t["z_root_calc"].clone().requires_grad_(True)
    l2d, lz, lzu = cal_l1_loss(pred, t["joints"], t["scale"], t["joints_valid"])
    l3d = cal_3d_loss(pred, t["joints3D"], t["scale"], t["K"],
                      torch.ones_like(pred[..., -1:]) if t["joints_valid"] is None else t["joints_valid"], zc)
    (weights[0] * l2d + weights[1] * lz + weights[2] * lzu + weights[3] * l3d).backward()
    return torch.stack((l2d, lz, lzu, l3d)).detach(), pred.grad.clone(), None if zc is None else zc.grad.clone()


def sign_margins(t, tied):
    """[B,21] bool: the joints with a difference whose sign is taken below MARGIN x the largest of its tensor in the sample."""
    d = (t["pred"] - t["joints"]).abs()
    lifted = convert_2_5D_to_3D(t["pred"], t["scale"], t["K"], True, t["z_root_calc"])
    d3 = (lifted - t["joints3D"]).abs()
    top = lambda x: x.reshape(x.shape[0], -1).max(1).values.view(-1, 1, 1)  # noqa: E731
    bad_l1 = (d[..., :2] <= MARGIN * top(d[..., :2])).any(-1) | (d[..., 2] <= MARGIN * top(d[..., 2:])[..., 0])
    if tied is not None:
        bad_l1[tied] = False
    return bad_l1 | (d3 <= MARGIN * top(d3)).any(-1)


def quadratic_holds(t, kind):
    a, disc = quadratic(t["pred"], t["K"])
    if kind != "clamps":
        return bool((a > MARGIN).all()) and bool((disc > MARGIN).all())
    z_root, _ = get_root_depth(t["pred"], t["K"], True)
    ok = bool(a[0] == 0) and bool(disc[0] < 1e-6) and abs(float(z_root[0]) - 500.0) < 1e-2
    ok = ok and bool(a[1] > MARGIN) and bool(disc[1] < -MARGIN)
    return ok and bool(a[2] > MARGIN) and bool(disc[2] > MARGIN)


def doubles(t):
    return {k: None if v is None else v.double() for k, v in t.items()}


def build(b, seed, kind, valid_none):
    """One candidate of a case -> (the float32 tensors, the tied joint, whether every margin holds).  The noise of a joint
    with a difference inside the sign margin is drawn again (a joint other than 0 and 2 moves nothing but itself)."""
    k_np, j_np = hands(b, seed)
    g = np.random.default_rng(seed + 5000)
    K, J = torch.from_numpy(k_np), torch.from_numpy(j_np)
    truth, scale = zip(*(convert_to_2_5D(K[i], J[i]) for i in range(b)))
    joints, scale = torch.stack(truth), torch.stack(scale)
    sd = np.array([4.0, 4.0, 0.15])
    noise = g.standard_normal((b, 21, 3)) * sd
    valid = None if valid_none else torch.from_numpy((g.uniform(size=(b, 21, 1)) >= 0.2).astype(np.float32))
    tied = (b - 1, 7) if kind == "ties" else None
    if kind == "clamps":
        valid[:, (0, 2)] = 1.0
    elif kind == "ties":
        valid[tied[0], tied[1]] = 1.0
    elif kind == "no_valid":
        valid = torch.zeros((b, 21, 1))
    for _ in range(100):
        pred = (joints.double() + torch.from_numpy(noise)).float()
        if kind == "clamps":
            pred[0, 2, :2] = pred[0, 0, :2]          # index MCP on the wrist's pixel: a = 0, both clamps active
            pred[1, 2, 2] = pred[1, 0, 2] + 3.0      # a bone three scale units deep: negative discriminant
        elif kind == "ties":
            pred[tied] = joints[tied]
        t = {"pred": pred, "joints": joints, "joints3D": J, "scale": scale, "K": K, "joints_valid": valid, "z_root_calc": None}
        if kind == "z_root_calc":
            t["z_root_calc"] = (get_root_depth(pred, K, True)[0] + 0.3).float()
        bad = (sign_margins(t, tied) | sign_margins(doubles(t), tied)).numpy()
        if not bad.any():
            return t, tied, quadratic_holds(t, kind) and quadratic_holds(doubles(t), kind)
        noise[bad] = g.standard_normal((int(bad.sum()), 3)) * sd
    return t, tied, False


def run_case(name, b, seed, kind="plain", valid_none=False):
    for attempt in range(200):
        t32, tied, ok = build(b, seed + 100 * attempt, kind, valid_none)
        if ok:
            break
    else:
        raise SystemExit(f"{name}: no seed satisfies the margins")
    t64 = doubles(t32)
    for v in t32.values():
        assert v is None or v.dtype == torch.float32
    case = {"name": name, "kind": kind, "seed": seed + 100 * attempt, "B": b}
    if tied is not None:
        case["tied"] = list(tied)
    for key, v in t32.items():
        if v is not None:
            case[key] = enc(v)
    for gold, t in (("gold32", t32), ("gold64", t64)):
        runs = [evaluate(t, w) for w in WEIGHTS]
        assert torch.equal(runs[0][0], runs[1][0]) or kind == "no_valid"
        out = {"losses": enc(runs[0][0]), "grad_pred": enc(torch.stack([r[1] for r in runs]))}
        if t["z_root_calc"] is not None:
            out["grad_z_root_calc"] = enc(torch.stack([r[2] for r in runs]))
        case[gold] = out
    if kind == "no_valid":
        assert bool(torch.isnan(runs[0][0]).all())
    return case


def main():
    torch.set_num_threads(1)
    cases = [run_case("b1", 1, 301), run_case("b3", 3, 303), run_case("b4_valid_none", 4, 304, valid_none=True),
             run_case("b5", 5, 305), run_case("b9", 9, 309), run_case("z_root_calc", 3, 313, "z_root_calc"),
             run_case("clamps", 3, 323, "clamps"), run_case("ties", 2, 332, "ties"), run_case("no_valid", 2, 342, "no_valid")]
    doc = {"weights": WEIGHTS, "loss_names": ["loss_2d", "loss_z", "loss_z_unscaled", "loss_3d"], "cases": cases}
    path = os.path.join(HERE, "g14_pose_losses.json")
    with open(path, "w") as f:
        json.dump(doc, f)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases")
    for c in cases:
        print(c["name"], c["B"], c["seed"], _ref_losses(c))


def _ref_losses(case):
    e = case["gold64"]["losses"]
    return np.frombuffer(base64.b64decode(e["f64"]), dtype="<f8").tolist()


if __name__ == "__main__":
    main()
