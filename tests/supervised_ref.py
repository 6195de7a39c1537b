"""Float64 NumPy restatement of the supervised sample's label side (peclr_amd/supervised.py, csrc/labels.hip): the three
conversions of the reference's data_loader/utils.py and the label chain of Data_Set.prepare_supervised_sample.  The
repository's own text; tests/test_supervised_host.py holds it to the reference's float64 results (g13_supervised.json, gold64)
at 1e-12 relative, the GPU tests then use it as the yardstick of what the device computes.

Everything is evaluated in float64 from whatever it is given; `label_chain` rounds each emitted tensor to float32 once and lets
the next stage read the rounded tensor, which is the kernel's arithmetic contract.
"""
import base64
import json
import os

import numpy as np

PARENT, CHILD = 0, 2  # wrist, index MCP
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_supervised.json")


def dec(entry):
    """One array of g13_supervised.json: {"f32" | "f64": base64 of little-endian bytes, "shape": [...]}."""
    kind = "f32" if "f32" in entry else "f64"
    a = np.frombuffer(base64.b64decode(entry[kind]), dtype="<f4" if kind == "f32" else "<f8")
    return a.reshape(entry["shape"]).copy()


def load_fixture():
    with open(GOLDEN) as f:
        return json.load(f)


def to_25d(k, j3d):
    """convert_to_2_5D for one sample: k [3,3], j3d [21,3] -> (joints25d [21,3], scale)."""
    k, j3d = np.asarray(k, np.float64), np.asarray(j3d, np.float64)
    scale = np.sqrt(((j3d[CHILD] - j3d[PARENT]) ** 2).sum())
    out = (j3d @ k.T) / j3d[:, 2:]
    out[:, 2] = (j3d[:, 2] - j3d[PARENT, 2]) / scale
    return out, scale


def inverse3(k):
    """Adjugate over determinant."""
    k = np.asarray(k, np.float64)
    c = np.array([[k[1, 1] * k[2, 2] - k[1, 2] * k[2, 1], k[0, 2] * k[2, 1] - k[0, 1] * k[2, 2], k[0, 1] * k[1, 2] - k[0, 2] * k[1, 1]],
                  [k[1, 2] * k[2, 0] - k[1, 0] * k[2, 2], k[0, 0] * k[2, 2] - k[0, 2] * k[2, 0], k[0, 2] * k[1, 0] - k[0, 0] * k[1, 2]],
                  [k[1, 0] * k[2, 1] - k[1, 1] * k[2, 0], k[0, 1] * k[2, 0] - k[0, 0] * k[2, 1], k[0, 0] * k[1, 1] - k[0, 1] * k[1, 0]]])
    det = k[0, 0] * c[0, 0] - k[0, 1] * (k[1, 0] * k[2, 2] - k[1, 2] * k[2, 0]) + k[0, 2] * c[2, 0]
    return c / det


def root_depth(j25d, k):
    """get_root_depth for one sample, with the two clamp(min=1e-6)."""
    j25d = np.asarray(j25d, np.float64)
    inv = inverse3(k)
    xn, yn, _ = inv @ np.array([j25d[PARENT, 0], j25d[PARENT, 1], 1.0])
    xm, ym, _ = inv @ np.array([j25d[CHILD, 0], j25d[CHILD, 1], 1.0])
    zn, zm = j25d[PARENT, 2], j25d[CHILD, 2]
    a = (xn - xm) ** 2 + (yn - ym) ** 2
    b = 2 * (zn * (xn ** 2 + yn ** 2 - xn * xm - yn * ym) + zm * (xm ** 2 + ym ** 2 - xn * xm - yn * ym))
    c = (xn * zn - xm * zm) ** 2 + (yn * zn - ym * zm) ** 2 + (zn - zm) ** 2 - 1.0
    disc = b ** 2 - 4 * a * c
    return 0.5 * (-b + np.sqrt(disc if not disc < 1e-6 else 1e-6)) / (a if not a < 1e-6 else 1e-6)


def to_3d(j25d, scale, k, z_root_calc=None):
    """convert_2_5D_to_3D for one sample -> (joints3d [21,3], the quadratic's root depth)."""
    j25d = np.asarray(j25d, np.float64)
    zr = root_depth(j25d, k)
    z = (j25d[:, 2:] + (zr if z_root_calc is None else np.float64(z_root_calc))) * np.float64(scale)
    hom = j25d.copy()
    hom[:, 2] = 1.0
    return (hom @ inverse3(k).T) * z, zr


def move_wrist_to_palm(j3d):
    out = np.array(j3d, np.float64)
    out[PARENT] = (out[PARENT] + out[CHILD]) / 2
    return out


def f32(a):
    """One rounding to float32, read back as float64."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def label_chain(k, j3d, T, use_palm=False, joints_raw=None):
    """The label side for one sample: k, j3d (and joints_raw) float32 values, T float64 -> dict of float64 arrays holding
    float32 values (each emitted tensor rounded once; a later stage reads the rounded tensor)."""
    k, j3d, T = np.asarray(k, np.float64), np.asarray(j3d, np.float64), np.asarray(T, np.float64)
    raw = j3d if joints_raw is None else np.asarray(joints_raw, np.float64)
    t32 = f32(T)
    k_new = f32(t32 @ k)
    if use_palm:
        j3d_out, raw_out = f32(move_wrist_to_palm(j3d)), f32(move_wrist_to_palm(raw))
        joints, scale = to_25d(k_new, j3d_out)
    else:
        j3d_out, raw_out = j3d, raw
        joints, scale = to_25d(k, j3d)
        hom = joints.copy()
        hom[:, 2] = 1.0
        joints[:, :2] = (hom @ T.T)[:, :2]
    joints, scale = f32(joints), f32(scale)
    rec, _ = to_3d(joints, scale, k_new)
    return {"joints": joints, "K": k_new, "scale": scale, "joints3D": j3d_out, "joints3D_recreated": f32(rec),
            "joints_raw": raw_out, "T": t32}
