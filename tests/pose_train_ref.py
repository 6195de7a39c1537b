"""Float64 NumPy restatement of the 2.5D pose head in train mode and of its backward, formula for formula as the kernels of
peclr_amd/csrc/pose_train.hip state them (reference: RN_25D_wMLPref.forward and ZrootMLP_ref.forward with BatchNorm1d on batch
statistics).  tests/test_pose_train_host.py holds it to the reference's own float64 run recorded in
tests/golden/g15_pose_head_train.npz; the GPU tests use it where the fixture records no tensor (the large weight gradients)."""
import numpy as np

NJ = 21
SLOPE = 0.01
MLP_KEYS = ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias", "6.weight", "6.bias")


def _bn_fwd(p, gamma, beta, eps):
    mean = p.mean(0)
    var = ((p - mean) ** 2).mean(0)                 # biased: what normalises
    invstd = 1.0 / np.sqrt(var + eps)
    xhat = (p - mean) * invstd
    return xhat * gamma + beta, xhat, invstd, mean, var


def forward(feat, K, fc_w, fc_b, mlp, bn_eps=(1e-5, 1e-5), eps=1e-8):
    """feat [B,2048], K [B or 1,3,3], mlp: dict of the ten parameters by MLP_KEYS -- all float64.  Returns (outputs, cache):
    outputs has out64, kp25d, kp2d, zrel, kp3d, zroot and the batch statistics mean1, var1, mean4, var4 (var biased)."""
    feat, K = np.asarray(feat, np.float64), np.asarray(K, np.float64)
    b = feat.shape[0]
    o = feat @ fc_w.T + fc_b
    o[:, 2] = 0.0
    kp25d = o[:, :63].reshape(b, NJ, 3)
    kinv = np.broadcast_to(np.linalg.inv(K), (b, 3, 3))
    uv1 = np.concatenate([kp25d[..., :2], np.ones((b, NJ, 1))], axis=2)
    ku = np.einsum("bjc,brc->bjr", uv1, kinv)
    zrel = kp25d[..., 2]
    xm, ym, xn, yn, zm, zn = ku[:, 3, 0], ku[:, 3, 1], ku[:, 8, 0], ku[:, 8, 1], zrel[:, 3], zrel[:, 8]
    a = (xn - xm) ** 2 + (yn - ym) ** 2
    bq = 2 * (zn * (xn ** 2 + yn ** 2 - xn * xm - yn * ym) + zm * (xm ** 2 + ym ** 2 - xn * xm - yn * ym))
    c = (xn * zn - xm * zm) ** 2 + (yn * zn - ym * zm) ** 2 + (zn - zm) ** 2 - 1
    d = bq ** 2 - 4 * a * c
    zr = np.clip((-bq + np.sqrt(np.maximum(d, eps))) / (2 * np.maximum(a, eps)), 4.0, 50.0)     # detached: no backward
    x = np.concatenate([zrel, ku[..., :2].reshape(b, 42), zr[:, None]], axis=1)
    y1, xhat1, invstd1, mean1, var1 = _bn_fwd(x @ mlp["0.weight"].T + mlp["0.bias"], mlp["1.weight"], mlp["1.bias"], bn_eps[0])
    h1 = np.where(y1 > 0, y1, SLOPE * y1)
    y2, xhat2, invstd2, mean4, var4 = _bn_fwd(h1 @ mlp["3.weight"].T + mlp["3.bias"], mlp["4.weight"], mlp["4.bias"], bn_eps[1])
    h2 = np.where(y2 > 0, y2, SLOPE * y2)
    zroot = zr + (h2 @ mlp["6.weight"].T)[:, 0] + mlp["6.bias"][0]
    kp3d = ku * (zrel + zroot[:, None])[..., None]
    out = {"out64": o, "kp25d": kp25d, "kp2d": kp25d[..., :2], "zrel": kp25d[..., 2:3], "kp3d": kp3d, "zroot": zroot,
           "mean1": mean1, "var1": var1, "mean4": mean4, "var4": var4, "y1": y1, "y2": y2}
    cache = dict(feat=feat, kinv=kinv, ku=ku, zrel=zrel, zroot=zroot, x=x, y1=y1, xhat1=xhat1, invstd1=invstd1, h1=h1, y2=y2,
                 xhat2=xhat2, invstd2=invstd2, h2=h2, fc_w=fc_w, mlp=mlp)
    return out, cache


def running_stats(running_mean, running_var, mean, var_biased, b, momentum=0.1):
    """BatchNorm's update: the batch variance enters unbiased."""
    return ((1 - momentum) * running_mean + momentum * mean, (1 - momentum) * running_var + momentum * var_biased * b / (b - 1))


def _bn_bwd(dy, xhat, invstd, gamma):
    b = dy.shape[0]
    dgamma, dbeta = (dy * xhat).sum(0), dy.sum(0)
    return gamma * invstd / b * (b * dy - dbeta - xhat * dgamma), dgamma, dbeta


def backward(cache, g_kp3d=None, g_out64=None, g_zroot=None):
    """Upstream gradients (None = zeros) -> dict: do [B,64], dfeat, dWfc, dbfc and the ten MLP gradients by MLP_KEYS."""
    c, mlp = cache, cache["mlp"]
    b = c["x"].shape[0]
    g3 = np.zeros((b, NJ, 3)) if g_kp3d is None else np.asarray(g_kp3d, np.float64)
    g25 = np.zeros((b, 64)) if g_out64 is None else np.asarray(g_out64, np.float64)
    gz = np.zeros(b) if g_zroot is None else np.asarray(g_zroot, np.float64)
    a = (g3 * c["ku"]).sum(2)                                   # [B,21]
    dzroot = gz + a.sum(1)
    dzrel = a.copy()
    dku = g3 * (c["zrel"] + c["zroot"][:, None])[..., None]
    g = {}
    g["6.weight"] = (dzroot[:, None] * c["h2"]).sum(0)[None, :]
    g["6.bias"] = dzroot.sum(keepdims=True)
    dh2 = dzroot[:, None] * mlp["6.weight"]
    dy2 = np.where(c["y2"] > 0, dh2, SLOPE * dh2)               # y == 0: the slope, as torch
    dp2, g["4.weight"], g["4.bias"] = _bn_bwd(dy2, c["xhat2"], c["invstd2"], mlp["4.weight"])
    g["3.weight"], g["3.bias"] = dp2.T @ c["h1"], dp2.sum(0)
    dh1 = dp2 @ mlp["3.weight"]
    dy1 = np.where(c["y1"] > 0, dh1, SLOPE * dh1)
    dp1, g["1.weight"], g["1.bias"] = _bn_bwd(dy1, c["xhat1"], c["invstd1"], mlp["1.weight"])
    g["0.weight"], g["0.bias"] = dp1.T @ c["x"], dp1.sum(0)
    dx = dp1 @ mlp["0.weight"]
    dzrel += dx[:, :NJ]
    dku[..., :2] += dx[:, NJ:63].reshape(b, NJ, 2)             # dx[:, 63] dropped: zr is detached
    duv = np.einsum("bjr,brc->bjc", dku, c["kinv"])[..., :2]
    do = g25.copy()
    do3 = do[:, :63].reshape(b, NJ, 3)                          # a view
    do3[..., :2] += duv
    do3[..., 2] += dzrel
    do[:, 2] = 0.0
    g.update(fc_grads(do, c["feat"], c["fc_w"]))
    g["do"] = do
    return g


def fc_grads(do, feat, fc_w):
    """The fc layer's gradients from the gradient at its output: plain linear algebra."""
    do, feat = np.asarray(do, np.float64), np.asarray(feat, np.float64)
    return {"dWfc": do.T @ feat, "dbfc": do.sum(0), "dfeat": do @ np.asarray(fc_w, np.float64)}


# ------------------------------------------------------------------ the fixture (tests/golden/make_golden_pose_train.py)
def load_fixture(golden_dir):
    import json
    import os

    with open(os.path.join(golden_dir, "g15_pose_head_train.json")) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(golden_dir, "g15_pose_head_train.npz"))), dict(np.load(os.path.join(golden_dir, "g11_pose.npz")))


def probes(n_out, n_in):
    """The generator's fixed probe vectors U [2, n_out], V [n_in, 2] for the two matrix gradients."""
    U = np.stack([np.cos(0.37 * (k + 1) * np.arange(n_out) + k) for k in range(2)])
    V = np.stack([np.sin(0.53 * (k + 1) * np.arange(n_in) + 2 * k) for k in range(2)], axis=1)
    return U, V


def case_inputs(npz, g11, name):
    """Float64 inputs of case `train_<B>_<default|per_sample>`: feat, K, G3, G25, Gz, fc_w, fc_b, mlp, and the initial
    running statistics rm1, rv1, rm4, rv4."""
    _, b, kname = name.split("_", 2)
    feat = np.concatenate([npz[f"steer_{b}"].astype(np.float64), npz[f"rest_{b}"].astype(np.float64) / 32], axis=1)
    K = (npz["K_default"] if kname == "default" else npz[f"K_{b}"]).astype(np.float64)
    w = "w/zroot_ref.zroot_ref."
    return dict(feat=feat, K=K, G3=npz[f"G3_{b}"] / 64.0, G25=npz[f"G25_{b}"] / 64.0, Gz=npz[f"Gz_{b}"] / 64.0,
                fc_w=g11["w/backend_model.fc.weight"].astype(np.float64), fc_b=g11["w/backend_model.fc.bias"].astype(np.float64),
                mlp={k: g11[w + k].astype(np.float64) for k in MLP_KEYS}, rm1=g11[w + "1.running_mean"].astype(np.float64),
                rv1=g11[w + "1.running_var"].astype(np.float64), rm4=g11[w + "4.running_mean"].astype(np.float64),
                rv4=g11[w + "4.running_var"].astype(np.float64))


def restated_case(npz, g11, name, momentum=0.1):
    """Forward and backward of the restatement on a case -> dict tensor name (the fixture's names) -> float64 array."""
    c = case_inputs(npz, g11, name)
    out, cache = forward(c["feat"], c["K"], c["fc_w"], c["fc_b"], c["mlp"])
    r = backward(cache, c["G3"], c["G25"], c["Gz"])
    r.update({k: out[k] for k in ("kp25d", "kp2d", "zrel", "kp3d", "zroot", "y1", "y2")})
    r["zr"] = cache["x"][:, 63]
    b = c["feat"].shape[0]
    r["1.running_mean"], r["1.running_var"] = running_stats(c["rm1"], c["rv1"], out["mean1"], out["var1"], b, momentum)
    r["4.running_mean"], r["4.running_var"] = running_stats(c["rm4"], c["rv4"], out["mean4"], out["var4"], b, momentum)
    return r
