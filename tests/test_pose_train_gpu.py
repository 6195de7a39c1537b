"""The 2.5D pose head in train mode on the HIP kernels (csrc/pose_train.hip): forward and backward against the reference's own
float64 run (tests/golden/g15_pose_head_train.npz; the tensors the fixture does not record come from the float64 restatement
that tests/test_pose_train_host.py holds to it), against the stock torch composition on the same device, determinism, options,
and one step of the whole model.

Metric, per tensor: e(t) = max|t - gold64| / max|gold64|; bound: e(dev) <= max(1e-5, C e_ref) with e_ref = e(gold32), the
reference's own float32 deviation (recorded by the fixture's generator).  1e-5 is the project's bound for this head in
test_pose_gpu.py::test_head_kernel_matches_the_reference.

C = 8, the largest constant the bound admits for an fp32 kernel of the same formulas.  Measured on MI355X
(profiles/pose_head_train_parity.txt): e(dev) exceeds the 1e-5 floor mostly at B = 2, where batch statistics of two samples
amplify the fp32 rounding of the MLP input by up to 1 / sqrt(eps).  There train_2_default has every gradient behind a BatchNorm
at 3.5 ... 5.2 times e_ref (worst: 6.weight, 4.11e-5 against 7.86e-6; `do` 1.33e-4 against 3.74e-5), train_2_per_sample -- the
same features under another K -- at 0.5 ... 0.9 times; at B >= 5 no ratio above the floor exceeds 0.95.  "Twice the worst
ratio" would ask for C = 16: the recipe's condition (C <= 8) is NOT met by that one case, and C stays at its cap.  The same
case with other summations inside the kernel, `do`: fp32 batch statistics 3.0e-4; as committed (float64 batch reductions, xhat
formed in float64 from the saved pre-activation) 1.3e-4; with float64 sums for the pre-activations too 1.9e-4 -- the figure
follows the draw of the input rounding, not the accuracy of the kernel's own sums.  Below the floor the closed-form root depth
(fp32, shared bit for bit with the evaluation head) is up to 22 times the reference's deviation where that happens to be under
one ulp (train_5_default zroot: 1.1e-6 against 5.1e-8)."""
import copy
import os
import random

import numpy as np
import pytest
import torch

from tests import pose_train_ref as ref
from tests.conftest import ROOT
from tests.test_pose_host import golden_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(ROOT, "tests", "golden")
C = 8.0
FLOOR = 1e-5
META, NPZ, G11 = ref.load_fixture(GOLDEN)
CASES = META["cases"]
SEQ = "zroot_ref.zroot_ref."
ZERO_BIAS = {"0.bias": "0.weight", "3.bias": "3.weight"}      # in front of a train-mode BatchNorm: mathematically 0


@pytest.fixture(scope="module")
def base_model():
    m = golden_model(G11).to(DEV).enable_hip().enable_hip_training().train()
    for p in m.backend_model.parameters():
        p.requires_grad_(False)
    for p in m.backend_model.fc.parameters():
        p.requires_grad_(True)
    return m


@pytest.fixture()
def model(base_model):
    """The module's model with g11's head state (running statistics, counters) restored and no gradients."""
    sd = base_model.state_dict()
    with torch.no_grad():
        for k, v in sd.items():
            if k.startswith(SEQ):
                v.copy_(torch.from_numpy(np.asarray(G11["w/" + k])))
    for p in base_model.parameters():
        p.grad = None
    return base_model


def dev_inputs(name, feat_grad=True):
    c = ref.case_inputs(NPZ, G11, name)
    t = {k: torch.from_numpy(c[k]).float().to(DEV) for k in ("feat", "K", "G3", "G25", "Gz")}
    t["feat"].requires_grad_(feat_grad)
    return t


def run_case(model, name, feat_grad=True, g3=True, g25=True, gz=True):
    """Forward and backward of the model's head on a case -> (out, dict of gradients by the fixture's names)."""
    t = dev_inputs(name, feat_grad)
    out = model.head(t["feat"], t["K"])
    terms = []
    if g3:
        terms.append((out["kp3d"] * t["G3"]).sum())
    if g25:
        terms.append((out["kp25d"].reshape(-1, 63) * t["G25"][:, :63]).sum())
    if gz:
        terms.append((out["zroot"] * t["Gz"]).sum())
    sum(terms).backward()
    seq = dict(model.zroot_ref.zroot_ref.named_parameters())
    g = {k: seq[k].grad for k in ref.MLP_KEYS}
    g.update(dWfc=model.backend_model.fc.weight.grad, dbfc=model.backend_model.fc.bias.grad, dfeat=t["feat"].grad)
    return out, g


def err(dev, gold, scale=None):
    gold = np.asarray(gold, np.float64)
    dev = dev.detach().double().cpu().numpy().reshape(gold.shape)
    return float(np.abs(dev - gold).max() / (np.abs(gold).max() if scale is None else scale))


def hold(case, key, e_dev, e_ref):
    """Print the figures (profiles/pose_head_train_parity.txt is made of these lines), assert the bound."""
    ratio = e_dev / e_ref
    print(f"parity {case} {key}: e_dev = {e_dev:.3e} e_ref = {e_ref:.3e} ratio = {ratio:.3f}")
    assert e_dev <= max(FLOOR, C * e_ref), (case, key, e_dev, e_ref)


def gold_of(name):
    """gold64 of a case: the recorded tensors, and the restatement's for those the fixture leaves out."""
    r = ref.restated_case(NPZ, G11, name, META["momentum"][0])
    gold = {k: r[k] for k in ("0.weight", "3.weight", "dWfc", "dbfc", "dfeat")}
    for k in ("kp25d", "kp3d", "zroot", "do", "0.bias", "1.weight", "1.bias", "3.bias", "4.weight", "4.bias", "6.weight", "6.bias",
              "1.running_mean", "1.running_var", "4.running_mean", "4.running_var"):
        gold[k] = NPZ[f"{name}/{k}"]
    gold["kp2d"], gold["zrel"] = gold["kp25d"][..., :2], gold["kp25d"][..., 2:3]
    return gold


# ------------------------------------------------------------------ 1. forward parity
@pytest.mark.parametrize("name", CASES)
def test_forward_matches_the_reference(model, name):
    t = dev_inputs(name, feat_grad=False)
    assert model.hip_train_path(t["feat"])
    out = model.head(t["feat"], t["K"])
    gold, e_ref = gold_of(name), META["e_ref"][name]
    assert sorted(out) == ["kp25d", "kp2d", "kp3d", "zrel", "zroot"]
    for key in ("kp3d", "kp25d", "kp2d", "zrel", "zroot"):
        hold(name, key, err(out[key], gold[key]), e_ref[key])
    seq = model.zroot_ref.zroot_ref
    for i in (1, 4):
        hold(name, f"{i}.running_mean", err(seq[i].running_mean, gold[f"{i}.running_mean"]), e_ref[f"{i}.running_mean"])
        hold(name, f"{i}.running_var", err(seq[i].running_var, gold[f"{i}.running_var"]), e_ref[f"{i}.running_var"])
        assert seq[i].num_batches_tracked.item() == int(NPZ[f"{name}/{i}.num_batches_tracked"]) == int(G11[f"w/{SEQ}{i}.num_batches_tracked"]) + 1
    assert (out["kp25d"][:, 0, 2] == 0).all() and (out["zrel"][:, 0] == 0).all()
    assert out["zrel"].data_ptr() == out["kp25d"][..., 2:3].data_ptr() and out["kp2d"].data_ptr() == out["kp25d"].data_ptr()   # views
    assert out["kp25d"].is_contiguous()           # what PoseLoss takes
    # kp3d[:, 0, 2] = ku_z (0 + zroot) with ku_z = 1 up to the rounding of K^-1's last row: one rounding apart
    z, k = out["zroot"].double(), out["kp3d"][:, 0, 2].double()
    assert ((z - k).abs() <= 2.0 ** -23 * z.abs()).all()


# ------------------------------------------------------------------ 2. backward parity
@pytest.mark.parametrize("name", CASES)
def test_backward_matches_the_reference(model, name):
    from peclr_amd import _capi

    t = dev_inputs(name, feat_grad=False)
    gold, e_ref = gold_of(name), META["e_ref"][name]
    fc, s = model.backend_model.fc, model.zroot_ref.zroot_ref
    with torch.no_grad():        # the binding itself: it also hands out `do`, the gradient at the fc output
        out64, kp3d, zroot, save = _capi.pose_head_train_fwd(t["feat"], fc.weight, fc.bias, model._mlp_tensors(), (s[1].eps, s[4].eps),
                                                             (s[1].momentum, s[4].momentum), (s[1].num_batches_tracked, s[4].num_batches_tracked),
                                                             t["K"], model.zroot_ref.eps_value)
        d_feat, d_fc_w, d_fc_b, d_mlp, d_out = _capi.pose_head_train_bwd(t["feat"], fc.weight, model._mlp_tensors(), t["K"], out64, zroot,
                                                                         save, t["G3"], t["G25"], t["Gz"])
    got = dict(zip(ref.MLP_KEYS, d_mlp), do=d_out, dfeat=d_feat, dWfc=d_fc_w, dbfc=d_fc_b)
    for key in ("do", "dfeat", "dWfc", "dbfc") + ref.MLP_KEYS:
        if key in ZERO_BIAS:
            w = np.abs(gold[ZERO_BIAS[key]]).max()
            e = float(got[key].abs().max()) / w
            print(f"parity {name} {key}: |dev| / max|d {ZERO_BIAS[key]}| = {e:.3e}")
            assert e <= 1e-5, (name, key)
        else:
            hold(name, key, err(got[key], gold[key]), e_ref[key])
    assert (d_fc_w[2] == 0).all() and d_fc_b[2] == 0 and (d_out[:, 2] == 0).all()
    assert torch.equal(d_out[:, 63], t["G25"][:, 63])
    # through autograd (G25's last column has no path there: kp25d is out64[:, :63]): the same bits, rows 2 and 63 exactly 0
    _, g = run_case(model, name)
    assert (g["dWfc"][[2, 63]] == 0).all() and (g["dbfc"][[2, 63]] == 0).all()
    for key in ref.MLP_KEYS:
        assert torch.equal(g[key], got[key].reshape(g[key].shape)), key
    keep = [i for i in range(64) if i != 63]
    assert torch.equal(g["dWfc"][keep], d_fc_w[keep]) and torch.equal(g["dbfc"][keep], d_fc_b[keep])


# ------------------------------------------------------------------ 3. against the stock composition on the same device
@pytest.mark.parametrize("name", ["train_5_per_sample", "train_67_default"])
def test_matches_the_stock_composition_in_float64(model, name):
    stock = copy.deepcopy(model).double().train()
    stock.enable_hip_training(False)
    c = ref.case_inputs(NPZ, G11, name)
    feat = torch.from_numpy(c["feat"]).to(DEV).requires_grad_(True)
    G3, G25, Gz = (torch.from_numpy(c[k]).to(DEV) for k in ("G3", "G25", "Gz"))
    K = torch.from_numpy(c["K"]).to(DEV)
    fc_out = stock.backend_model.fc(feat)
    fc_out.retain_grad()
    grabbed = {}
    hook = stock.zroot_ref.register_forward_hook(lambda mod, inputs, o: grabbed.__setitem__("zroot", o))    # (returns None)
    so = stock._head_stock(fc_out.clone(), K)
    hook.remove()
    zroot = grabbed["zroot"].reshape(-1)
    ((so["kp3d"] * G3).sum() + (so["kp25d"].reshape(-1, 63) * G25[:, :63]).sum() + (zroot * Gz).sum()).backward()
    out, g = run_case(model, name)
    e_ref = META["e_ref"][name]
    for key in ("kp3d", "kp25d"):
        hold(name + "/stock", key, err(out[key], so[key].detach().cpu().numpy()), e_ref[key])
    hold(name + "/stock", "zroot", err(out["zroot"], zroot.detach().cpu().numpy()), e_ref["zroot"])
    sp = dict(stock.zroot_ref.zroot_ref.named_parameters())
    sg = {k: sp[k].grad for k in ref.MLP_KEYS}
    sg.update(dWfc=stock.backend_model.fc.weight.grad, dbfc=stock.backend_model.fc.bias.grad, dfeat=feat.grad)
    for key in ("dfeat", "dWfc", "dbfc") + ref.MLP_KEYS:
        if key in ZERO_BIAS:
            assert float(g[key].abs().max()) <= 1e-5 * float(sg[ZERO_BIAS[key]].abs().max()), key
        else:
            hold(name + "/stock", key, err(g[key], sg[key].cpu().numpy()), e_ref[key])
    for i in (1, 4):
        a, b = model.zroot_ref.zroot_ref[i], stock.zroot_ref.zroot_ref[i]
        hold(name + "/stock", f"{i}.running_var", err(a.running_var, b.running_var.cpu().numpy()), e_ref[f"{i}.running_var"])
        assert torch.equal(a.num_batches_tracked, b.num_batches_tracked)


# ------------------------------------------------------------------ 4. determinism
def _step(model, t):
    out = model.head(t["feat"], t["K"])
    loss = (out["kp3d"] * t["G3"]).sum() + (out["kp25d"].reshape(-1, 63) * t["G25"][:, :63]).sum() + (out["zroot"] * t["Gz"]).sum()
    params = [t["feat"], *model.backend_model.fc.parameters(), *model.zroot_ref.zroot_ref.parameters()]
    grads = torch.autograd.grad(loss, params)
    return [out["kp3d"].detach(), out["kp25d"].detach(), out["zroot"].detach(), *grads]


def test_eager_runs_and_a_graph_replay_agree_bit_for_bit(model):
    first, second = dev_inputs("train_37_per_sample"), dev_inputs("train_37_default")
    second["K"] = second["K"].expand(37, 3, 3).contiguous()
    second["G3"] = second["G3"] * 0.5
    a, b = _step(model, first), _step(model, first)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    static = {k: v.detach().clone().requires_grad_(k == "feat") for k, v in first.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _step(model, static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    nbt = [model.zroot_ref.zroot_ref[i].num_batches_tracked for i in (1, 4)]
    before = [int(n.item()) for n in nbt]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _step(model, static)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, captured):
        assert torch.equal(x, y)
    with torch.no_grad():
        for k, v in second.items():
            static[k].copy_(v)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert [int(n.item()) for n in nbt] == [v + 3 for v in before]        # one per replay, none for the capture itself
    eager = _step(model, second)
    for x, y in zip(captured, eager):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], eager[0]) and not torch.equal(a[3], eager[3])      # the replay read the new inputs


def test_forward_and_backward_do_not_synchronise_with_the_host(model):
    t = dev_inputs("train_5_per_sample")
    _step(model, t)                              # (first use: allocator, library load)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _step(model, t)
        with torch.no_grad():
            model.head(t["feat"], t["K"])
    finally:
        torch.cuda.set_sync_debug_mode(0)


# ------------------------------------------------------------------ 5. options
def test_features_without_grad_skip_dfeat_and_change_nothing_else(model):
    from peclr_amd import _capi

    _, with_feat = run_case(model, "train_5_per_sample")
    with_feat = {k: v.clone() for k, v in with_feat.items()}
    for p in model.parameters():
        p.grad = None
    _capi.EVENT_LOG = {}
    try:
        _, without = run_case(model, "train_5_per_sample", feat_grad=False)
        torch.cuda.synchronize()
        kernels = {k: [e[4] for e in v] for k, v in _capi.EVENT_LOG.items()}
    finally:
        _capi.EVENT_LOG = None
    assert kernels == {"pose_head_train_fwd": ["4 launches"], "pose_head_train_bwd": ["5 launches"]}
    assert without["dfeat"] is None and with_feat["dfeat"] is not None
    for k in with_feat:
        if k != "dfeat":
            assert torch.equal(with_feat[k], without[k]), k


@pytest.mark.parametrize("missing", ["g3", "g25", "gz"])
def test_a_missing_upstream_gradient_means_zeros(model, missing):
    from peclr_amd import _capi

    name = "train_5_default"
    _, g = run_case(model, name, **{missing: False})
    t = dev_inputs(name, feat_grad=False)
    fc, s = model.backend_model.fc, model.zroot_ref.zroot_ref
    ups = {"g3": t["G3"], "g25": torch.cat([t["G25"][:, :63], torch.zeros(5, 1, device=DEV)], 1), "gz": t["Gz"]}
    ups[missing] = torch.zeros_like(ups[missing])
    with torch.no_grad():
        out64, _, zroot, save = _capi.pose_head_train_fwd(t["feat"], fc.weight, fc.bias, model._mlp_tensors(), (s[1].eps, s[4].eps),
                                                          (s[1].momentum, s[4].momentum), (s[1].num_batches_tracked, s[4].num_batches_tracked),
                                                          t["K"], model.zroot_ref.eps_value)
        d_feat, d_fc_w, d_fc_b, d_mlp, _ = _capi.pose_head_train_bwd(t["feat"], fc.weight, model._mlp_tensors(), t["K"], out64, zroot, save,
                                                                     ups["g3"], ups["g25"], ups["gz"])
    zeros = dict(zip(ref.MLP_KEYS, d_mlp), dfeat=d_feat, dWfc=d_fc_w, dbfc=d_fc_b)
    for k in zeros:
        assert torch.equal(g[k], zeros[k].reshape(g[k].shape)), k


def test_train_mode_under_no_grad_updates_the_running_statistics_identically(model):
    t = dev_inputs("train_37_default")
    out = model.head(t["feat"], t["K"])
    seq = model.zroot_ref.zroot_ref
    with_grad = [out["kp3d"].detach().clone()] + [b.clone() for i in (1, 4) for b in seq[i].buffers()]
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.startswith(SEQ):
                v.copy_(torch.from_numpy(np.asarray(G11["w/" + k])))
        out = model.head(t["feat"], t["K"])
    assert not out["kp3d"].requires_grad and "zroot" in out
    for a, b in zip(with_grad, [out["kp3d"]] + [b for i in (1, 4) for b in seq[i].buffers()]):
        assert torch.equal(a, b)
    assert seq[1].num_batches_tracked.item() == int(G11[f"w/{SEQ}1.num_batches_tracked"]) + 1


def test_with_the_switch_off_train_mode_is_the_stock_path(model):
    t = dev_inputs("train_5_per_sample", feat_grad=False)
    off = copy.deepcopy(model).enable_hip_training(False)
    twin = copy.deepcopy(off)
    out = off.head(t["feat"], t["K"])
    stock = twin._head_stock(twin.backend_model.fc(t["feat"]), t["K"])
    assert sorted(out) == ["kp25d", "kp2d", "kp3d", "zrel"]
    for k in out:
        assert torch.equal(out[k], stock[k]), k
    for a, b in zip(off.zroot_ref.buffers(), twin.zroot_ref.buffers()):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        model.head(t["feat"][:1], t["K"][:1])


# ------------------------------------------------------------------ 6. one step of the whole model
def test_one_supervised_step_of_the_whole_model():
    from peclr_amd import PoseLoss, SupervisedAugmenter, _capi
    from peclr_amd import bn2d
    from peclr_amd.pose import RN25DwMLPref
    from tests.test_supervised_gpu import hands

    torch.manual_seed(5)
    b, hw = 8, (64, 64)
    m = RN25DwMLPref("rn50").to(DEV).enable_hip().enable_hip_training().train()
    k, j3d = hands(b, 31, hw, focal=200.0)
    images = torch.randint(0, 256, (b, hw[0], hw[1], 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).to(DEV)
    aug = SupervisedAugmenter({"resize": True}, {"resize_shape": [64, 64]}, rng=random.Random(1))
    batch = aug(images, torch.from_numpy(k), torch.from_numpy(j3d))
    assert tuple(batch["image"].shape) == (b, 3, 64, 64)
    ups = {}
    _capi.EVENT_LOG = {}
    try:
        with bn2d.routing(force=True):
            feat = m.features(batch["image"])
            feat.retain_grad()
            out = m.head(feat, batch["K"])         # forward() is features() + this head
            out["kp25d"].register_hook(lambda g: ups.__setitem__("g25", g))
            out["zroot"].register_hook(lambda g: ups.__setitem__("gz", g))
            total, _ = PoseLoss()(out["kp25d"], batch, z_root_calc=out["zroot"])
            total.backward()
        torch.cuda.synchronize()
        head = {k: [e[4] for e in v] for k, v in _capi.EVENT_LOG.items() if k.startswith("pose_head_train")}
    finally:
        _capi.EVENT_LOG = None
    assert bn2d.end_backward() == 0
    assert sum(int(s.split()[0]) for v in head.values() for s in v) == 10, head      # DESIGN.md 5.z'': 4 forward + 6 backward
    assert torch.isfinite(total)
    for name, p in m.named_parameters():
        g = p.grad
        assert g is not None and torch.isfinite(g).all(), name
        if name in (SEQ + "0.bias", SEQ + "3.bias"):
            continue
        if name.startswith("backend_model.fc."):
            assert (g[[2, 63]] == 0).all() and (g[[i for i in range(64) if i not in (2, 63)]] != 0).any(), name
        else:
            assert (g != 0).any(), name
    # the gradient at the pooled features is the head-only function's, bit for bit
    f2 = feat.detach().clone().requires_grad_(True)
    out2 = m.head(f2, batch["K"])
    d_feat, = torch.autograd.grad([out2["kp25d"], out2["zroot"]], f2, [ups["g25"], ups["gz"]])
    assert torch.equal(feat.grad, d_feat)
