"""The supervised pose losses' host side (peclr_amd/pose_loss.py) and the float64 restatement the GPU tests measure against
(tests/pose_loss_ref.py), on the reference's own results (tests/golden/g14_pose_losses.json).  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import pose_loss_ref as ref

FIX = ref.load_fixture()
CASES = FIX["cases"]
IDS = [c["name"] for c in CASES]
WEIGHTS = FIX["weights"]
REL = 1e-12  # both sides are float64 and differ only in evaluation order and in how the 3 x 3 inverse is taken


def close(got, want, what):
    """Within REL of the tensor's largest magnitude; NaN where the reference has NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    if np.isnan(want).all():
        return
    err = np.nan_to_num(np.abs(got - want))
    top = np.nanmax(np.abs(want))
    print(f"{what}: worst error / largest magnitude {err.max() / top:.3e}")
    assert err.max() <= REL * top, (what, err.max() / top)


def test_fixture_is_what_the_issue_describes():
    assert os.path.getsize(ref.GOLDEN) < 150 * 1024
    assert WEIGHTS == [[1.0, 1.0, 0.0, 1.0], [0.5, 2.0, 3.0, 0.25]] and FIX["loss_names"] == list(ref.LOSS_NAMES)
    assert sorted(c["B"] for c in CASES if c["kind"] == "plain") == [1, 3, 4, 5, 9]
    assert sorted(c["kind"] for c in CASES if c["kind"] != "plain") == ["clamps", "no_valid", "ties", "z_root_calc"]
    assert sum("joints_valid" not in c for c in CASES) == 1
    for c in CASES:
        inp = ref.case_inputs(c)
        assert all(v is None or v.dtype == np.float32 for v in inp.values())
        assert (inp["z_root_calc"] is not None) == (c["kind"] == "z_root_calc")
    ties = next(c for c in CASES if c["kind"] == "ties")
    inp, (s, j) = ref.case_inputs(ties), ties["tied"]
    assert np.array_equal(inp["pred"][s, j], inp["joints"][s, j]) and inp["joints_valid"][s, j, 0] == 1.0
    clamps = ref.case_inputs(next(c for c in CASES if c["kind"] == "clamps"))
    assert np.array_equal(clamps["pred"][0, 0, :2], clamps["pred"][0, 2, :2])
    assert clamps["pred"][1, 2, 2] == np.float32(clamps["pred"][1, 0, 2] + np.float32(3.0))
    assert not ref.case_inputs(next(c for c in CASES if c["kind"] == "no_valid"))["joints_valid"].any()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_agrees_with_the_reference_in_float64(case):
    inp, g64 = ref.case_inputs(case), {k: ref.dec(v) for k, v in case["gold64"].items()}
    for i, w in enumerate(WEIGHTS):
        losses, grad, grad_z = ref.losses_and_grads(inp, w)
        close(losses, g64["losses"], "losses")
        close(grad, g64["grad_pred"][i], f"grad_pred, weights {w}")
        assert (grad_z is None) == ("grad_z_root_calc" not in g64)
        if grad_z is not None:
            close(grad_z, g64["grad_z_root_calc"][i], f"grad_z_root_calc, weights {w}")


def test_restatement_on_the_special_cases():
    by_kind = {c["kind"]: c for c in CASES}
    # ties: the L1 gradients vanish at the tied joint (sign(0) = 0), so only the 3D loss moves it
    s, j = by_kind["ties"]["tied"]
    _, grad, _ = ref.losses_and_grads(ref.case_inputs(by_kind["ties"]), [1.0, 1.0, 1.0, 0.0])
    assert np.all(grad[s, j] == 0.0) and np.count_nonzero(grad[s]) == 3 * (np.count_nonzero(ref.case_inputs(by_kind["ties"])["joints_valid"][s]) - 1)
    # clamps: both clamps active in sample 0 (root depth 0.5 sqrt(1e-6) / 1e-6) and the gradient through b is there
    inp = ref.case_inputs(by_kind["clamps"])
    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in inp.items() if v is not None}
    z_root = ref.root_depth(t["pred"], ref.inverse3(t["K"])).numpy()
    assert abs(z_root[0] - 500.0) < 1e-6
    _, grad, _ = ref.losses_and_grads(inp, WEIGHTS[0])
    assert abs(grad[0, 0, 0]) > 100 * np.median(np.abs(grad[0]))
    # no valid joint: 0 / 0
    losses, grad, _ = ref.losses_and_grads(ref.case_inputs(by_kind["no_valid"]), WEIGHTS[0])
    assert np.isnan(losses).all() and np.isnan(grad).all()


# ------------------------------------------------------------------ the public functions
def _host_batch(b=2):
    inp = ref.case_inputs(next(c for c in CASES if c["B"] >= b and c["kind"] == "plain" and "joints_valid" in c))
    return {k: torch.from_numpy(v[:b].copy()) for k, v in inp.items() if v is not None}


def test_cpu_tensors_are_refused():
    from peclr_amd import PoseLoss, _capi, l1_loss, loss_3d, pose_losses

    t = _host_batch()
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        pose_losses(t["pred"], t["joints"], t["joints3D"], t["scale"], t["K"], t["joints_valid"])
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        l1_loss(t["pred"], t["joints"], t["scale"])
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        loss_3d(t["pred"], t["joints3D"], t["scale"], t["K"], t["joints_valid"], torch.ones(2))
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        PoseLoss((1, 1, 0, 1))(t["pred"], t)


def test_wrong_shapes_are_refused_before_any_device_call(monkeypatch):
    from peclr_amd import PoseLoss, _capi, l1_loss, loss_3d, pose_losses

    def no_device(*a, **k):
        raise AssertionError("device call")

    monkeypatch.setattr(_capi, "pose_loss", no_device)
    monkeypatch.setattr(_capi, "pose_loss_bwd", no_device)
    t = _host_batch()
    p, j, j3, s, k, v = (t[n] for n in ("pred", "joints", "joints3D", "scale", "K", "joints_valid"))
    with pytest.raises(ValueError, match="pred"):
        pose_losses(p[:, :20], j, j3, s, k)
    with pytest.raises(ValueError, match="pred"):
        pose_losses(p.reshape(2, 63), j, j3, s, k)
    with pytest.raises(ValueError, match="joints3d"):
        pose_losses(p, j, j3[:1], s, k)
    with pytest.raises(ValueError, match="scale"):
        pose_losses(p, j, j3, s.reshape(2, 1), k)
    with pytest.raises(ValueError, match="K"):
        pose_losses(p, j, j3, s, k[:, :2])
    with pytest.raises(ValueError, match="joints_valid"):
        pose_losses(p, j, j3, s, k, v.reshape(2, 21))
    with pytest.raises(ValueError, match="z_root_calc"):
        pose_losses(p, j, j3, s, k, v, torch.ones(2, 1))
    with pytest.raises(ValueError, match="joints"):
        l1_loss(p, j[:, :, :2], s)
    with pytest.raises(ValueError, match="joints3d"):
        loss_3d(p, None, s, k)
    with pytest.raises(ValueError, match="K"):
        PoseLoss()(p, dict(t, K=k[0]))
    with pytest.raises(ValueError, match="weights"):
        PoseLoss((1, 1, 1))
    with pytest.raises(ValueError, match="unknown loss names"):
        PoseLoss({"loss_2D": 1.0})
    assert PoseLoss({"loss_3d": 2.0}).weights == {"loss_2d": 0.0, "loss_z": 0.0, "loss_z_unscaled": 0.0, "loss_3d": 2.0}


def test_autograd_plumbing_with_the_native_calls_replaced(monkeypatch):
    """`pose_losses`, its two thin views and `PoseLoss` around stand-ins for the two native calls (the restatement's Jacobian
    handed from the forward stand-in to the backward one): which tensor goes where, which loss a view keeps, that an unused
    loss sends a zero upstream, that `z_root_calc` gets its gradient only when it asks."""
    from peclr_amd import PoseLoss, _capi, l1_loss, loss_3d, pose_losses

    calls = []

    def forward(pred, joints, joints3d, scale, K, joints_valid=None, z_root_calc=None):
        calls.append(("fwd", joints is not None, joints3d is not None, K is not None, z_root_calc is not None))
        b = pred.shape[0]
        d = lambda t: None if t is None else t.detach().double()  # noqa: E731
        with torch.enable_grad():
            p = d(pred).requires_grad_(True)
            zc = None if z_root_calc is None else d(z_root_calc).requires_grad_(True)
            out = ref.losses(p, p.detach() if joints is None else d(joints), torch.zeros(b, 21, 3, dtype=torch.float64) if joints3d is None
                             else d(joints3d), d(scale), torch.eye(3, dtype=torch.float64).repeat(b, 1, 1) if K is None else d(K),
                             d(joints_valid), zc)
            if joints3d is None:
                out = out * torch.tensor([1.0, 1.0, 1.0, 0.0], dtype=torch.float64)
            rows = [torch.autograd.grad(out[i], [p] + ([] if zc is None else [zc]), retain_graph=True, allow_unused=True) for i in range(4)]
        jac = torch.stack([torch.zeros_like(p) if r[0] is None else r[0] for r in rows])
        jac_z = None if zc is None else torch.stack([torch.zeros(b, dtype=torch.float64) if r[1] is None else r[1] for r in rows])
        return out.detach().float(), jac, torch.zeros(b, 21, 3, dtype=torch.float64), jac_z, torch.ones(1, dtype=torch.float64)

    def backward(up, jac, g_3d, jac_z, scale, inv_valid, want_z_root=False):
        calls.append(("bwd", want_z_root))
        assert up.dtype == torch.float32 and tuple(up.shape) == (4,)
        grad = torch.einsum("i,ibjc->bjc", up.double(), jac).float()
        return grad, (torch.einsum("i,ib->b", up.double(), jac_z).float() if want_z_root else None)

    monkeypatch.setattr(_capi, "pose_loss", forward)
    monkeypatch.setattr(_capi, "pose_loss_bwd", backward)
    t = _host_batch(3)
    inp = {k: v.numpy() for k, v in t.items()}
    inp["z_root_calc"] = None
    p, j, j3, s, k, v = (t[n] for n in ("pred", "joints", "joints3D", "scale", "K", "joints_valid"))

    w = WEIGHTS[1]
    pred = p.clone().requires_grad_(True)
    out = pose_losses(pred, j, j3, s, k, v)
    assert list(out) == list(ref.LOSS_NAMES) and all(o.dim() == 0 and o.dtype == torch.float32 for o in out.values())
    sum(wi * out[n] for wi, n in zip(w, ref.LOSS_NAMES)).backward()
    want_l, want_g, _ = ref.losses_and_grads(inp, w)
    assert np.allclose(torch.stack(list(out.values())).detach().numpy(), want_l, rtol=1e-6)
    assert np.allclose(pred.grad.numpy(), want_g, rtol=1e-5, atol=1e-9)
    assert calls == [("fwd", True, True, True, False), ("bwd", False)]

    # the views: the same call, one term left out; the loss they do not return sends a zero upstream
    calls.clear()
    pred = p.clone().requires_grad_(True)
    three = l1_loss(pred, j, s, v)
    assert len(three) == 3 and all(torch.equal(a.detach(), out[n].detach()) for a, n in zip(three, ref.LOSS_NAMES))
    (three[0] + three[2]).backward()
    assert np.allclose(pred.grad.numpy(), ref.losses_and_grads(inp, [1, 0, 1, 0])[1], rtol=1e-5, atol=1e-9)
    zc = torch.full((3,), 4.0, requires_grad=True)
    pred = p.clone().requires_grad_(True)
    one = loss_3d(pred, j3, s, k, v, zc)
    one.backward()
    _, want_g, want_z = ref.losses_and_grads(dict(inp, z_root_calc=zc.detach().numpy()), [0, 0, 0, 1])
    assert np.allclose(pred.grad.numpy(), want_g, rtol=1e-5, atol=1e-9) and np.allclose(zc.grad.numpy(), want_z, rtol=1e-5)
    assert calls == [("fwd", True, False, False, False), ("bwd", False), ("fwd", False, True, True, True), ("bwd", True)]

    # z_root_calc that asks for no gradient gets none computed
    calls.clear()
    pred = p.clone().requires_grad_(True)
    total, parts = PoseLoss(WEIGHTS[0])(pred, t, z_root_calc=zc.detach())
    total.backward()
    assert calls == [("fwd", True, True, True, True), ("bwd", False)] and list(parts) == list(ref.LOSS_NAMES)
    want_l, want_g, _ = ref.losses_and_grads(dict(inp, z_root_calc=zc.detach().numpy()), WEIGHTS[0])
    assert np.allclose(float(total.detach()), float(np.dot(WEIGHTS[0], want_l)), rtol=1e-6)
    assert np.allclose(pred.grad.numpy(), want_g, rtol=1e-5, atol=1e-9)


def test_entry_points_are_declared_bound_and_refuse_null():
    from peclr_amd import _capi
    from tests.test_capi_abi import declared_signatures

    declared = declared_signatures()
    for name in ("peclr_pose_loss", "peclr_pose_loss_bwd"):
        assert declared[name] == (_capi.SIGNATURES[name][0], list(_capi.SIGNATURES[name][1]))
    L = _capi.lib()
    assert L.peclr_pose_loss(*([None] * 7), 4, *([None] * 7)) == -1
    assert L.peclr_pose_loss_bwd(*([None] * 6), 4, None, None, None) == -1
    one = 64  # any non-null address: the checks below fail before a launch
    assert L.peclr_pose_loss(*([one] * 5), None, None, 0, *([one] * 6), None) == -1                  # B = 0
    assert L.peclr_pose_loss(one, None, None, one, None, None, None, 4, *([one] * 6), None) == -1   # neither truth
    assert L.peclr_pose_loss(one, None, one, one, None, None, None, 4, *([one] * 6), None) == -1    # joints3d without K
    assert L.peclr_pose_loss_bwd(one, one, one, None, one, one, 4, one, one, None) == -1            # grad_z without g_zroot
