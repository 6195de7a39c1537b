"""The supervised pose losses on the device (csrc/pose_loss.hip, peclr_amd/pose_loss.py) against the reference's own results
(tests/golden/g14_pose_losses.json) and the float64 restatement tests/pose_loss_ref.py (held to the reference at 1e-12 by
tests/test_pose_loss_host.py).

The bounds are those of tests/test_supervised_gpu.py; they follow from float64 evaluation rounded once.  Against the
reference's float64 result ON THE SAME INPUTS (gold64):
  losses      |dev - gold64| <= 2^-23 |gold64|
  gradients   |dev - gold64| <= max(2^-23 |gold64|, 2^-40 max |gold64| over the sample), element by element
and against its float32 result the same bound plus |gold32 - gold64|.  In the "clamps" case the root depth has slope 5e5 in
`b`, and there the gradient bound against gold64 is the float32 triangle form too: the bound above plus |gold32 - gold64| (the
kernel may be no further from the float64 truth than the reference's own float32 run plus one rounding).
"""
import random

import numpy as np
import pytest
import torch

from tests import pose_loss_ref as ref
from tests import supervised_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIX = ref.load_fixture()
CASES = FIX["cases"]
IDS = [c["name"] for c in CASES]
WEIGHTS = FIX["weights"]
EPS, FLOOR = 2.0 ** -23, 2.0 ** -40


def dev32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def per_sample_max(a):
    a = np.abs(a)
    return a.reshape(a.shape[0], -1).max(axis=1).reshape((-1,) + (1,) * (a.ndim - 1))


def check(got, g64, g32=None, what="", floor=True, triangle=False):
    """The bounds of the module docstring, element by element; prints the worst ratio.  got, g64, g32: [B, ...] (floor: the
    absolute floor of a gradient tensor; triangle: the "clamps" form of the gold64 bound)."""
    got, g64 = np.asarray(got, np.float64), np.asarray(g64, np.float64)
    assert got.shape == g64.shape, (what, got.shape, g64.shape)
    bound = np.maximum(EPS * np.abs(g64), FLOOR * per_sample_max(g64)) if floor else EPS * np.abs(g64)
    slack = np.abs(np.asarray(g32, np.float64) - g64) if g32 is not None else None
    bound64 = bound + slack if triangle else bound
    err = np.abs(got - g64)
    print(f"{what}: worst |dev - gold64| / bound = {np.max(err / np.where(bound64 == 0, 1, bound64)):.3f}")
    assert np.all(err <= bound64), (what, float(np.max(err - bound64)))
    if g32 is not None:
        err32, bound32 = np.abs(got - np.asarray(g32, np.float64)), slack + bound
        print(f"{what}: worst |dev - gold32| / bound = {np.max(err32 / np.where(bound32 == 0, 1, bound32)):.3f}")
        assert np.all(err32 <= bound32), (what, float(np.max(err32 - bound32)))


def run(inp, w):
    """Forward and `(w . losses).sum().backward()` on the device -> (losses [4] tensor, pred.grad, z_root_calc.grad or None)."""
    from peclr_amd import pose_losses

    pred = inp["pred"].clone().requires_grad_(True)
    zc = None if inp["z_root_calc"] is None else inp["z_root_calc"].clone().requires_grad_(True)
    out = pose_losses(pred, inp["joints"], inp["joints3D"], inp["scale"], inp["K"], inp["joints_valid"], zc)
    assert list(out) == list(ref.LOSS_NAMES)
    losses = torch.stack([out[n] for n in ref.LOSS_NAMES])
    assert all(o.dim() == 0 and o.dtype == torch.float32 and o.is_cuda for o in out.values())
    (losses * torch.tensor(w, device=DEV, dtype=torch.float32)).sum().backward()
    return losses.detach(), pred.grad, None if zc is None else zc.grad


def on_device(inp):
    return {k: dev32(v) for k, v in inp.items()}


# ------------------------------------------------------------------ 1. every fixture case, both weight vectors
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_losses_and_gradients_against_the_reference(case):
    inp = on_device(ref.case_inputs(case))
    g64, g32 = ({k: ref.dec(v).astype(np.float64) for k, v in case[g].items()} for g in ("gold64", "gold32"))
    clamps = case["kind"] == "clamps"
    for i, w in enumerate(WEIGHTS):
        losses, grad, grad_z = run(inp, w)
        assert grad.dtype == torch.float32 and tuple(grad.shape) == (case["B"], 21, 3)
        if case["kind"] == "no_valid":  # 0 / 0 in the reference, in either precision, losses and gradients
            assert np.isnan(g64["losses"]).all() and np.isnan(g64["grad_pred"]).all()
            assert torch.isnan(losses).all() and torch.isnan(grad).all()
            continue
        check(host(losses)[None], g64["losses"][None], g32["losses"][None], f"losses, w = {w}", floor=False)
        check(host(grad), g64["grad_pred"][i], g32["grad_pred"][i], f"grad_pred, w = {w}", triangle=clamps)
        assert (grad_z is None) == ("grad_z_root_calc" not in g64)
        if grad_z is not None:
            check(host(grad_z)[:, None], g64["grad_z_root_calc"][i][:, None], g32["grad_z_root_calc"][i][:, None],
                  f"grad_z_root_calc, w = {w}")


# ------------------------------------------------------------------ 2. - 4. the special cases, outright
def test_tied_joint_has_exactly_zero_l1_gradient():
    case = next(c for c in CASES if c["kind"] == "ties")
    s, j = case["tied"]
    inp = on_device(ref.case_inputs(case))
    _, grad, _ = run(inp, [1.0, 1.0, 1.0, 0.0])
    assert torch.all(grad[s, j] == 0.0), grad[s, j]
    others = inp["joints_valid"][s, :, 0].bool()
    others[j] = False
    assert torch.all(grad[s][others] != 0.0)


def test_no_valid_joint_gives_four_nan_losses():
    from peclr_amd import pose_losses

    inp = on_device(ref.case_inputs(next(c for c in CASES if c["kind"] == "no_valid")))
    out = pose_losses(inp["pred"], inp["joints"], inp["joints3D"], inp["scale"], inp["K"], inp["joints_valid"])
    assert len(out) == 4 and all(bool(torch.isnan(v)) for v in out.values())


def test_clamped_root_depth_keeps_its_gradient_through_b():
    """Sample 0 of "clamps": both clamps active, and the root depth still falls by 0.5 / 1e-6 per unit of b.  The wrist's u
    gradient stands two orders above the sample's median (127 x in the reference's float64 run with the first weight vector,
    1288 x for the 3D loss alone)."""
    inp = on_device(ref.case_inputs(next(c for c in CASES if c["kind"] == "clamps")))
    for w in (WEIGHTS[0], [0.0, 0.0, 0.0, 1.0]):
        _, grad, _ = run(inp, w)
        g = host(grad)[0]
        print(f"w = {w}: |grad wrist u| = {abs(g[0, 0]):.4f}, median |grad| = {np.median(np.abs(g)):.3e}")
        assert abs(g[0, 0]) > 100 * np.median(np.abs(g))


# ------------------------------------------------------------------ 5. more than one pass of the fold
def big_batch(n, seed):
    """n synthetic hands (tests/test_supervised_gpu.py: hands) with the fixture's kind of prediction -> float32 NumPy inputs."""
    from tests.test_supervised_gpu import hands

    k, j3d = hands(n, seed)
    g = np.random.default_rng(seed + 1)
    joints, scale = zip(*(supervised_ref.to_25d(k[i], j3d[i]) for i in range(n)))
    joints, scale = np.array(joints, dtype=np.float32), np.array(scale, dtype=np.float32)
    pred = (joints + g.standard_normal((n, 21, 3)) * np.array([4.0, 4.0, 0.15])).astype(np.float32)
    valid = (g.uniform(size=(n, 21, 1)) >= 0.2).astype(np.float32)
    return {"pred": pred, "joints": joints, "joints3D": j3d, "scale": scale, "K": k, "joints_valid": valid, "z_root_calc": None}


def test_batch_of_261_against_the_restatement():
    """261 = 256 + 5: the fold's threads make a second pass with a ragged remainder; 66 workgroups, the last one with one wave."""
    inp = big_batch(261, 77)
    w = WEIGHTS[1]
    want_l, want_g, _ = ref.losses_and_grads(inp, w)
    losses, grad, _ = run(on_device(inp), w)
    check(host(losses)[None], want_l[None], what="losses, B = 261", floor=False)
    check(host(grad), want_g, what="grad_pred, B = 261")


# ------------------------------------------------------------------ 6. the thin views
def test_l1_loss_and_loss_3d_are_the_entries_of_pose_losses():
    from peclr_amd import l1_loss, loss_3d, pose_losses

    for case in (next(c for c in CASES if c["name"] == "b5"), next(c for c in CASES if c["kind"] == "z_root_calc")):
        inp = on_device(ref.case_inputs(case))
        grads = []
        for which in ("all", "views"):
            pred = inp["pred"].clone().requires_grad_(True)
            zc = None if inp["z_root_calc"] is None else inp["z_root_calc"].clone().requires_grad_(True)
            if which == "all":
                out = pose_losses(pred, inp["joints"], inp["joints3D"], inp["scale"], inp["K"], inp["joints_valid"], zc)
                got = [out[n] for n in ref.LOSS_NAMES]
            else:
                got = [*l1_loss(pred, inp["joints"], inp["scale"], inp["joints_valid"]),
                       loss_3d(pred, inp["joints3D"], inp["scale"], inp["K"], inp["joints_valid"], zc)]
            grads.append([got, [torch.autograd.grad(v, pred, retain_graph=True)[0] for v in got]])
        for n, a, b, ga, gb in zip(ref.LOSS_NAMES, grads[0][0], grads[1][0], grads[0][1], grads[1][1]):
            assert torch.equal(a, b), n
            assert torch.equal(ga, gb), n


# ------------------------------------------------------------------ 7. run to run
def test_two_calls_are_bit_identical():
    inp = on_device(big_batch(37, 5))
    a, b = run(inp, WEIGHTS[1]), run(inp, WEIGHTS[1])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------ 8. one captured graph, forward and backward
def test_forward_and_backward_replay_from_a_graph():
    from peclr_amd import pose_losses

    first = on_device(dict(ref.case_inputs(next(c for c in CASES if c["name"] == "b5")), z_root_calc=np.full(5, 3.5, np.float32)))
    second = on_device(dict(big_batch(5, 11), z_root_calc=np.full(5, 4.0, np.float32)))
    w = torch.tensor(WEIGHTS[1], device=DEV, dtype=torch.float32)
    static = {k: v.clone() for k, v in first.items()}
    static["pred"].requires_grad_(True)
    static["z_root_calc"].requires_grad_(True)

    def step(t):
        out = pose_losses(t["pred"], t["joints"], t["joints3D"], t["scale"], t["K"], t["joints_valid"], t["z_root_calc"])
        losses = torch.stack([out[n] for n in ref.LOSS_NAMES])
        grad, grad_z = torch.autograd.grad((losses * w).sum(), (t["pred"], t["z_root_calc"]))
        return losses.detach(), grad, grad_z

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(static)
    graph.replay()
    on_first = [t.clone() for t in captured]
    with torch.no_grad():
        for k, v in second.items():
            static[k].copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    second["pred"].requires_grad_(True)
    second["z_root_calc"].requires_grad_(True)
    eager = step(second)
    for name, a, b in zip(("losses", "grad_pred", "grad_z_root_calc"), captured, eager):
        assert torch.equal(a, b), name
    assert not torch.equal(on_first[0], eager[0]) and not torch.equal(on_first[1], eager[1])   # the replay read the new inputs


# ------------------------------------------------------------------ 9. on the dict SupervisedAugmenter returns
def test_pose_loss_module_on_a_supervised_batch():
    from peclr_amd import PoseLoss, SupervisedAugmenter
    from tests.test_supervised_gpu import hands

    b, hw = 4, (64, 64)
    k, j3d = hands(b, 31, hw, focal=200.0)
    images = torch.zeros((b, hw[0], hw[1], 3), dtype=torch.uint8, device=DEV)
    aug = SupervisedAugmenter({"resize": True}, {"resize_shape": [64, 64]}, rng=random.Random(1))   # every augmentation off
    batch = aug(images, torch.from_numpy(k), torch.from_numpy(j3d))
    crit = PoseLoss({"loss_2d": 1.0, "loss_z": 1.0, "loss_3d": 1.0})
    pred = (batch["joints"] + 1.0).requires_grad_(True)
    total, parts = crit(pred, batch)
    exact = float((pred.detach().double() - batch["joints"].double())[..., :2].abs().mean())
    print(f"loss_2d = {parts['loss_2d'].item()!r}; mean |pred - joints| over u, v in float64 = {exact!r}")
    assert abs(parts["loss_2d"].item() - 1.0) <= 2.0 ** -23
    assert abs(parts["loss_2d"].item() - exact) <= 2.0 ** -23 * exact
    assert total.item() == (parts["loss_2d"] + parts["loss_z"] + parts["loss_3d"]).item()
    opt = torch.optim.Adam([pred], lr=0.01)
    start = total.item()
    for _ in range(40):
        opt.zero_grad(set_to_none=True)
        total, _ = crit(pred, batch)
        total.backward()
        opt.step()
    end = crit(pred, batch)[0].item()
    print(f"total: {start:.6f} -> {end:.6f} after 40 Adam steps")
    assert end < start
