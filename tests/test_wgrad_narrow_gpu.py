"""The weight gradient of 3x3 and stride-2 convolutions on feature maps narrower than 6 columns (`bn2d._wgrad_narrow_x6`: the
taps' pixels gathered, then one fixed-order dY^T X on peclr_gemm_x6t_f32) -- the route `routing(force=True)` takes where the
padded-pixel-space kernels do not apply -- and the weight planes an eager forward sees after a hipGraph replay.

Shapes: the 11 such convolutions of a ResNet-50 on 8 crops of 64 x 64 (layer3 at 4 x 4, layer4 at 2 x 2, the stride-2 entries
of both stages).  Bound: the project's calibration rule -- e = max|dW - gold64| / max|gold64| against float64 autograd on the
CPU, e(narrow) <= max(6 e(MIOpen fp32 on the same tensors), 1e-5)."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (Cin, Cout, input H = W, stride, kernel)
SHAPES = [(256, 256, 4, 1, 3), (512, 512, 2, 1, 3), (256, 256, 8, 2, 3), (512, 512, 4, 2, 3), (512, 1024, 8, 2, 1), (1024, 2048, 4, 2, 1),
          (64, 64, 5, 1, 3), (512, 1024, 2, 2, 1), (256, 256, 2, 2, 3), (128, 128, 1, 1, 3)]      # ... and down to one-pixel maps


@pytest.mark.parametrize("cin,cout,hw,stride,k", SHAPES)
def test_narrow_weight_gradient_against_float64(cin, cout, hw, stride, k):
    from peclr_amd import bn2d

    g = torch.Generator().manual_seed(cin + hw + stride)
    x = torch.randn(8, cin, hw, hw, generator=g).relu_()
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    w64 = w.double().requires_grad_()
    y = F.conv2d(x.double(), w64, None, stride, k // 2)
    gy = torch.randn(y.shape, generator=g)
    (gold,) = torch.autograd.grad(y, w64, gy.double())
    cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)  # noqa: E731
    xd, wd, gyd = cl(x), cl(w), cl(gy)
    got = bn2d._wgrad_narrow_x6(gyd, xd, wd, None, stride=stride, taps=k * k)
    again = bn2d._wgrad_narrow_x6(gyd, xd, wd, None, stride=stride, taps=k * k)
    stock = torch.ops.aten.convolution_backward(gyd, xd, wd, None, [stride] * 2, [k // 2] * 2, [1, 1], False, [0, 0], 1, [False, True, False])[1]
    assert got.shape == wd.shape and got.stride() == wd.stride()
    assert torch.equal(got, again)
    scale = float(gold.abs().max())
    e_dev, e_stock = (float((t.double().cpu() - gold).abs().max()) / scale for t in (got, stock))
    print(f"narrow wgrad {cin}->{cout} {hw}x{hw} s{stride} k{k}: e_narrow = {e_dev:.3e} e_miopen32 = {e_stock:.3e}")
    assert e_dev <= max(6 * e_stock, 1e-5)


def test_forced_routing_takes_the_narrow_route_and_default_routing_does_not(monkeypatch):
    from peclr_amd import bn2d
    from peclr_amd.pose import RN25DwMLPref

    calls = {"narrow": 0, "miopen": 0}
    narrow, miopen = bn2d._wgrad_narrow_x6, bn2d._conv_wgrad
    monkeypatch.setattr(bn2d, "_wgrad_narrow_x6", lambda *a, **k: (calls.__setitem__("narrow", calls["narrow"] + 1), narrow(*a, **k))[1])
    monkeypatch.setattr(bn2d, "_conv_wgrad", lambda *a, **k: (calls.__setitem__("miopen", calls["miopen"] + 1), miopen(*a, **k))[1])
    torch.manual_seed(2)
    m = RN25DwMLPref("rn50").to(DEV).enable_hip().train()
    x = torch.randn(8, 3, 64, 64, device=DEV).contiguous(memory_format=torch.channels_last)
    with bn2d.routing(force=True):
        m.features(x).sum().backward()
        bn2d.end_backward()
    assert calls == {"narrow": 11, "miopen": 0}        # layer3.1-5 + layer4.1-2 conv2, and conv2 + shortcut of layer3.0 and layer4.0
    for p in m.parameters():
        p.grad = None
    calls.update(narrow=0, miopen=0)
    m2 = copy.deepcopy(m)
    m2.features(x).sum().backward()                     # default routing: small shapes stay where they were
    bn2d.end_backward()
    assert calls["narrow"] == 0 and calls["miopen"] > 0


def test_an_eager_forward_after_a_replay_sees_the_replayed_weights():
    """Pretraining path: the replayed optimiser launch writes the parameters through raw pointers; an eager forward after it
    (validation, a ragged batch) must re-pack its weight planes -- its output equals the same forward after an explicit re-pack."""
    import warnings

    from peclr_amd import Hybrid2Model, Trainer, _capi, bn2d, hybrid2_config
    from peclr_amd.bn2d import enable_hip_batchnorm

    warnings.simplefilter("ignore")
    torch.manual_seed(11)
    n = 8
    cfg = hybrid2_config(resnet_size="18", projection_head_input_dim=512, augmentation=["crop", "rotate"], batch_size=n, num_samples=64,
                         warmup_epochs=1, pretrained=False)
    model = Hybrid2Model(cfg).to(DEV).train()
    model.encoder = model.encoder.to(memory_format=torch.channels_last)
    enable_hip_batchnorm(model.encoder)
    g = torch.Generator().manual_seed(12)
    batch = {"transformed_image1": torch.randn(n, 3, 64, 64, generator=g), "transformed_image2": torch.randn(n, 3, 64, 64, generator=g),
             "jitter_x_1": torch.randint(-14, 1, (n,), generator=g), "jitter_x_2": torch.randint(-14, 1, (n,), generator=g),
             "jitter_y_1": torch.randint(-14, 1, (n,), generator=g), "jitter_y_2": torch.randint(-14, 1, (n,), generator=g),
             "angle_1": torch.randint(-45, 46, (n,), generator=g).double(), "angle_2": torch.randint(-45, 46, (n,), generator=g).double()}
    batch = {k: v.to(DEV) for k, v in batch.items()}
    for k in ("transformed_image1", "transformed_image2"):
        batch[k] = batch[k].contiguous(memory_format=torch.channels_last)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with bn2d.routing(force=True), torch.cuda.stream(side):
        tr = Trainer(max_epochs=10).attach(model)
        tr.zero_grad()
        tr.capture_step_graph(batch, warmup=1)
        model.eval()
        with torch.no_grad():
            model.encoder(batch["transformed_image1"])             # an eager forward between replays: its planes are fresh now
        model.train()
        for _ in range(3):
            tr.replay_step()
        model.eval()
        with torch.no_grad():
            after_replay = model.encoder(batch["transformed_image1"]).clone()
            _capi.WEIGHTS_EPOCH += 1                                # what forces a re-pack of every plane set
            repacked = model.encoder(batch["transformed_image1"]).clone()
        tr.close()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(after_replay, repacked)
