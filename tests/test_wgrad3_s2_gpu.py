"""peclr_wgrad3s2_h (csrc/wgrad_h.hip, wgrad3_h_s2_kernel): the 16-bit 3x3 / padding-1 / stride-2 weight gradient -- X as four
parity planes, each in the padded pixel space of dY's geometry, all nine taps in one workgroup, fixed-order slabs -- against
float64 on the SAME 16-bit inputs (`-m gpu`).  The bar is the project's own for a 16-bit 3x3 weight gradient
(tests/test_conv_h_gpu.py, tests/test_wgrad3_wide_gpu.py): fp32 accumulation of exact 16-bit products,
max |got - ref| <= 3e-6 max |ref| max(1, sqrt(output pixels / 4096)).
Replaces MIOpen's 16-bit weight gradient of the convolutions that open layers 2 - 4 (torchvision's Bottleneck / BasicBlock
behind the reference's resnet_model.py under `precision: 16`) where `ROUTING.wgrad16_s2` is on."""
import functools

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.bfloat16, torch.float16]

# (images, cout, cin, ho, wo), all of >= 512 output pixels: the smallest shapes that meet each way the plane map can go wrong
SHAPES = [(512, 64, 64, 1, 1),         # 2 x 2 inputs: every tap with a = 0 or b = 0 is padding, every slot an image boundary
          (9, 64, 64, 1, 62),          # one output row, the widest row accepted
          (86, 64, 64, 6, 1),          # one output column
          (8, 64, 64, 8, 8),
          (11, 64, 64, 7, 7),          # layer4's geometry, odd output width
          (3, 64, 64, 14, 14),
          (2, 128, 64, 16, 16), (2, 64, 128, 16, 16),      # tile indexing in M and in N
          (4, 64, 64, 28, 28),         # several slabs: boundaries inside rows and between images
          (1, 64, 64, 9, 62)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module")
def capi():
    from peclr_amd import _capi

    _capi.lib()
    return _capi


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def bar(nb, ho, wo):
    return 3e-6 * max(1.0, (nb * ho * wo / 4096) ** 0.5)


def reference(gy, x):
    """[Cout, Cin, 3, 3] in float64 from the 16-bit operands."""
    wz = torch.zeros(gy.shape[1], x.shape[1], 3, 3, device=gy.device, dtype=torch.float64)
    return torch.ops.aten.convolution_backward(gy.double(), x.double(), wz, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


def as_weight(dw, cout, cin):
    return dw.view(cout, 3, 3, cin).permute(0, 3, 1, 2).double()


@functools.lru_cache(maxsize=None)
def problem(dtype, shape):
    """(gy, x, float64 reference) of one shape: built once, shared by the tests below, never written to."""
    nb, cout, cin, ho, wo = shape
    g = torch.Generator(device=DEV).manual_seed(nb + cout + cin + ho + wo)
    x = nhwc(torch.randn(nb, cin, 2 * ho, 2 * wo, device=DEV, generator=g).to(dtype))
    gy = nhwc(torch.randn(nb, cout, ho, wo, device=DEV, generator=g).to(dtype))
    return gy, x, reference(gy, x)


def rel_err(got, ref):
    return float((got - ref).abs().max()) / float(ref.abs().max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_wgrad3_s2_matches_float64(capi, dtype, shape):
    nb, cout, cin, ho, wo = shape
    gy, x, ref = problem(dtype, shape)
    assert capi.wgrad3_s2_h_ok(gy, x)
    dw = capi.wgrad3_s2_h(gy, x)
    assert dw.shape == (cout, 9 * cin) and dw.dtype == torch.float32
    err = rel_err(as_weight(dw, cout, cin), ref)
    print(f"{shape} {dtype}: {err:.3e} of the scale (bar {bar(nb, ho, wo):.3e}), {capi.lib().peclr_wgrad3s2_h_slabs(cout, cin, nb, ho, wo)} slabs")
    assert err <= bar(nb, ho, wo), err
    for _ in range(4):
        assert torch.equal(capi.wgrad3_s2_h(gy, x), dw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ho,wo", [(14, 14), (3, 62), (171, 1), (13, 15)])      # three images of >= 171 output pixels each
def test_one_hot_taps_meet_exactly_their_pixel(capi, dtype, ho, wo):
    """dY zero but for one pixel of the SECOND of three images, holding a random channel vector: each of the nine taps of dW is
    that vector times exactly X[img, 2 oh + a - 1, 2 ow + b - 1, :], or zero where that pixel is outside the image.  Sees a swapped plane, a shift taken from the wrong row pitch, and the last row
    of the previous image read as padding."""
    c = 64
    nb = 3
    g = torch.Generator(device=DEV).manual_seed(100 * ho + wo)
    x = nhwc(torch.randn(nb, c, 2 * ho, 2 * wo, device=DEV, generator=g).to(dtype))
    val = torch.randn(c, device=DEV, generator=g).to(dtype)
    pixels = {(0, 0), (0, wo - 1), (ho - 1, 0), (ho - 1, wo - 1), (ho // 2, wo // 2)}
    for oh, ow in sorted(pixels):
        gy = nhwc(torch.zeros(nb, c, ho, wo, device=DEV, dtype=dtype))
        gy[1, :, oh, ow] = val
        assert capi.wgrad3_s2_h_ok(gy, x)
        got, ref = as_weight(capi.wgrad3_s2_h(gy, x), c, c), reference(gy, x)
        patch = torch.zeros(c, 3, 3, device=DEV, dtype=torch.float64)          # [Cin, 3, 3]: what the nine taps meet
        for a in range(3):
            for b in range(3):
                r, q = 2 * oh + a - 1, 2 * ow + b - 1
                if 0 <= r < 2 * ho and 0 <= q < 2 * wo:
                    patch[:, a, b] = x[1, :, r, q].double()
        by_hand = val.double().view(c, 1, 1, 1) * patch.unsqueeze(0)
        assert rel_err(ref, by_hand) <= 1e-14
        assert rel_err(got, ref) <= bar(nb, ho, wo), ((oh, ow), rel_err(got, ref))
        assert rel_err(got, by_hand) <= bar(nb, ho, wo), ((oh, ow), rel_err(got, by_hand))
        assert torch.equal(got == 0, by_hand == 0), (oh, ow)                   # the taps outside the image are zero, no others


def embedded(t, fill=1e4):
    """The same channels_last tensor as an interior view of a larger buffer filled with `fill` (margins: four image rows)."""
    nb, c, h, w = t.shape
    margin = 4 * w * c
    buf = torch.full((t.numel() + 2 * margin,), fill, device=t.device, dtype=t.dtype)
    inner = buf[margin:margin + t.numel()].view(nb, h, w, c).permute(0, 3, 1, 2)
    inner.copy_(t)
    assert inner.is_contiguous(memory_format=torch.channels_last) and inner.data_ptr() % 16 == 0
    return inner


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[8]], ids=lambda s: "x".join(map(str, s)))
def test_padding_is_zero_not_memory(capi, dtype, shape):
    """The operands as interior views of buffers filled with 1e4: a fetch outside an image (a padding row or column, a slot
    before the first or after the last pixel) would show as an error of ~1e4 times the scale."""
    nb, cout, cin, ho, wo = shape
    gy, x, ref = problem(dtype, shape)
    dw = capi.wgrad3_s2_h(embedded(gy), embedded(x))
    assert rel_err(as_weight(dw, cout, cin), ref) <= bar(nb, ho, wo)
    assert torch.equal(dw, capi.wgrad3_s2_h(gy, x))


@pytest.mark.parametrize("dtype,shape", [(torch.bfloat16, SHAPES[4]), (torch.float16, SHAPES[8])])
def test_s2_weight_gradient_in_a_graph(capi, dtype, shape):
    """Kernel + slab reduction captured once and replayed three times into a NaN-filled output: bit-equal to the eager result
    (no host synchronisation, no atomics, nothing that depends on the launch)."""
    gy, x, _ = problem(dtype, shape)
    eager = capi.wgrad3_s2_h(gy, x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = capi.wgrad3_s2_h(gy, x)
    for _ in range(3):
        static.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layer2_first_bottleneck_takes_the_s2_kernel(dtype):
    """The bottleneck that opens layer2 on the fused path under autocast, 8 x 256 x 16 x 16: with ROUTING.wgrad16_s2 conv2's
    weight gradient is ONE conv3x3_wgrad launch on wgrad3_h_s2_kernel, agrees with the MIOpen route (the field off) within the
    8 ULP the block tests of tests/test_conv_h_gpu.py allow a 16-bit weight gradient, and is bit-identical from run to run."""
    from peclr_amd import _capi
    from peclr_amd import bn2d as B
    from peclr_amd import resnet

    def block():             # a fresh one per run: a training pass moves the running statistics, which the fused sums are shifted by
        torch.manual_seed(3)
        ds = torch.nn.Sequential(resnet.conv1x1(256, 512, 2), B.FusedBatchNormAct2d(512))
        net = resnet.Bottleneck(256, 128, stride=2, downsample=ds, norm_layer=B.FusedBatchNormAct2d)
        net = net.to(DEV).to(memory_format=torch.channels_last).train()
        B.enable_hip_batchnorm(net)
        return net

    g = torch.Generator().manual_seed(64)
    x = nhwc((torch.randn(8, 256, 16, 16, generator=g) * 0.7 + 0.3).to(DEV).to(dtype))
    gy = nhwc(torch.randn(8, 512, 8, 8, generator=g).to(DEV))

    def run(s2):
        net = block()
        _capi.EVENT_LOG = {}
        try:
            with B.routing(force=True, wgrad16_s2=s2):
                with torch.autocast("cuda", dtype=dtype):
                    y = net(x.clone().requires_grad_())
                y.backward(gy.to(y.dtype))
                torch.cuda.synchronize()
                assert B.last_backward_leftovers == 0 and B.end_backward() == 0
            kernels = [e[4] for k, v in _capi.EVENT_LOG.items() if k.split("~")[0] == "conv3x3_wgrad" for e in v]
        finally:
            _capi.EVENT_LOG = None
        return net.conv2.weight.grad.detach().clone(), kernels

    ours, kernels = run(True)
    assert kernels == ["wgrad3_h_s2_kernel"], kernels
    again, _ = run(True)
    assert torch.equal(ours, again)
    stock, kernels = run(False)
    assert kernels == [], kernels
    rel = float((ours.double() - stock.double()).norm() / stock.double().norm())
    print(f"{dtype}: conv2.weight.grad, in-tree against MIOpen: {rel:.3e} (bar {8 * ULP[dtype]:.3e})")
    assert ours.dtype == torch.float32 and rel <= 8 * ULP[dtype], rel


class _AtenConvBackwards(TorchDispatchMode):
    """The aten convolution_backward calls that run under it: [dtype, dY shape, x shape, weight shape, stride, output mask]."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if getattr(func, "_overloadpacket", None) is torch.ops.aten.convolution_backward:
            self.seen.append([str(args[0].dtype), list(args[0].shape), list(args[1].shape), list(args[2].shape), list(args[4]), list(args[10])])
        return func(*args, **(kwargs or {}))


def test_no_3x3_stride2_weight_gradient_left_on_aten():
    """resnet50 on the fused path, bf16 autocast, one forward + backward at 16 x 3 x 224 x 224: with ROUTING.wgrad16_s2 no aten
    convolution_backward with a 3x3 weight and stride [2, 2] runs, and two passes from the same seed give bit-equal gradients
    for every parameter; with the field off exactly the three of layer2.0 / layer3.0 / layer4.0 are seen."""
    from peclr_amd import bn2d as B
    from peclr_amd import resnet

    g = torch.Generator().manual_seed(8)
    x = nhwc(torch.randn(16, 3, 224, 224, generator=g).to(DEV))
    gy = torch.randn(16, 1000, generator=g).to(DEV)

    def run(s2):
        torch.manual_seed(7)
        net = resnet.resnet50().to(DEV).to(memory_format=torch.channels_last).train()
        B.enable_hip_batchnorm(net)
        convs = _AtenConvBackwards()
        with B.routing(wgrad16_s2=s2), convs:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = net(x)
            y.backward(gy.to(y.dtype))
            B.end_backward()
        torch.cuda.synchronize()
        return {name: p.grad.detach().clone() for name, p in net.named_parameters()}, convs.seen

    def s2_3x3(seen):
        return [c for c in seen if c[3][2:] == [3, 3] and c[4] == [2, 2]]

    grads, seen = run(True)
    print("aten convolution_backward calls left with wgrad16_s2 on:", seen)
    assert s2_3x3(seen) == [], s2_3x3(seen)
    again, seen2 = run(True)
    assert seen2 == seen
    differ = [name for name in grads if not torch.equal(grads[name], again[name])]
    assert differ == [], differ
    _, seen_off = run(False)
    print("... and with it off:", seen_off)
    assert sorted(c[3] for c in s2_3x3(seen_off)) == [[128, 128, 3, 3], [256, 256, 3, 3], [512, 512, 3, 3]], seen_off
    assert all(c[5] == [False, True, False] for c in s2_3x3(seen_off))
