"""peclr_wgrad3w_h (csrc/wgrad_h.hip, wgrad3_h_kernel<F16, W3WArgs>): the 16-bit 3x3 / padding-1 / stride-1 weight gradient for rows wider
than 62 pixels -- every image cut into column segments, each a pseudo-image of the padded pixel space whose halo slots hold
zero for dY and the neighbouring segment's pixels for X -- against float64 on the SAME 16-bit inputs (`-m gpu`).  The bar is
test_wgrad3_h_matches_float64's (tests/test_conv_h_gpu.py): fp32 accumulation of exact 16-bit products,
max |got - ref| <= 3e-6 max |ref| max(1, sqrt(pixels / 4096)).
Replaces MIOpen's 16-bit weight gradient of layer1's 3x3 convolutions for inputs above 248 px (torchvision's Bottleneck behind
the reference's resnet_model.py under `precision: 16`)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.bfloat16, torch.float16]

# (nb, cout, cin, h, w): the smallest shapes that meet each way the segmentation can go wrong
SHAPES = [(1, 64, 64, 9, 63),          # first width the one-ring kernel refuses; segments of 32 and 31 columns
          (2, 64, 64, 4, 64),          # 256 x 256 input; an image boundary
          (5, 64, 64, 1, 112),         # H = 1: every tap row but the middle one is padding
          (1, 128, 64, 5, 112), (1, 64, 128, 5, 112),      # tile indexing in M and in N
          (3, 64, 64, 2, 100),
          (1, 64, 64, 5, 123),         # three segments
          (2, 64, 64, 3, 127),
          (1, 64, 64, 2, 256),         # five segments
          (2, 64, 64, 40, 112),        # several slabs: boundaries inside segment rows and between pseudo-images
          (1, 64, 64, 1, 512)]         # the widest row the entry point takes: nine segments


@pytest.fixture(scope="module")
def capi():
    from peclr_amd import _capi

    _capi.lib()
    return _capi


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def bar(nb, h, w):
    return 3e-6 * max(1.0, (nb * h * w / 4096) ** 0.5)


def reference(gy, x):
    """[Cout, Cin, 3, 3] in float64 from the 16-bit operands."""
    wz = torch.zeros(gy.shape[1], x.shape[1], 3, 3, device=gy.device, dtype=torch.float64)
    return torch.ops.aten.convolution_backward(gy.double(), x.double(), wz, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


def as_weight(dw, cout, cin):
    return dw.view(cout, 3, 3, cin).permute(0, 3, 1, 2).double()


@functools.lru_cache(maxsize=None)
def problem(dtype, shape):
    """(gy, x, float64 reference) of one shape: built once, shared by the tests below, never written to."""
    nb, cout, cin, h, w = shape
    g = torch.Generator(device=DEV).manual_seed(nb + cout + cin + h + w)
    x = nhwc(torch.randn(nb, cin, h, w, device=DEV, generator=g).to(dtype))
    gy = nhwc(torch.randn(nb, cout, h, w, device=DEV, generator=g).to(dtype))
    return gy, x, reference(gy, x)


def rel_err(got, ref):
    return float((got - ref).abs().max()) / float(ref.abs().max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_wgrad3_wide_matches_float64(capi, dtype, shape):
    nb, cout, cin, h, w = shape
    gy, x, ref = problem(dtype, shape)
    assert capi.wgrad_h_ok(gy, x, 9, 1)
    dw = capi.wgrad_h(gy, x, 9, 1)
    assert dw.shape == (cout, 9 * cin) and dw.dtype == torch.float32
    err = rel_err(as_weight(dw, cout, cin), ref)
    print(f"{shape} {dtype}: {err:.3e} of the scale (bar {bar(nb, h, w):.3e}), {capi.lib().peclr_wgrad3w_h_slabs(cout, cin, nb, h, w)} slabs")
    assert err <= bar(nb, h, w), err
    for _ in range(4):
        assert torch.equal(capi.wgrad_h(gy, x, 9, 1), dw)


# (w, columns either side of a seam): 112 = 56 + 56, 123 = 41 + 41 + 41, 63 = 32 + 31, 127 = 43 + 42 + 42
SEAMS = [(112, 55, 56), (123, 40, 41), (123, 81, 82), (63, 31, 32), (127, 42, 43), (127, 84, 85)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w,left,right", SEAMS)
def test_segment_seams_read_the_neighbouring_segment(capi, dtype, w, left, right):
    """dY one-hot at the last pixel of a segment, then at the first of the next one, in a middle row of the second image: every
    tap of dW is dY's value times ONE pixel of X -- for the taps that cross the seam a pixel of the neighbouring segment, which
    the halo slot of X must hold (and dY's halo slot must not: the pixel would count twice)."""
    nb, c, h = 2, 64, 5
    g = torch.Generator(device=DEV).manual_seed(w + left)
    x = nhwc(torch.randn(nb, c, h, w, device=DEV, generator=g).to(dtype))
    val = torch.randn(c, device=DEV, generator=g).to(dtype)
    for col in (left, right):
        gy = nhwc(torch.zeros(nb, c, h, w, device=DEV, dtype=dtype))
        gy[1, :, 2, col] = val
        assert capi.wgrad_h_ok(gy, x, 9, 1)
        got, ref = as_weight(capi.wgrad_h(gy, x, 9, 1), c, c), reference(gy, x)
        patch = x[1, :, 1:4, col - 1:col + 2].double()                        # [Cin, 3, 3]: what the nine taps meet
        assert rel_err(ref, val.double().view(c, 1, 1, 1) * patch.unsqueeze(0)) <= 1e-14
        assert rel_err(got, ref) <= bar(nb, h, w), (col, rel_err(got, ref))


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
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[6], SHAPES[7]], ids=lambda s: "x".join(map(str, s)))
def test_padding_is_zero_not_memory(capi, dtype, shape):
    """The operands as interior views of buffers filled with 1e4: a fetch outside an image (a padding row, a column outside
    the image, a slot before the first or after the last pixel) would show as an error of ~1e4 times the scale."""
    nb, cout, cin, h, w = shape
    gy, x, ref = problem(dtype, shape)
    dw = capi.wgrad_h(embedded(gy), embedded(x), 9, 1)
    assert rel_err(as_weight(dw, cout, cin), ref) <= bar(nb, h, w)
    assert torch.equal(dw, capi.wgrad_h(gy, x, 9, 1))


@pytest.mark.parametrize("dtype,shape", [(torch.bfloat16, SHAPES[1]), (torch.float16, SHAPES[6])])
def test_wide_weight_gradient_in_a_graph(capi, dtype, shape):
    """Kernel + slab reduction captured once and replayed three times: bit-equal to the eager result (no host synchronisation,
    no atomics, nothing that depends on the launch)."""
    gy, x, _ = problem(dtype, shape)
    eager = capi.wgrad_h(gy, x, 9, 1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = capi.wgrad_h(gy, x, 9, 1)
    for _ in range(3):
        static.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layer1_bottleneck_takes_the_wide_kernel(dtype):
    """One layer1 bottleneck on the fused path under autocast, 2 x 256 x 64 x 64: with ROUTING.wgrad16_wide conv2's weight
    gradient is ONE conv3x3_wgrad launch on wgrad3_h_kernel's segmented route, agrees with the MIOpen route (the field off) within the 8 ULP the
    block tests of tests/test_conv_h_gpu.py allow a 16-bit weight gradient, and is bit-identical from run to run."""
    from peclr_amd import _capi
    from peclr_amd import bn2d as B
    from peclr_amd import resnet

    def block():             # a fresh one per run: a training pass moves the running statistics, which the fused sums are shifted by
        torch.manual_seed(3)
        net = resnet.Bottleneck(256, 64, norm_layer=B.FusedBatchNormAct2d).to(DEV).to(memory_format=torch.channels_last).train()
        B.enable_hip_batchnorm(net)
        return net

    g = torch.Generator().manual_seed(64)
    x = nhwc((torch.randn(2, 256, 64, 64, generator=g) * 0.7 + 0.3).to(DEV).to(dtype))
    gy = nhwc(torch.randn(2, 256, 64, 64, generator=g).to(DEV))

    def run(wide):
        net = block()
        _capi.EVENT_LOG = {}
        try:
            with B.routing(force=True, wgrad16_wide=wide):
                with torch.autocast("cuda", dtype=dtype):
                    y = net(x.clone().requires_grad_())
                y.backward(gy.to(y.dtype))
                torch.cuda.synchronize()
                assert B.last_backward_leftovers == 0 and B.end_backward() == 0
            kernels = [e[4] for k, v in _capi.EVENT_LOG.items() if k.split("~")[0] == "conv3x3_wgrad" for e in v]
        finally:
            _capi.EVENT_LOG = None
        return net.conv2.weight.grad.detach().clone(), kernels

    wide, kernels = run(True)
    assert kernels == ["wgrad3_h_kernel (segments)"], kernels
    again, _ = run(True)
    assert torch.equal(wide, again)
    stock, kernels = run(False)
    assert kernels == [], kernels
    rel = float((wide.double() - stock.double()).norm() / stock.double().norm())
    print(f"{dtype}: conv2.weight.grad, in-tree against MIOpen: {rel:.3e} (bar {8 * ULP[dtype]:.3e})")
    assert wide.dtype == torch.float32 and rel <= 8 * ULP[dtype], rel
