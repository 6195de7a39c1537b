"""The 16-bit 3x3 / padding-1 / stride-2 weight gradient (peclr_wgrad3s2_h, csrc/wgrad_h.hip: four parity planes of X through LDS
rings), the parts that need no GPU: the slab counts, the entry point's refusals (argument validation precedes any launch), the
predicate `_capi.wgrad3_s2_h_ok`, the routing switch `ROUTING.wgrad16_s2` / PECLR_WGRAD16_S2, and which path `bn2d._wgrad_h`
takes for the convolutions that open layers 2 - 4."""
import ctypes

import pytest
import torch

NULL, SHAPE, ALIGN, WORKSPACE, UNSUPPORTED = -1, -2, -3, -4, -5      # (tests/test_wgrad3_wide_host.py checks them against the header)
BF16, F16 = 1, 2
# (images, Cout, Cin, Ho, Wo) of ResNet-50's three 3x3 / stride-2 convolutions at the bench's C2 configuration (256 images of 224 px)
C2 = [(256, 128, 128, 28, 28), (256, 256, 256, 14, 14), (256, 512, 512, 7, 7)]


@pytest.fixture(scope="module")
def capi():
    from peclr_amd import _capi

    _capi.lib()
    return _capi


def policy(m, n, nb, ho, wo):
    """`w3_slabs` on the padded slots of the OUTPUT, under the kernel's 64 x 32 channel tiles: ~512 workgroups, at least sixteen
    32-slot steps per slab."""
    slots = nb * (ho + 1) * (wo + 1)
    want = max(1, min(-(-512 // ((m // 64) * (n // 32))), -(-slots // 512)))
    chunk = -(-(-(-slots // want)) // 32) * 32
    return -(-slots // chunk)


def test_slab_counts(capi):
    L = capi.lib()
    for nb, m, n, ho, wo in C2 + [(1, 64, 64, 9, 62), (512, 64, 64, 1, 1)]:
        assert L.peclr_wgrad3s2_h_slabs(m, n, nb, ho, wo) == policy(m, n, nb, ho, wo) >= 1, (m, n, nb, ho, wo)
    assert L.peclr_wgrad3s2_h_slabs(128, 128, 256, 28, 28) == 64 and L.peclr_wgrad3s2_h_slabs(512, 512, 256, 7, 7) == 4
    assert L.peclr_wgrad3s2_h_slabs(64, 64, 9, 1, 62) >= 1 and L.peclr_wgrad3s2_h_slabs(64, 64, 9, 1, 63) == 0
    assert L.peclr_wgrad3s2_h_slabs(96, 64, 8, 8, 8) == 0 and L.peclr_wgrad3s2_h_slabs(64, 96, 8, 8, 8) == 0
    assert L.peclr_wgrad3s2_h_slabs(64, 32, 8, 8, 8) == 0
    for bad in [(0, 64, 8, 8, 8), (64, 0, 8, 8, 8), (64, 64, 0, 8, 8), (64, 64, 8, 0, 8), (64, 64, 8, 8, 0), (64, 64, -1, 8, 8)]:
        assert L.peclr_wgrad3s2_h_slabs(*bad) == 0, bad
    assert L.peclr_wgrad3s2_h_slabs(64, 64, 1 << 20, 31, 31) == 0        # 2^30 padded slots: beyond the magic divisions' range
    assert L.peclr_wgrad3s2_h_slabs(64, 64, (1 << 20) - 1, 31, 31) >= 1


def test_entry_point_refuses_before_any_launch(capi):
    """No GPU here: every call below must return from the validation, in w3_check's order NULL, SHAPE, ALIGN, WORKSPACE,
    UNSUPPORTED.  The pointers are host memory, 16-byte aligned; none is ever dereferenced."""
    L = capi.lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    m, n, nb, ho, wo = 64, 64, 8, 8, 8
    ns = L.peclr_wgrad3s2_h_slabs(m, n, nb, ho, wo)
    assert ns >= 1

    def call(dtype=BF16, m=m, n=n, nb=nb, ho=ho, wo=wo, a=p, b=p, slabs=p, ns=ns, zeros=p):
        return L.peclr_wgrad3s2_h(dtype, m, n, nb, ho, wo, a, b, slabs, ns, zeros, None)

    for which in ("a", "b", "slabs", "zeros"):
        assert call(**{which: None}) == NULL, which
    assert call(a=None, wo=63) == NULL                                 # (NULL comes first)
    assert call(wo=63) == SHAPE
    assert call(wo=0) == SHAPE and call(ho=0) == SHAPE and call(nb=0) == SHAPE
    assert call(m=96) == SHAPE and call(n=96) == SHAPE and call(n=32) == SHAPE
    assert call(nb=1 << 20, ho=31, wo=31) == SHAPE                     # padded slots beyond the magic divisions' 2^30
    assert call(m=96, a=p + 2) == SHAPE                                # (SHAPE before ALIGN)
    for which in ("a", "b", "slabs", "zeros"):
        assert call(**{which: p + 2}) == ALIGN, which
    assert call(a=p + 2, ns=ns + 1) == ALIGN                           # (ALIGN before WORKSPACE)
    assert call(ns=ns + 1) == WORKSPACE and call(ns=0) == WORKSPACE
    assert call(ns=ns + 1, dtype=0) == WORKSPACE                       # (WORKSPACE before UNSUPPORTED)
    assert call(dtype=0) == UNSUPPORTED and call(dtype=7) == UNSUPPORTED


def operands(nb, cout, cin, ho, wo, dtype=torch.bfloat16, xdtype=None, h=None, w=None, cl=(True, True)):
    gy = torch.zeros(nb, cout, ho, wo, dtype=dtype)
    x = torch.zeros(nb, cin, 2 * ho if h is None else h, 2 * wo if w is None else w, dtype=xdtype or dtype)
    return (gy.contiguous(memory_format=torch.channels_last) if cl[0] else gy,
            x.contiguous(memory_format=torch.channels_last) if cl[1] else x)


def test_predicate(capi):
    refused = []

    def ok(*a, **k):
        gy, x = operands(*a, **k)
        good = capi.wgrad3_s2_h_ok(gy, x)
        assert capi.wgrad_h_ok(gy, x, 9, 2) is False                   # the stride-1 predicate keeps refusing stride 2
        if not good:
            with pytest.raises(capi.PeclrHipError):                    # ... and the wrapper raises before it touches a pointer
                capi.wgrad3_s2_h(gy, x)
            refused.append((a, k))
        return good

    for dtype in (torch.bfloat16, torch.float16):
        for shape in C2:
            assert ok(*shape, dtype=dtype), (shape, dtype)
    assert ok(9, 64, 64, 1, 62) and ok(512, 64, 64, 1, 1)
    assert not ok(8, 64, 64, 8, 8, dtype=torch.float32)
    assert not ok(8, 64, 64, 8, 8, xdtype=torch.float16) and not ok(8, 64, 64, 8, 8, dtype=torch.float16, xdtype=torch.bfloat16)
    assert not ok(8, 96, 64, 8, 8) and not ok(8, 64, 96, 8, 8) and not ok(8, 64, 32, 8, 8)
    assert not ok(9, 64, 64, 1, 63)
    assert not ok(8, 64, 64, 8, 8, h=15) and not ok(8, 64, 64, 8, 8, h=17) and not ok(8, 64, 64, 8, 8, w=15) and not ok(8, 64, 64, 8, 8, h=8, w=8)
    assert not ok(7, 64, 64, 8, 8) and not ok(2, 64, 64, 8, 8) and not ok(511, 64, 64, 1, 1)      # fewer than 512 output pixels
    assert not ok(8, 64, 64, 8, 8, cl=(False, True)) and not ok(8, 64, 64, 8, 8, cl=(True, False))
    assert len(refused) == 16


def test_routing_field_follows_environment_and_override(monkeypatch):
    """`Routing()` reads PECLR_WGRAD16_S2 when it is built (as `bn2d.ROUTING` is at import); `routing(...)` overrides and restores."""
    from peclr_amd import bn2d as B

    for value, want in (("0", False), ("1", True)):
        monkeypatch.setenv("PECLR_WGRAD16_S2", value)
        assert B.Routing().wgrad16_s2 is want
    before = B.ROUTING.wgrad16_s2
    with B.routing(wgrad16_s2=not before):
        assert B.ROUTING.wgrad16_s2 is (not before)
    assert B.ROUTING.wgrad16_s2 is before


# (images, Ho = Wo, stride, wgrad16, wgrad16_s2, force) -> route
ROUTES = [(8, 8, 2, True, True, False, "s2"), (8, 8, 2, True, False, False, "miopen"), (8, 8, 2, False, True, False, "miopen"),
          (8, 8, 2, True, False, True, "miopen"), (8, 8, 2, True, True, True, "s2"),
          (2, 8, 2, True, True, False, "miopen"), (2, 8, 2, True, True, True, "miopen"),       # 128 output pixels: aten, whatever `force` says
          (8, 8, 1, True, True, False, "wgrad_h"), (8, 8, 1, True, False, False, "wgrad_h"), (8, 8, 1, False, True, False, "miopen"),
          (2, 8, 1, True, True, True, "miopen")]


@pytest.mark.parametrize("nb,ho,stride,w16,s2,force,route", ROUTES)
def test_which_path_a_3x3_weight_gradient_takes(monkeypatch, capi, nb, ho, stride, w16, s2, force, route):
    """bn2d._wgrad_h on CPU tensors with the kernels replaced by recorders: a 3x3 / stride-2 convolution reaches
    _capi.wgrad3_s2_h only with ROUTING.wgrad16 AND ROUTING.wgrad16_s2 on a shape the predicate accepts, MIOpen (`_conv_wgrad`,
    stride (2, 2), padding (1, 1)) otherwise; stride-1 shapes go where they went, whatever the new field says."""
    from peclr_amd import bn2d as B

    calls = []
    monkeypatch.setattr(capi, "wgrad_h", lambda gy, x, taps=1, stride=1, **k: calls.append(("wgrad_h", taps, stride)) or torch.zeros(gy.shape[1], taps * x.shape[1]))
    monkeypatch.setattr(capi, "wgrad3_s2_h", lambda gy, x, **k: calls.append(("s2",)) or torch.zeros(gy.shape[1], 9 * x.shape[1]))
    monkeypatch.setattr(B, "_conv_wgrad", lambda gy, x, weight, stride, padding, param=None: calls.append(("miopen", tuple(stride), tuple(padding))) or torch.zeros_like(weight))
    conv = torch.nn.Conv2d(64, 64, 3, stride=stride, padding=1, bias=False).to(memory_format=torch.channels_last)
    gy = torch.zeros(nb, 64, ho, ho, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    x = torch.zeros(nb, 64, stride * ho, stride * ho, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert B._overlap_stream() is None
    with B.routing(wgrad16=w16, wgrad16_s2=s2, force=force):
        dw = B._wgrad_h(gy, x, conv, stride)
    assert tuple(dw.shape) == tuple(conv.weight.shape)
    want = {"s2": ("s2",), "wgrad_h": ("wgrad_h", 9, 1), "miopen": ("miopen", (stride, stride), (1, 1))}[route]
    assert calls == [want], calls
