"""The 16-bit 3x3 weight gradient for rows wider than 62 pixels (peclr_wgrad3w_h, csrc/wgrad_h.hip: column segments), the parts
that need no GPU: the entry points' refusals (argument validation precedes any launch), the slab counts, the routing switch
`ROUTING.wgrad16_wide` / PECLR_WGRAD16_WIDE, and which path `bn2d._wgrad_h` takes for a 64-pixel row."""
import ctypes
import os
import re

import pytest
import torch

from tests.conftest import ROOT

NULL, SHAPE, ALIGN, WORKSPACE, UNSUPPORTED = -1, -2, -3, -4, -5
BF16, F16 = 1, 2
DEFAULT_ON = True        # profiles/wgrad3_wide_timing.txt decided it: in-tree is faster at both shapes, in both formats


@pytest.fixture(scope="module")
def capi():
    from peclr_amd import _capi

    _capi.lib()
    return _capi


def test_error_codes_are_the_headers(capi):
    """(the constants above are the header's PECLR_ERR_* / PECLR_DTYPE_* values)"""
    text = open(os.path.join(ROOT, "include", "peclr_hip.h")).read()
    values = {k: int(v) for k, v in re.findall(r"#define\s+(PECLR_(?:ERR|DTYPE)_\w+)\s+\(?(-?\d+)\)?", text)}
    assert (values["PECLR_ERR_NULL"], values["PECLR_ERR_SHAPE"], values["PECLR_ERR_ALIGN"], values["PECLR_ERR_WORKSPACE"],
            values["PECLR_ERR_UNSUPPORTED"]) == (NULL, SHAPE, ALIGN, WORKSPACE, UNSUPPORTED)
    assert (values["PECLR_DTYPE_BF16"], values["PECLR_DTYPE_F16"]) == (BF16, F16)


def test_wide_entry_points_refuse_before_any_launch(capi):
    """No GPU here: every call below must return from the validation, in the header's order NULL, SHAPE, ALIGN, WORKSPACE,
    UNSUPPORTED.  The pointers are host memory, 16-byte aligned; none is ever dereferenced."""
    L = capi.lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    m, n, nb, h, w = 64, 64, 1, 5, 112
    ns = L.peclr_wgrad3w_h_slabs(m, n, nb, h, w)
    assert ns >= 1

    def call(dtype=BF16, m=m, n=n, nb=nb, h=h, w=w, a=p, b=p, slabs=p, ns=ns, zeros=p):
        return L.peclr_wgrad3w_h(dtype, m, n, nb, h, w, a, b, slabs, ns, zeros, None)

    for which in ("a", "b", "slabs", "zeros"):
        assert call(**{which: None}) == NULL, which
    assert call(a=None, w=62) == NULL                                  # (NULL comes first)
    assert call(w=62) == SHAPE                                         # the one-ring entry point's rows
    assert call(w=capi.WGRAD3W_MAX_W + 1) == SHAPE
    assert call(w=0) == SHAPE and call(h=0) == SHAPE and call(nb=0) == SHAPE
    assert call(m=96) == SHAPE and call(n=96) == SHAPE
    assert call(nb=1 << 20, h=63, w=512) == SHAPE                      # padded slots beyond the magic divisions' 2^30
    assert call(m=96, a=p + 2) == SHAPE                                # (SHAPE before ALIGN)
    for which in ("a", "b", "slabs", "zeros"):
        assert call(**{which: p + 2}) == ALIGN, which
    assert call(a=p + 2, ns=ns + 1) == ALIGN                           # (ALIGN before WORKSPACE)
    assert call(ns=ns + 1) == WORKSPACE and call(ns=0) == WORKSPACE
    assert call(ns=ns + 1, dtype=0) == WORKSPACE                       # (WORKSPACE before UNSUPPORTED)
    assert call(dtype=0) == UNSUPPORTED and call(dtype=7) == UNSUPPORTED


def test_slab_counts(capi):
    L = capi.lib()
    assert L.peclr_wgrad3w_h_slabs(64, 64, 1, 5, 112) >= 1
    assert L.peclr_wgrad3w_h_slabs(64, 64, 1, 5, 62) == 0
    assert L.peclr_wgrad3w_h_slabs(64, 64, 1, 5, capi.WGRAD3W_MAX_W) >= 1
    assert L.peclr_wgrad3w_h_slabs(64, 64, 1, 5, capi.WGRAD3W_MAX_W + 1) == 0
    assert L.peclr_wgrad3w_h_slabs(96, 64, 1, 5, 112) == 0 and L.peclr_wgrad3w_h_slabs(64, 96, 1, 5, 112) == 0
    assert L.peclr_wgrad3w_h_slabs(64, 64, 1 << 20, 63, 512) == 0
    # the policy of peclr_wgrad3_h_slabs on the segmented slot count: ~512 workgroups, at least sixteen 32-slot steps per slab
    for m, n, nb, h, w in [(64, 64, 1, 5, 112), (64, 64, 128, 112, 112), (128, 64, 2, 40, 112), (256, 256, 3, 7, 63), (64, 64, 128, 64, 64)]:
        nseg = (w + 60) // 61
        slots = nb * nseg * (h + 1) * ((w + nseg - 1) // nseg + 2)
        want = max(1, min(-(-512 // ((m // 64) * (n // 64))), -(-slots // 512)))
        chunk = -(-(-(-slots // want)) // 32) * 32
        assert L.peclr_wgrad3w_h_slabs(m, n, nb, h, w) == -(-slots // chunk), (m, n, nb, h, w)
    # the old entry point keeps its range
    assert L.peclr_wgrad3_h_slabs(64, 64, 1, 5, 63) == 0 and L.peclr_wgrad3_h_slabs(64, 64, 4, 5, 62) >= 1
    assert L.peclr_wgrad3_h(BF16, 64, 64, 4, 5, 63, 16, 16, 16, 1, 16, None) == SHAPE


def test_wgrad_h_ok_takes_wide_rows(capi):
    def ok(w, cout=64, cin=64, nb=2, h=8, dtype=torch.bfloat16, taps=9, stride=1):
        gy = torch.zeros(nb, cout, h, w, dtype=dtype).contiguous(memory_format=torch.channels_last)
        x = torch.zeros(nb, cin, h * stride, w * stride, dtype=dtype).contiguous(memory_format=torch.channels_last)
        return capi.wgrad_h_ok(gy, x, taps, stride)

    assert ok(62) and ok(63) and ok(64) and ok(112) and ok(capi.WGRAD3W_MAX_W) and not ok(capi.WGRAD3W_MAX_W + 1)
    assert ok(64, dtype=torch.float16) and not ok(64, dtype=torch.float32)
    assert not ok(64, cout=96) and not ok(64, cin=32) and not ok(64, stride=2)
    assert not ok(64, nb=1, h=7)                                       # fewer than 512 pixels: unchanged


def test_routing_field_follows_environment_and_override(monkeypatch):
    """`Routing()` reads PECLR_WGRAD16_WIDE when it is built (as `bn2d.ROUTING` is at import); `routing(...)` overrides and restores."""
    from peclr_amd import bn2d as B

    for value, want in (("0", False), ("1", True)):
        monkeypatch.setenv("PECLR_WGRAD16_WIDE", value)
        assert B.Routing().wgrad16_wide is want
    monkeypatch.delenv("PECLR_WGRAD16_WIDE")
    assert B.Routing().wgrad16_wide is DEFAULT_ON
    before = B.ROUTING.wgrad16_wide
    with B.routing(wgrad16_wide=not before):
        assert B.ROUTING.wgrad16_wide is (not before)
    assert B.ROUTING.wgrad16_wide is before


@pytest.mark.parametrize("w,wide,route", [(64, True, "wgrad_h"), (64, False, "miopen"), (112, True, "wgrad_h"), (112, False, "miopen"),
                                          (62, True, "wgrad_h"), (62, False, "wgrad_h")])
def test_which_path_a_wide_3x3_weight_gradient_takes(monkeypatch, capi, w, wide, route):
    """bn2d._wgrad_h on CPU tensors with the kernels replaced by recorders: a 3x3 / stride-1 convolution whose rows are wider
    than 62 pixels reaches _capi.wgrad_h only with ROUTING.wgrad16_wide, MIOpen (`_conv_wgrad`) otherwise; narrower rows do
    not look at the field."""
    from peclr_amd import bn2d as B

    calls = []
    real_ok = capi.wgrad_h_ok
    monkeypatch.setattr(capi, "wgrad_h_ok", lambda *a, **k: calls.append("wgrad_h_ok") or real_ok(*a, **k))
    monkeypatch.setattr(capi, "wgrad_h", lambda gy, x, taps=1, stride=1, **k: calls.append(("wgrad_h", taps, stride)) or torch.zeros(gy.shape[1], taps * x.shape[1]))
    monkeypatch.setattr(B, "_conv_wgrad", lambda gy, x, weight, stride, padding, param=None: calls.append(("miopen", tuple(stride), tuple(padding))) or torch.zeros_like(weight))
    conv = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False).to(memory_format=torch.channels_last)
    x = torch.zeros(2, 64, 5, w, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    gy = torch.zeros(2, 64, 5, w, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert B._overlap_stream() is None
    with B.routing(wgrad16=True, wgrad16_wide=wide):
        dw = B._wgrad_h(gy, x, conv, 1)
    assert tuple(dw.shape) == tuple(conv.weight.shape)
    assert calls[-1] == (("wgrad_h", 9, 1) if route == "wgrad_h" else ("miopen", (1, 1), (1, 1))), calls
    assert len([c for c in calls if c != "wgrad_h_ok"]) == 1
    with B.routing(wgrad16=False, wgrad16_wide=wide):                  # the 16-bit switch as a whole still rules
        del calls[:]
        B._wgrad_h(gy, x, conv, 1)
    assert calls == [("miopen", (1, 1), (1, 1))]
