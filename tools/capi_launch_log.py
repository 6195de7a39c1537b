#!/usr/bin/env python
"""Record what peclr_amd/_capi.py hands to libpeclr_hip.so: every wrapper once per branch, on small seeded inputs.

    python tools/capi_launch_log.py OUT.json [label of the tree, e.g. its commit]

A forwarding proxy over `_capi._LIB` notes every native call; EVENT_LOG / LAUNCH_ORDER give the timed launches.  Per wrapper
call the log holds `native`: [[entry point, summarised arguments], ...] and `timed`: [[tag, nbytes, flops, kernel], ...] in
launch order.  Arguments: integers and floats literally; a pointer as null, as "<input name>+<byte offset>" when it lies in a
named input tensor, as "ret<i>+<byte offset>" when it lies in the i-th tensor the wrapper returned, else "tmp<k>" (numbered by
first appearance in that wrapper call; tensors made during the call are kept alive until it is summarised); a struct passed by reference as {"struct": [its fields]}; a host array as "host".
Two trees marshal alike exactly when their logs are equal: tests/golden/capi_launch_log.json is the log of the commit named
in its first key, tests/test_capi_launch_log_gpu.py compares the working tree with it.  Only public names of _capi, `lib()`
and `_LIB` are used, so this file runs unchanged on an older tree."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

from peclr_amd import _capi  # noqa: E402

DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


class _Proxy:
    """Stands in for the CDLL: forwards every call, noting those of declared entry points."""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in _capi.SIGNATURES:
            return fn

        def forward(*args):
            self._calls.append((name, [_raw(a, ty is ctypes.c_void_p) for a, ty in zip(args, _capi.SIGNATURES[name][1])]))
            return fn(*args)

        return forward


def _raw(a, is_ptr):
    if a is None:
        return None
    if isinstance(a, ctypes.c_void_p):                   # ctypes.cast(host array, c_void_p)
        return "host"
    if type(a).__name__ == "CArgObject":                 # ctypes.byref(struct)
        s = a._obj
        return {"struct": [_raw(getattr(s, f), ty is ctypes.c_void_p) for f, ty in s._fields_]}
    if is_ptr:
        return ("ptr", int(a)) if int(a) else None
    return float(a) if isinstance(a, float) else int(a)


def _span(t):
    if t.numel() == 0:
        return 0
    return (1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))) * t.element_size()


def _tensors(obj):
    """The tensors (or None) of a wrapper's return value, in order."""
    if obj is None or isinstance(obj, torch.Tensor):
        return [obj]
    if isinstance(obj, dict):
        return [t for v in obj.values() for t in _tensors(v)]
    if isinstance(obj, (tuple, list)):
        return [t for v in obj for t in _tensors(v)]
    return []


def _resolve(native, inputs, ret):
    regions = [(name, t.data_ptr(), _span(t)) for name, t in inputs.items() if isinstance(t, torch.Tensor) and t.is_cuda]
    regions += [(f"ret{i}", t.data_ptr(), _span(t)) for i, t in enumerate(_tensors(ret)) if t is not None and t.is_cuda]
    tmp = {}

    def label(v):
        if isinstance(v, dict):
            return {"struct": [label(f) for f in v["struct"]]}
        if not (isinstance(v, tuple) and v[0] == "ptr"):
            return v
        for name, start, span in regions:
            if start <= v[1] < start + max(span, 1):
                return f"{name}+{v[1] - start}"
        return tmp.setdefault(v[1], f"tmp{len(tmp)}")

    return [[name, [label(v) for v in args]] for name, args in native]


class _KeepAlive(TorchDispatchMode):
    """Holds every tensor made during one wrapper call until the call has been summarised: no temporary is freed meanwhile, so the
    allocator cannot hand a temporary's address to a tensor the wrapper returns, and "tmp" / "ret" never depend on its state."""

    def __init__(self):
        super().__init__()
        self.kept = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        self.kept.append(out)
        return out


class Recorder:
    def __init__(self):
        self.calls, self.cases, self.errors = [], [], []

    def __call__(self, label, fn, **inputs):
        """Run one wrapper call `fn` whose tensor arguments are `inputs` (by role name); returns what it returned."""
        torch.cuda.synchronize()
        del self.calls[:]
        _capi.EVENT_LOG, _capi.LAUNCH_ORDER = {}, []
        keep = _KeepAlive()
        try:
            with keep:
                ret = fn()
        except _capi.PeclrHipError as e:                  # a refused call is part of the record (and a finding: see `record`)
            self.cases.append({"case": label, "error": str(e)})
            self.errors.append(f"{label}: {e}")
            return None
        seen, timed = {}, []
        for tag in _capi.LAUNCH_ORDER:
            i = seen[tag] = seen.get(tag, -1) + 1
            timed.append([tag, *_capi.EVENT_LOG[tag][i][2:]])
        self.cases.append({"case": label, "native": _resolve(self.calls, inputs, ret), "timed": timed})
        return ret


def rnd(*shape, seed=0, dtype=F32, scale=1.0):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def bn_tables(x2d):
    """(save [mean, invstd], scale_shift) of the columns of a [rows, C] matrix, gamma 1 and beta 0."""
    xf = x2d.float()
    mean, invstd = xf.mean(0), 1.0 / (xf.var(0, unbiased=False) + 1e-5).sqrt()
    return torch.stack([mean, invstd]).contiguous(), torch.stack([invstd, -mean * invstd]).contiguous()


# ------------------------------------------------------------------ the projection head, the loss and the optimiser
def head(rec):
    c = _capi
    m, n, k = 12, 96, 48
    bias = rnd(n, seed=3)
    for name, layout, a, b in (("nt", c.GEMM_NT, rnd(m, k, seed=1), rnd(n, k, seed=2)), ("nn", c.GEMM_NN, rnd(m, k, seed=1), rnd(k, n, seed=2)),
                               ("tn", c.GEMM_TN, rnd(k, m, seed=1), rnd(k, n, seed=2))):
        rec(f"gemm {name}", lambda: c.gemm(layout, a, b), a=a, b=b)
        rec(f"gemm {name} bias", lambda: c.gemm(layout, a, b, bias), a=a, b=b, bias=bias)
        rec(f"gemm {name} split_k 3", lambda: c.gemm(layout, a, b, split_k=3, tag="probe"), a=a, b=b)
        rec(f"gemm {name} split_k 3 bias", lambda: c.gemm(layout, a, b, bias, split_k=3), a=a, b=b, bias=bias)
    rec("pick_split_k", lambda: c.pick_split_k(256, 512, 2048))
    slabs, sbias = rnd(2, 5, 12, seed=31), rnd(12, seed=32)
    rec("slab_reduce", lambda: c.slab_reduce(slabs), slabs=slabs)
    rec("slab_reduce bias", lambda: c.slab_reduce(slabs, sbias, tag="probe"), slabs=slabs, bias=sbias)

    m, h = 12, 96
    parts, bias, gamma, beta = rnd(1, m, h, seed=10), rnd(h, seed=11), 0.5 + rnd(h, seed=12).abs(), rnd(h, seed=13, scale=0.2)
    rm, rv, nbt = rnd(h, seed=14, scale=0.1), 1.0 + rnd(h, seed=15, scale=0.1).abs(), torch.zeros((), dtype=torch.int64, device=DEV)
    named = dict(a_slabs=parts, bias=bias, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, nbt=nbt)
    a_pre, a_out, save = rec("bn_relu_fwd train", lambda: c.bn_relu_fwd(parts, bias, gamma, beta, 1e-5, 0.1, True, rm, rv, nbt), **named)
    rec("bn_relu_fwd eval", lambda: c.bn_relu_fwd(parts, bias, gamma, beta, 1e-5, 0.1, False, rm, rv, nbt), **named)
    da = rnd(m, h, seed=16)
    for training in (True, False):
        rec(f"bn_relu_bwd training={training}", lambda: c.bn_relu_bwd(da, a_pre, save, gamma, beta, training),
            d_a_out=da, a_pre=a_pre, save=save, gamma=gamma, beta=beta)

    n = 3
    p_slabs = rnd(1, 2 * n, 128, seed=20)
    g = np.random.default_rng(21)
    jit = tuple(torch.from_numpy(g.integers(-14, 1, n)).to(DEV) for _ in range(4))
    ang = tuple(torch.from_numpy(g.integers(-45, 46, n).astype(np.float64)).to(DEV) for _ in range(2))
    named = dict(p_slabs=p_slabs, jx1=jit[0], jx2=jit[1], jy1=jit[2], jy2=jit[3], a1=ang[0], a2=ang[1])
    flags = c.ALIGN_CROP | c.ALIGN_ROTATE
    p, z, norms, row_stats = rec("align_fwd crop rotate", lambda: c.align_fwd(p_slabs, n, flags, jit, (224, 448), ang), **named)
    dz = rnd(2 * n, 128, seed=22)
    rec("align_bwd crop rotate", lambda: c.align_bwd(dz, p, z, norms, n, flags, ang), dz=dz, p=p, z=z, norms=norms, a1=ang[0], a2=ang[1])
    p1, z1, norms1, _ = rec("align_fwd single norm", lambda: c.align_fwd(p_slabs, n, c.ALIGN_SINGLE_NORM, None, (1, 1), None, want_stats=False),
                            p_slabs=p_slabs)
    rec("align_bwd single norm", lambda: c.align_bwd(dz, p1, z1, norms1, n, c.ALIGN_SINGLE_NORM, None), dz=dz, p=p1, z=z1, norms=norms1)

    one = torch.full((1,), 0.37, device=DEV)
    for n_half, zz, stats in ((n, z, row_stats), (128, torch.nn.functional.normalize(rnd(256, 128, seed=40)).contiguous(), None)):
        mg = 2 * n_half
        rec(f"ntxent_jsplit {mg}", lambda: (c.ntxent_jsplit(mg, mg, False), c.ntxent_jsplit(mg, mg, True)))
        rec(f"ntxent_fwd {mg} sim", lambda: c.ntxent_fwd(zz, 0, zz, n_half, 2.0, 1.0 / mg, None, 0, want_sim=True), z_rows=zz)
        _, lse, _ = rec(f"ntxent_fwd {mg} statistics={stats is not None}",
                        lambda: c.ntxent_fwd(zz, 0, zz, n_half, 2.0, 1.0 / mg, stats, n_half if stats is not None else 0),
                        z_rows=zz, row_stats=stats)
        rec(f"ntxent_bwd {mg}", lambda: c.ntxent_bwd(zz, 0, zz, n_half, 2.0, lse, one, 1.0 / mg), z_rows=zz, lse_all=lse, dloss=one)

    # the fused optimiser on the tensors of tests/test_hip_parity.py's LARS test: two groups, a channels_last filter, a zero tensor
    shapes = [(64, 3, 7, 7), (64,), (5000,), (512, 2048), (1,), (4097,)]
    params = [rnd(*s, seed=70 + i) for i, s in enumerate(shapes)]
    params[0], params[1] = nhwc(params[0]), torch.zeros_like(params[1])
    grads = [torch.randn_like(t) for t in params]
    m1, m2 = [torch.zeros_like(t) for t in params], [torch.zeros_like(t) for t in params]
    sizes = [t.numel() for t in params]
    chunk_tensor, chunk_offset, begin = [], [], [0]
    for t, sz in enumerate(sizes):
        chunk_tensor += [t] * len(range(0, sz, c.OPT_CHUNK))
        chunk_offset += list(range(0, sz, c.OPT_CHUNK))
        begin.append(len(chunk_tensor))
    wl = dict(ptrs=torch.tensor([t.data_ptr() for seq in (params, grads, m1, m2) for t in seq], dtype=torch.int64, device=DEV),
              sizes=torch.tensor(sizes, dtype=torch.int64, device=DEV), chunk_tensor=torch.tensor(chunk_tensor, dtype=torch.int32, device=DEV),
              chunk_offset=torch.tensor(chunk_offset, dtype=torch.int64, device=DEV), begin=torch.tensor(begin, dtype=torch.int32, device=DEV),
              group=torch.tensor([0, 0, 0, 1, 1, 1], dtype=torch.int32, device=DEV),
              norms_ws=torch.empty(2 * len(chunk_tensor), dtype=torch.float32, device=DEV))
    hyper = torch.zeros(18, device=DEV)
    hyper[0], hyper[1], hyper[16], hyper[17] = 1.1e-3, 1.1e-3, 0.1, 0.001
    amp_state = torch.zeros(4, dtype=torch.int32, device=DEV)
    amp_state.view(torch.float32)[0] = 65536.0

    def step(lars, **kw):
        epoch = c.WEIGHTS_EPOCH
        c.lars_adam_step(wl["ptrs"], wl["sizes"], len(params), wl["chunk_tensor"], wl["chunk_offset"], wl["begin"], wl["group"], len(chunk_tensor),
                         wl["norms_ws"], [1.1e-3, 1.1e-3], [1e-6, 0.0], 0.9, 0.999, 1e-8, 0.1, 0.001, lars, 0.02, 1e-8, True, **kw)
        return c.WEIGHTS_EPOCH - epoch

    for lars in (1, 0):
        assert rec(f"lars_adam_step lars={lars}", lambda: step(lars), **wl) == 1
    rec("lars_adam_step device hyper-parameters", lambda: step(1, device_hyper=hyper), hyper=hyper, **wl)
    rec("lars_adam_step amp", lambda: step(1, amp=(amp_state, 2.0, 0.5, 2000)), amp_state=amp_state, **wl)

    m, n, k = 8200, 1100, 100
    a, b, d = rnd(m, k, seed=21), rnd(k, n, seed=24), rnd(m, n, seed=25)
    rec("gemm_add nn", lambda: c.gemm_add(c.GEMM_NN, a, b, d), a=a, b=b, addend=d)
    m, n, k = 300, 132, 64
    a, bt, d = rnd(m, k, seed=1), rnd(n, k, seed=2), rnd(m, n, seed=3)
    rec("gemm_x6", lambda: c.gemm_x6(a, bt), a=a, b_t=bt)
    out = torch.empty((m, n), device=DEV)
    rec("gemm_x6 addend out", lambda: c.gemm_x6(a, bt, d, tag="probe", out=out), a=a, b_t=bt, addend=d, out=out)
    a, b = rnd(8196, 132, seed=4), rnd(8196, 260, seed=5)
    rec("gemm_x6_tn", lambda: c.gemm_x6_tn(a, b), a=a, b=b)
    for half, name in ((BF16, "bf16"), (F16, "fp16")):
        a, bt, d = rnd(300, 64, seed=1, dtype=half), rnd(128, 64, seed=2, dtype=half), rnd(300, 128, seed=3, dtype=half)
        rec(f"gemm_add_half {name}", lambda: c.gemm_add_half(a, bt, d), a=a, b_t=bt, addend=d)
        rec(f"gemm_add_half {name} no addend", lambda: c.gemm_add_half(a, bt, None, tag="probe"), a=a, b_t=bt)


# ------------------------------------------------------------------ the six-product GEMMs and convolutions (fp32)
def x6(rec):
    c = _capi
    w0, w1 = rnd(128, 64, seed=50, scale=0.05), rnd(64, 128, seed=51, scale=0.05)
    for pair in (False, True):
        pk = rec(f"X6Planes pair={pair}", lambda: c.X6Planes([(w0, False), (w1, True)], pair=pair), w0=w0, w1=w1)
        named = dict(w0=w0, w1=w1, table=pk.table, planes0=pk.planes[0], planes1=pk.planes[1])
        if pair:
            named.update(absmax=pk.absmax, scales=pk.scales)
        rec(f"X6Planes.pack pair={pair}", lambda: pk.pack() and None, **named)
        assert (pk.count, pk.shapes, pk.pair, pk.nbytes) == (2, [(128, 64), (128, 64)], pair, pk.planes[0].numel() * 2 + 4 * 2 * 128 * 64)
    triple = c.X6Planes([(w0, False)]).pack()
    paired = c.X6Planes([(w0, False)], pair=True).pack()

    def gemm_modes(m, s2):
        a, n = rnd(m, 64, seed=52), 128
        planes = triple.planes[0]
        named = dict(a=a, planes=planes)
        addend, shift, x = rnd(m, n, seed=53), rnd(n, seed=54, scale=0.1), rnd(m, n, seed=55)
        save, ss = bn_tables(x)
        mask = torch.randint(-2 ** 31, 2 ** 31 - 1, (m, n // 32), dtype=torch.int32).to(DEV)
        if s2 is not None:
            compact = rnd(m // 4, n, seed=56)
            rec(f"gemm_x6p {m} addend_s2", lambda: c.gemm_x6p(a, planes, n, compact, addend_s2=s2), addend=compact, **named)
            rec(f"gemm_x6p {m} addend_s2 bn_bwd", lambda: c.gemm_x6p(a, planes, n, compact, addend_s2=s2, bn_bwd=(x, save, ss, None, True)),
                addend=compact, x=x, save=save, ss=ss, **named)
            return
        rec(f"gemm_x6p {m}", lambda: c.gemm_x6p(a, planes, n), **named)
        rec(f"gemm_x6p {m} addend", lambda: c.gemm_x6p(a, planes, n, addend, tag="probe", tile_rows=128), addend=addend, **named)
        rec(f"gemm_x6p {m} stat_shift", lambda: c.gemm_x6p(a, planes, n, stat_shift=shift), stat_shift=shift, **named)
        rec(f"gemm_x6p {m} bn_bwd", lambda: c.gemm_x6p(a, planes, n, bn_bwd=(x, save, ss, None, True)), x=x, save=save, ss=ss, **named)
        rec(f"gemm_x6p {m} bn_bwd mask", lambda: c.gemm_x6p(a, planes, n, addend, bn_bwd=(x, save, ss, mask, True)),
            addend=addend, x=x, save=save, ss=ss, mask=mask, **named)
        rec(f"gemm_x6p {m} addend_mask", lambda: c.gemm_x6p(a, planes, n, addend, addend_mask=mask), addend=addend, addend_mask=mask, **named)
        rec(f"gemm_x6p {m} addend_mask bn_bwd", lambda: c.gemm_x6p(a, planes, n, addend, addend_mask=mask, bn_bwd=(x, save, ss, None, False)),
            addend=addend, addend_mask=mask, x=x, save=save, ss=ss, **named)
        amax, scale = a.abs().max().reshape(1), paired.scale(0)
        pn = dict(a=a, planes=paired.planes[0], a_absmax=amax, w_scale=scale)
        rec(f"gemm_x6p {m} pair", lambda: c.gemm_x6p(a, paired.planes[0], n, pair=(amax, scale)), **pn)
        rec(f"gemm_x6p {m} pair stat_shift", lambda: c.gemm_x6p(a, paired.planes[0], n, stat_shift=shift, pair=(amax, scale)), stat_shift=shift, **pn)

    gemm_modes(300, None)
    gemm_modes(2 * 12 * 12, (12, 12))

    nb, cin, cout, h, w = 3, 64, 64, 7, 7
    w4 = nhwc(rnd(cout, cin, 3, 3, seed=60, scale=0.05)).permute(0, 2, 3, 1)
    pk = c.X6Planes([(w4.reshape(cout, 9 * cin), False), (w4.reshape(cout * 9, cin), 9)]).pack()
    pp = c.X6Planes([(w4.reshape(cout, 9 * cin), False)], pair=True).pack()
    x, gy = nhwc(rnd(nb, cin, h, w, seed=61)), nhwc(rnd(nb, cout, h, w, seed=62))
    addend, shift = nhwc(rnd(nb, cout, h, w, seed=63)), rnd(cout, seed=64, scale=0.1)
    xb = nhwc(rnd(nb, cout, h, w, seed=65))
    save, ss = bn_tables(xb.permute(0, 2, 3, 1).reshape(-1, cout))
    rec("conv3x3_x6p", lambda: c.conv3x3_x6p(x, pk.planes[0], cout), x=x, planes=pk.planes[0])
    rec("conv3x3_x6p flip", lambda: c.conv3x3_x6p(gy, pk.planes[1], cin, flip=True, tag="probe"), x=gy, planes=pk.planes[1])
    rec("conv3x3_x6p addend variant 0", lambda: c.conv3x3_x6p(x, pk.planes[0], cout, addend=addend, variant=0), x=x, planes=pk.planes[0], addend=addend)
    rec("conv3x3_x6p stat_shift", lambda: c.conv3x3_x6p(x, pk.planes[0], cout, stat_shift=shift), x=x, planes=pk.planes[0], stat_shift=shift)
    rec("conv3x3_x6p flip bn_bwd", lambda: c.conv3x3_x6p(gy, pk.planes[1], cin, flip=True, bn_bwd=(xb, save, ss, None, True)),
        x=gy, planes=pk.planes[1], bn_x=xb, save=save, ss=ss)
    amax, scale = x.abs().max().reshape(1), pp.scale(0)
    rec("conv3x3_x6p pair", lambda: c.conv3x3_x6p(x, pp.planes[0], cout, pair=(amax, scale)), x=x, planes=pp.planes[0], a_absmax=amax, w_scale=scale)

    xb2 = nhwc(rnd(nb, cin, 2 * h, 2 * w, seed=66))
    save2, ss2 = bn_tables(xb2.permute(0, 2, 3, 1).reshape(-1, cin))
    rec("conv3x3_s2_dgrad_x6p", lambda: c.conv3x3_s2_dgrad_x6p(gy, pk.planes[1], cin), gy=gy, planes=pk.planes[1])
    rec("conv3x3_s2_dgrad_x6p bn_bwd", lambda: c.conv3x3_s2_dgrad_x6p(gy, pk.planes[1], cin, bn_bwd=(xb2, save2, ss2, None, True)),
        gy=gy, planes=pk.planes[1], bn_x=xb2, save=save2, ss=ss2)

    for nb, cin, cout, ho, taps in ((5, 64, 128, 6, 1), (3, 64, 64, 14, 9)):
        wt = rnd(cout, taps * cin, seed=67, scale=0.05)
        pk2 = c.X6Planes([(wt, False)]).pack()
        x = nhwc(rnd(nb, cin, 2 * ho, 2 * ho, seed=68))
        shift = rnd(cout, seed=69, scale=0.1)
        rec(f"conv_s2_x6p taps {taps}", lambda: c.conv_s2_x6p(x, pk2.planes[0], cout, taps), x=x, planes=pk2.planes[0])
        rec(f"conv_s2_x6p taps {taps} stat_shift", lambda: c.conv_s2_x6p(x, pk2.planes[0], cout, taps, stat_shift=shift),
            x=x, planes=pk2.planes[0], stat_shift=shift)

    a, b = rnd(3000, 512, seed=70), rnd(3000, 128, seed=71)
    rec("gemm_x6t taps 1", lambda: c.gemm_x6t(a, b), a=a, b=b)
    a, b = rnd(5 * 10 * 10, 64, seed=72), rnd(5 * 10 * 10, 64, seed=73)
    rec("gemm_x6t taps 9", lambda: c.gemm_x6t(a, b, taps=9, hw=(10, 10), tag="probe"), a=a, b=b)
    a, b = rnd(5 * 6 * 6, 128, seed=74), rnd(5 * 12 * 12, 64, seed=75)
    rec("gemm_x6t taps 1 stride 2", lambda: c.gemm_x6t(a, b, taps=1, hw=(6, 6), stride=2), a=a, b=b)
    a, b = rnd(3 * 14 * 14, 64, seed=76), rnd(3 * 28 * 28, 64, seed=77)
    rec("gemm_x6t taps 9 stride 2", lambda: c.gemm_x6t(a, b, taps=9, hw=(14, 14), stride=2), a=a, b=b)


# ------------------------------------------------------------------ the 16-bit GEMMs and convolutions
def half(rec):
    c = _capi
    for dt, name in ((BF16, "bf16"), (F16, "fp16")):
        w0, w1 = rnd(64, 32, seed=80, scale=0.05), rnd(32, 64, seed=81, scale=0.05)
        pk = rec(f"HPlanes {name}", lambda: c.HPlanes([(w0, False), (w1, True)], dt), w0=w0, w1=w1)
        rec(f"HPlanes.pack {name}", lambda: pk.pack() and None, w0=w0, w1=w1, table=pk.table, planes0=pk.planes[0], planes1=pk.planes[1])
        assert (pk.count, pk.shapes, pk.dtype, pk.nbytes) == (2, [(64, 32), (64, 32)], dt, pk.planes[0].numel() * 2 + 4 * 2 * 64 * 32)
        planes, n = pk.planes[0], 64
        for m, s2 in ((300, None), (2 * 12 * 12, (12, 12))):
            a = rnd(m, 32, seed=82, dtype=dt)
            named = dict(a=a, planes=planes)
            addend, shift, x = rnd(m, n, seed=83, dtype=dt), rnd(n, seed=84, scale=0.1), rnd(m, n, seed=85, dtype=dt)
            save, ss = bn_tables(x)
            mask = torch.randint(-2 ** 31, 2 ** 31 - 1, (m, n // 32), dtype=torch.int32).to(DEV)
            if s2 is not None:
                compact = rnd(m // 4, n, seed=86, dtype=dt)
                rec(f"gemm_h {name} {m} addend_s2", lambda: c.gemm_h(a, planes, n, compact, addend_s2=s2), addend=compact, **named)
                continue
            rec(f"gemm_h {name} {m}", lambda: c.gemm_h(a, planes, n), **named)
            rec(f"gemm_h {name} {m} addend", lambda: c.gemm_h(a, planes, n, addend, tag="probe", tile_rows=128), addend=addend, **named)
            rec(f"gemm_h {name} {m} stat_shift", lambda: c.gemm_h(a, planes, n, stat_shift=shift), stat_shift=shift, **named)
            rec(f"gemm_h {name} {m} bn_bwd", lambda: c.gemm_h(a, planes, n, bn_bwd=(x, save, ss, None, True)), x=x, save=save, ss=ss, **named)
            rec(f"gemm_h {name} {m} bn_bwd mask", lambda: c.gemm_h(a, planes, n, addend, bn_bwd=(x, save, ss, mask, True)),
                addend=addend, x=x, save=save, ss=ss, mask=mask, **named)
            rec(f"gemm_h {name} {m} addend_mask", lambda: c.gemm_h(a, planes, n, addend, addend_mask=mask), addend=addend, addend_mask=mask, **named)

        nb, cin, cout, h, w = 2, 64, 64, 9, 7
        w4 = nhwc(rnd(cout, cin, 3, 3, seed=87, scale=0.05)).permute(0, 2, 3, 1)
        w1x1 = rnd(cout, cin, seed=88, scale=0.05)
        pk = c.HPlanes([(w4.reshape(cout, 9 * cin), False), (w4.reshape(cout * 9, cin), 9), (w1x1, False)], dt).pack()
        x, gy = nhwc(rnd(nb, cin, h, w, seed=89, dtype=dt)), nhwc(rnd(nb, cout, h, w, seed=90, dtype=dt))
        shift = rnd(cout, seed=91, scale=0.1)
        xb = nhwc(rnd(nb, cin, h, w, seed=92, dtype=dt))
        save, ss = bn_tables(xb.permute(0, 2, 3, 1).reshape(-1, cin))
        rec(f"conv_h {name}", lambda: c.conv_h(x, pk.planes[0], cout), x=x, planes=pk.planes[0])
        rec(f"conv_h {name} stat_shift", lambda: c.conv_h(x, pk.planes[0], cout, stat_shift=shift, tag="probe"), x=x, planes=pk.planes[0], stat_shift=shift)
        rec(f"conv_h {name} flip", lambda: c.conv_h(gy, pk.planes[1], cin, flip=True), x=gy, planes=pk.planes[1])
        rec(f"conv_h {name} flip bn_bwd", lambda: c.conv_h(gy, pk.planes[1], cin, flip=True, bn_bwd=(xb, save, ss, None, True)),
            x=gy, planes=pk.planes[1], bn_x=xb, save=save, ss=ss)
        x2 = nhwc(rnd(3, cin, 14, 14, seed=93, dtype=dt))
        rec(f"conv_h {name} taps 1 stride 2", lambda: c.conv_h(x2, pk.planes[2], cout, taps=1, stride=2), x=x2, planes=pk.planes[2])
        rec(f"conv_h {name} taps 9 stride 2 stat_shift", lambda: c.conv_h(x2, pk.planes[0], cout, stride=2, stat_shift=shift),
            x=x2, planes=pk.planes[0], stat_shift=shift)

        rec(f"wgrad_h {name} taps 1", lambda: c.wgrad_h(gy, x), gy=gy, x=x)
        gy2 = nhwc(rnd(3, cout, 7, 7, seed=94, dtype=dt))
        rec(f"wgrad_h {name} taps 1 stride 2", lambda: c.wgrad_h(gy2, x2, 1, 2, tag="probe"), gy=gy2, x=x2)
        x9, gy9 = nhwc(rnd(9, cin, h, w, seed=95, dtype=dt)), nhwc(rnd(9, cout, h, w, seed=96, dtype=dt))
        rec(f"wgrad_h {name} taps 9", lambda: c.wgrad_h(gy9, x9, 9, 1), gy=gy9, x=x9)
        rec(f"wgrad_h {name} taps 9 tag", lambda: c.wgrad_h(gy9, x9, 9, 1, tag="probe"), gy=gy9, x=x9)

        save2, ss2 = bn_tables(x2.permute(0, 2, 3, 1).reshape(-1, cin))
        rec(f"conv3x3_s2_dgrad_h {name}", lambda: c.conv3x3_s2_dgrad_h(gy2, pk.planes[1], cin), gy=gy2, planes=pk.planes[1])
        rec(f"conv3x3_s2_dgrad_h {name} bn_bwd", lambda: c.conv3x3_s2_dgrad_h(gy2, pk.planes[1], cin, bn_bwd=(x2, save2, ss2, None, True)),
            gy=gy2, planes=pk.planes[1], bn_x=x2, save=save2, ss=ss2)


# ------------------------------------------------------------------ the stem and the BatchNorm passes
def stem(rec):
    c = _capi
    weight = rnd(64, 3, 7, 7, seed=100, scale=0.05)
    x = nhwc(rnd(5, 3, 9, 8, seed=101))
    shift = rnd(64, seed=102, scale=0.1)
    for dt, name in ((F32, "fp32"), (BF16, "bf16")):
        pk = rec(f"StemPlanes {name}", lambda: c.StemPlanes(weight, dt), weight=weight)
        rec(f"StemPlanes.pack {name}", lambda: pk.pack() and None, weight=weight, planes=pk.planes)
        rec(f"stem_conv {name}", lambda: c.stem_conv(x, pk), x=x, planes=pk.planes)
        rec(f"stem_conv {name} stat_shift", lambda: c.stem_conv(x, pk, stat_shift=shift, tag="probe"), x=x, planes=pk.planes, stat_shift=shift)
        gy = nhwc(rnd(5, 64, 5, 4, seed=103, dtype=dt))
        rec(f"stem_wgrad {name}", lambda: c.stem_wgrad(gy, x), gy=gy, x=x)


def bn2d(rec):
    c = _capi
    n, ch, h, w = 4, 64, 8, 8
    gamma, beta = 0.5 + rnd(ch, seed=110).abs(), rnd(ch, seed=111, scale=0.2)
    rm, rv, nbt = rnd(ch, seed=112, scale=0.1), 1.0 + rnd(ch, seed=113, scale=0.1).abs(), torch.zeros((), dtype=torch.int64, device=DEV)
    stats = dict(gamma=gamma, beta=beta, running_mean=rm, running_var=rv, nbt=nbt)
    w64 = rnd(ch, ch, seed=114, scale=0.05)
    for dt, name in ((F32, "fp32"), (BF16, "bf16")):
        x, res, dy = nhwc(rnd(n, ch, h, w, seed=115, dtype=dt)), nhwc(rnd(n, ch, h, w, seed=116, dtype=dt)), nhwc(rnd(n, ch, h, w, seed=117, dtype=dt))
        fwd = lambda residual, relu, training=True, **kw: c.bn2d_fwd(x, residual, gamma, beta, rm, rv, nbt, training, 1e-5, 0.1, relu, **kw)
        for relu in (False, True):
            for residual in (None, res):
                tag = f"{name} relu={relu} residual={residual is not None}"
                y, save, ss, mask = rec(f"bn2d_fwd {tag}", lambda: fwd(residual, relu), x=x, residual=residual, **stats)
                rec(f"bn2d_bwd {tag}", lambda: c.bn2d_bwd(dy, x, y, None, save, ss, True, relu, residual is not None), dy=dy, x=x, y=y, save=save, ss=ss)
        y, save, ss, mask = rec(f"bn2d_fwd {name} want_mask", lambda: fwd(res, True, want_mask=True), x=x, residual=res, **stats)
        rec(f"bn2d_bwd {name} mask", lambda: c.bn2d_bwd(dy, x, y, mask, save, ss, True, True, True), dy=dy, x=x, y=y, mask=mask, save=save, ss=ss)
        rec(f"bn2d_bwd {name} recomputed ReLU", lambda: c.bn2d_bwd(dy, x, None, None, save, ss, True, True, False), dy=dy, x=x, save=save, ss=ss)
        rec(f"bn2d_fwd {name} eval", lambda: fwd(None, True, training=False), x=x, **stats)
        rec(f"bn2d_bwd {name} eval", lambda: c.bn2d_bwd(dy, x, y, None, save, ss, False, True, False), dy=dy, x=x, y=y, save=save, ss=ss)
        xs = nhwc(rnd(n, ch, h, w, seed=118, dtype=dt))
        _, _, ss_s, _ = rec(f"bn2d_fwd {name} apply=False", lambda: c.bn2d_fwd(xs, None, gamma, beta, rm, rv, nbt, True, 1e-5, 0.1, False, apply=False), x=xs, **stats)
        rec(f"bn2d_apply {name}", lambda: c.bn2d_apply(xs, ss_s, relu=False), x=xs, ss=ss_s)
        rec(f"bn2d_fwd {name} residual_bn", lambda: fwd(None, True, want_mask=True, residual_bn=(xs, ss_s)), x=x, shortcut_x=xs, shortcut_ss=ss_s, **stats)
        # statistics and the backward reduction handed over by the GEMM that produced x / dy
        a = rnd(n * h * w, ch, seed=119, dtype=dt)
        shift = rm.clone()
        if dt == F32:
            planes = c.X6Planes([(w64, False)]).pack().planes[0]
            xg, partial, ns = c.gemm_x6p(a, planes, ch, stat_shift=shift)
        else:
            planes = c.HPlanes([(w64, False)], dt).pack().planes[0]
            xg, partial, ns = c.gemm_h(a, planes, ch, stat_shift=shift)
        x_pre = xg.view(n, h, w, ch).permute(0, 3, 1, 2)
        y, save, ss, mask = rec(f"bn2d_fwd {name} pre", lambda: fwd_on(c, x_pre, stats, pre=(partial, ns, shift)), x=x_pre, partial=partial, shift=shift, **stats)
        bwd = (x_pre, save, ss, None, True)
        dyg, bpartial, bns = c.gemm_x6p(a, planes, ch, bn_bwd=bwd) if dt == F32 else c.gemm_h(a, planes, ch, bn_bwd=bwd)
        dy_pre = dyg.view(n, h, w, ch).permute(0, 3, 1, 2)
        rec(f"bn2d_bwd {name} pre", lambda: c.bn2d_bwd(dy_pre, x_pre, None, None, save, ss, True, True, False, pre=(bpartial, bns)),
            dy=dy_pre, x=x_pre, save=save, ss=ss, partial=bpartial)
        if dt == F32:
            slot = rec("absmax_slot", lambda: c.absmax_slot(x.device))
            y, save, ss, _ = rec("bn2d_fwd fp32 absmax", lambda: fwd(None, True, absmax=slot), x=x, absmax=slot, **stats)
            rec("bn2d_apply fp32 absmax", lambda: c.bn2d_apply(x, ss, absmax=slot), x=x, ss=ss, absmax=slot)
            rec("bn2d_bwd fp32 absmax", lambda: c.bn2d_bwd(dy, x, y, None, save, ss, True, True, True, absmax=slot), dy=dy, x=x, y=y, save=save, ss=ss, absmax=slot)

        xa, ra = nhwc(rnd(5, ch, 3, 3, seed=120, dtype=dt)), nhwc(rnd(5, ch, 3, 3, seed=121, dtype=dt))
        for training in (True, False):
            pooled, mask, save, ss = rec(f"bn2d_avgpool_fwd {name} training={training}",
                                         lambda: c.bn2d_avgpool_fwd(xa, ra, gamma, beta, rm, rv, nbt, training, 1e-5, 0.1), x=xa, residual=ra, **stats)
            dp = rnd(5, ch, seed=122)
            rec(f"bn2d_avgpool_bwd {name} training={training}", lambda: c.bn2d_avgpool_bwd(dp, xa, mask, save, ss, training),
                d_pooled=dp, x=xa, mask=mask, save=save, ss=ss)
        for shape in ((3, ch, 15, 17), (1, ch, 1, 5)):
            xp = nhwc(rnd(*shape, seed=123, dtype=dt))
            for training in (True, False):
                tag = f"{name} {shape[2]}x{shape[3]} training={training}"
                y, x_at_max, code, save, ss = rec(f"bn2d_pool_fwd {tag}", lambda: c.bn2d_pool_fwd(xp, gamma, beta, rm, rv, nbt, training, 1e-5, 0.1), x=xp, **stats)
                dyp = nhwc(torch.randn_like(y.float()).to(dt))
                rec(f"bn2d_pool_bwd {tag}", lambda: c.bn2d_pool_bwd(dyp, xp, x_at_max, code, save, ss, training),
                    dy=dyp, x=xp, x_at_max=x_at_max, code=code, save=save, ss=ss)


def fwd_on(c, x, stats, **kw):
    return c.bn2d_fwd(x, None, stats["gamma"], stats["beta"], stats["running_mean"], stats["running_var"], stats["nbt"], True, 1e-5, 0.1, True, **kw)


# ------------------------------------------------------------------ the augmenter
def augment(rec):
    from peclr_amd.augment import (EXT_BLUR, EXT_COLOR_DROP, EXT_INTS, EXT_NOISE, EXT_SOBEL, IMAGENET_MEAN, IMAGENET_STD, RaggedImages,
                                   TwoViewAugmenter, noise_cdf_table)

    c = _capi
    g = torch.Generator().manual_seed(130)
    jit = (0.73, 0.44, 0.9, 13.0)
    record = lambda win: [1.0, 0, 0, 0, 1.0, 0, 0.0, *map(float, win), 1.0, *jit]          # no rotation; crop window; colour jitter
    table = torch.from_numpy(np.array(noise_cdf_table(25.0), dtype=np.uint32).view(np.int32).copy()).to(DEV)
    coefs = torch.tensor([256, 256], dtype=torch.int32, device=DEV)                          # blur lengths (1, 1): images under 20 pixels

    def ext_for(flags):
        ext = torch.zeros((2, 2, EXT_INTS), dtype=torch.int32)
        ext[..., 0], ext[..., 6] = flags, (0 if flags & EXT_BLUR else -1)
        return ext.to(DEV)

    modes = (("ops 0", 0), ("pre", EXT_SOBEL), ("pre blur", EXT_SOBEL | EXT_BLUR), ("post", EXT_NOISE | EXT_COLOR_DROP))

    # uniform: two 9 x 8 images, windows (x0, y0, cw, ch) inside them
    images = torch.randint(0, 256, (2, 9, 8, 3), generator=g, dtype=torch.uint8).to(DEV)
    wins = [[(1, 1, 6, 7), (0, 2, 8, 5)], [(2, 0, 5, 9), (0, 0, 8, 9)]]
    params = torch.tensor([[record(wn) for wn in vs] for vs in wins], dtype=torch.float64).to(DEV)
    for nhwc_out in (True, False):
        rec(f"augment_views channels_last={nhwc_out}", lambda: c.augment_views(images, params, (16, 16), IMAGENET_MEAN, IMAGENET_STD, nhwc_out),
            images=images, params=params)
    for name, ops in modes:
        ext = ext_for(ops)
        rec(f"augment_views_ext {name}", lambda: c.augment_views_ext(images, params, ext, coefs, (1, 1), table, table.numel(), 4242, 3, ops, (16, 16),
                                                                     IMAGENET_MEAN, IMAGENET_STD),
            images=images, params=params, ext=ext, coefs=coefs, noise_table=table)

    # ragged: a 9 x 8 and a 5 x 12 image
    sizes = [(9, 8), (5, 12)]
    ragged = RaggedImages.from_list([torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes], DEV)
    wins = [[(1, 1, 6, 7), (2, 0, 9, 5)], [(2, 0, 5, 9), (0, 1, 12, 3)]]
    views = [[{"crop": wn} for wn in vs] for vs in wins]
    params = torch.tensor([[record(wn) for wn in vs] for vs in wins], dtype=torch.float64).to(DEV)
    geom, tab = TwoViewAugmenter.ragged_tables(sizes, ragged.offsets, views)
    for nhwc_out in (True, False):
        rec(f"augment_views_ragged channels_last={nhwc_out}",
            lambda: c.augment_views_ragged(ragged.data, geom, tab, params, (16, 16), IMAGENET_MEAN, IMAGENET_STD, nhwc_out), packed=ragged.data, params=params)
    for name, ops in modes:
        ext = ext_for(ops)
        rec(f"augment_views_ragged_ext {name}",
            lambda: c.augment_views_ragged_ext(ragged.data, geom, tab, params, ext, coefs, table, table.numel(), 4242, 3, ops, (16, 16), IMAGENET_MEAN,
                                               IMAGENET_STD),
            packed=ragged.data, params=params, ext=ext, coefs=coefs, noise_table=table)


# ------------------------------------------------------------------ the pose model's crop and head, and the scores
def pose(rec):
    c = _capi
    g = torch.Generator().manual_seed(140)
    b = 2
    images = torch.randint(0, 256, (b, 9, 8, 3), generator=g, dtype=torch.uint8).to(DEV)
    T = torch.tensor([[1.5, 0.1, 0.5], [-0.1, 1.5, 1.0], [0.0, 0.0, 1.0]], dtype=torch.float64).repeat(b, 1, 1).to(DEV)
    K64 = torch.tensor([[500.0, 0.0, 112.0], [0.0, 500.0, 112.0], [0.0, 0.0, 1.0]], dtype=torch.float64).repeat(b, 1, 1).to(DEV)
    table = rnd(3, 256, seed=141)
    rec("pose_crop", lambda: c.pose_crop(images, T, K64, table, 16), images=images, T=T, K=K64, table=table)
    rec("pose_crop no K", lambda: c.pose_crop(images, T, None, table, 16), images=images, T=T, table=table)

    feat, fc_w, fc_b = rnd(b, 2048, seed=142), rnd(64, 2048, seed=143, scale=0.02), rnd(64, seed=144, scale=0.1)
    shapes = [(128, 64), (128,), (128,), (128,), (128,), (128,), (128, 128), (128,), (128,), (128,), (128,), (128,), (1, 128), (1,)]
    mlp = [rnd(*s, seed=145 + i, scale=0.1) for i, s in enumerate(shapes)]
    for i in (5, 11):
        mlp[i] = 1.0 + mlp[i].abs()                     # running variances
    K = K64.float().contiguous()
    T1 = T.clone()
    named = dict(feat=feat, fc_w=fc_w, fc_b=fc_b, K=K)
    _, _, _, _, status = rec("pose_head pass 1", lambda: c.pose_head(feat, fc_w, fc_b, mlp, (1e-5, 1e-5), K, 1e-6, T1=T1, size=224), T1=T1, **named)
    scale = torch.ones(b, dtype=torch.float64, device=DEV)
    rec("pose_head pass 2", lambda: c.pose_head(feat, fc_w, fc_b, mlp, (1e-5, 1e-5), K, 1e-6, scale=scale, status=status), scale=scale, status=status, **named)
    rec("pose_head one K", lambda: c.pose_head(feat, fc_w, fc_b, mlp, (1e-5, 1e-5), K[:1].contiguous(), 1e-6), feat=feat, fc_w=fc_w, fc_b=fc_b)

    b = 4
    for dt, name in ((F32, "fp32"), (torch.float64, "fp64")):
        pred, gt = rnd(b, 21, 3, seed=150).to(dt), rnd(b, 21, 3, seed=151).to(dt)
        thr = torch.linspace(0.0, 3.0, 5, dtype=dt, device=DEV)
        counts = torch.zeros((2, 21, 5), dtype=torch.int64, device=DEV)
        rec(f"pose_eval {name}", lambda: c.pose_eval(pred, gt), pred=pred, gt=gt)
        rec(f"pose_eval {name} no transform", lambda: c.pose_eval(pred, gt, want_transform=False), pred=pred, gt=gt)
        rec(f"pose_eval {name} no Procrustes", lambda: c.pose_eval(pred, gt, dim=2, procrustes=False), pred=pred, gt=gt)
        rec(f"pose_eval {name} thresholds", lambda: c.pose_eval(pred, gt, thr=thr, counts=counts), pred=pred, gt=gt, thr=thr, counts=counts)
        cursor = torch.zeros(2, dtype=torch.int32, device=DEV)
        dist, dist_al = torch.empty((8, 21), dtype=dt, device=DEV), torch.empty((8, 21), dtype=dt, device=DEV)
        status = torch.zeros(8, dtype=torch.int32, device=DEV)
        rec(f"pose_eval {name} streaming",
            lambda: c.pose_eval(pred, gt, thr=thr, counts=counts, status=status, dist=dist, dist_aligned=dist_al, cursor=cursor, want_transform=False),
            pred=pred, gt=gt, thr=thr, counts=counts, status=status, dist=dist, dist_aligned=dist_al, cursor=cursor)
        rec(f"pose_eval {name} streaming 2-D", lambda: c.pose_eval(pred, gt, dim=2, procrustes=False, status=status, dist=dist, cursor=cursor),
            pred=pred, gt=gt, status=status, dist=dist, cursor=cursor)


GROUPS = (head, x6, half, stem, bn2d, augment, pose)


def record(label="working tree"):
    """Run every group; returns {"recorded_from": label, "cases": [...]}.  The module's state is put back afterwards."""
    saved = (_capi._LIB, _capi.EVENT_LOG, _capi.LAUNCH_ORDER, _capi.TAG_BOUND_SUFFIX)
    rec = Recorder()
    _capi._LIB = _Proxy(_capi.lib(), rec.calls)
    _capi.TAG_BOUND_SUFFIX = True
    torch.manual_seed(0)
    try:
        for group in GROUPS:
            try:
                group(rec)
            except (TypeError, ValueError, AttributeError, IndexError, KeyError, AssertionError) as e:   # a mistake in this file
                rec.errors.append(f"{group.__name__} stopped: {type(e).__name__}: {e}")
        torch.cuda.synchronize()
    finally:
        _capi._LIB, _capi.EVENT_LOG, _capi.LAUNCH_ORDER, _capi.TAG_BOUND_SUFFIX = saved
    return {"recorded_from": label, "cases": rec.cases, "errors": rec.errors}


if __name__ == "__main__":
    log = record(*sys.argv[2:3])
    with open(sys.argv[1], "w") as f:
        json.dump(log, f, indent=0, separators=(",", ":"))
        f.write("\n")
    for line in log["errors"]:
        print("ERROR", line)
    print(f"{len(log['cases'])} wrapper calls, {sum(len(k['native']) for k in log['cases'])} native calls -> {sys.argv[1]}")
    sys.exit(2 if log["errors"] else 0)
