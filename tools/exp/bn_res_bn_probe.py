"""Kernel timings (HIP events, median of 10 after 3 warm-ups, random data) at the four downsample-block shapes of the 2 x 128 @224
step, fp32 and bf16: the pair of apply launches (peclr_bn2d_bwd_apply with d_residual, then without a mask on that tensor) + the
MASK 0 reduce, against the dual apply (peclr_bn2d_bwd_apply_res_bn) + the MASK 3 reduce.  Run from the repository root:
python tools/exp/bn_res_bn_probe.py  (profiles/r07_shortcut_bwd_kernel_probe.txt)."""
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
from peclr_amd import _capi as capi

DEV = "cuda:0"
L = capi.lib()
s = capi._stream()


def timeit(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


for dtype, io, e in ((torch.float32, 0, 4), (torch.bfloat16, 1, 2)):
    for r, c in ((256 * 56 * 56, 256), (256 * 28 * 28, 512), (256 * 14 * 14, 1024), (256 * 7 * 7, 2048)):
        g = torch.Generator().manual_seed(c)
        mk = lambda: torch.randn(r, c, device=DEV, dtype=dtype)
        dy, x3, xs = mk(), mk(), mk()
        mask = torch.randint(-2 ** 31, 2 ** 31, (r, c // 32), device=DEV, dtype=torch.int64).to(torch.int32)
        dx, dxs, dres = torch.empty_like(dy), torch.empty_like(dy), torch.empty_like(dy)
        tab = lambda: (torch.randn(2, c, device=DEV).abs() + 0.5)
        save, ss, coef, save_s, ss_s, coef_s = tab(), tab(), tab(), tab(), tab(), tab()
        a1, a2 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        am = (lambda t: t.data_ptr()) if io == 0 else (lambda t: None)
        ns = capi.bn2d_n_split(r, c, io)
        part = torch.empty(2 * ns, c, device=DEV)
        old1 = lambda: L.peclr_bn2d_bwd_apply(dy.data_ptr(), x3.data_ptr(), None, mask.data_ptr(), io, r, c, 1, save[0].data_ptr(), save[1].data_ptr(),
                                              ss.data_ptr(), coef.data_ptr(), dx.data_ptr(), dres.data_ptr(), am(a1), s)
        old2 = lambda: L.peclr_bn2d_bwd_apply(dres.data_ptr(), xs.data_ptr(), None, None, io, r, c, 0, save_s[0].data_ptr(), save_s[1].data_ptr(),
                                              ss_s.data_ptr(), coef_s.data_ptr(), dxs.data_ptr(), None, am(a2), s)
        new = lambda: L.peclr_bn2d_bwd_apply_res_bn(dy.data_ptr(), mask.data_ptr(), x3.data_ptr(), xs.data_ptr(), io, r, c, save[0].data_ptr(),
                                                    save[1].data_ptr(), ss.data_ptr(), coef.data_ptr(), save_s[0].data_ptr(), save_s[1].data_ptr(),
                                                    ss_s.data_ptr(), coef_s.data_ptr(), dx.data_ptr(), dxs.data_ptr(), am(a1), am(a2), s)
        red0 = lambda: L.peclr_bn2d_bwd_reduce(dres.data_ptr(), xs.data_ptr(), None, None, io, r, c, 0, save_s[0].data_ptr(), save_s[1].data_ptr(),
                                               ss_s.data_ptr(), part.data_ptr(), ns, s)
        red3 = lambda: L.peclr_bn2d_bwd_reduce(dy.data_ptr(), xs.data_ptr(), None, mask.data_ptr(), io, r, c, 1, save_s[0].data_ptr(), save_s[1].data_ptr(),
                                               ss_s.data_ptr(), part.data_ptr(), ns, s)
        assert old1() == 0 and old2() == 0 and new() == 0 and red0() == 0 and red3() == 0
        t1, t2, tn, r0, r3 = timeit(old1), timeit(old2), timeit(new), timeit(red0), timeit(red3)
        nb = 5 * e * r * c + r * c // 8
        print(f"{str(dtype)[6:]:9s} R={r:7d} C={c:5d}  apply DRES {t1[0]:7.1f} us + apply MASK0 {t2[0]:7.1f} us = {t1[0] + t2[0]:7.1f} | dual {tn[0]:7.1f} us "
              f"(min {tn[1]:.1f} max {tn[2]:.1f}; {nb / tn[0] / 1e6:.2f} TB/s) | reduce MASK0 {r0[0]:6.1f} us, MASK3 {r3[0]:6.1f} us", flush=True)
        del dy, x3, xs, mask, dx, dxs, dres
        torch.cuda.empty_cache()
