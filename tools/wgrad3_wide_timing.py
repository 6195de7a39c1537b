"""Time of the 16-bit 3x3 / stride-1 weight gradient of rows wider than 62 pixels, the two routes `bn2d._wgrad_h` chooses between
with `ROUTING.wgrad16_wide`: in-tree (`_capi.wgrad_h`: wgrad3_h_kernel over column segments + the fixed-order slab reduction, fp32 out) against
MIOpen (`bn2d._conv_wgrad`: the 16-bit weight gradient + its cast to fp32), same process, same operands.  Warm; a window is ITERS
back-to-back calls between two device events; the two routes alternate window by window, one window of each is thrown away;
median, minimum and maximum over the windows.  The field defaults on only if the in-tree median is not above MIOpen's at every
shape and in both formats (profiles/wgrad3_wide_timing.txt keeps the run that decided it).

    python tools/wgrad3_wide_timing.py [--iters 200] [--windows 9] [--shapes 128x64x64x112x112,128x64x64x64x64]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIOPEN_USER_DB_PATH", os.path.join(ROOT, ".miopen", "db"))
os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", os.path.join(ROOT, ".miopen", "cache"))

SHAPES = "128x64x64x112x112,128x64x64x64x64"       # (images, Cout, Cin, H, W): layer1 of config C5 (2 x 64 views @448) and of a 256 x 256 input


def _window(fn, iters):
    """`iters` back-to-back calls -> microseconds per call by device events."""
    import torch

    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--shapes", default=SHAPES)
    args = ap.parse_args(argv)
    if args.windows < 7:
        ap.error("at least 7 windows")

    import torch

    from peclr_amd import _capi
    from peclr_amd import bn2d as B

    assert torch.cuda.is_available(), "a timing needs the GPU"
    rows, verdict = [], True
    for shape in args.shapes.split(","):
        nb, cout, cin, h, w = (int(v) for v in shape.split("x"))
        for dtype in (torch.bfloat16, torch.float16):
            g = torch.Generator(device="cuda").manual_seed(nb + h + w)
            x = torch.randn(nb, cin, h, w, device="cuda", generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
            gy = torch.randn(nb, cout, h, w, device="cuda", generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
            weight = torch.zeros(cout, cin, 3, 3, device="cuda").contiguous(memory_format=torch.channels_last)
            assert _capi.wgrad_h_ok(gy, x, 9, 1) and w > _capi.WGRAD3_MAX_W, shape
            fns = {"in-tree (wgrad3_h_kernel, segments + slab reduce)": lambda: _capi.wgrad_h(gy, x, 9, 1),
                   "MIOpen (16-bit weight gradient + cast to fp32)": lambda: B._conv_wgrad(gy, x, weight, (1, 1), (1, 1), weight)}
            ours, theirs = (fn() for fn in fns.values())
            ours = ours.view(cout, 3, 3, cin).permute(0, 3, 1, 2)
            rel = float((ours.double() - theirs.double()).norm() / theirs.double().norm())
            for fn in fns.values():                      # warm: code objects, MIOpen's choice of algorithm, the allocator
                _window(fn, 3)
            samples = {name: [] for name in fns}
            for win in range(args.windows + 1):
                for name, fn in fns.items():
                    t = _window(fn, args.iters)
                    if win:
                        samples[name].append(t)
            base = {"shape": shape, "dtype": str(dtype).split(".")[1], "iters": args.iters, "windows": args.windows,
                    "slabs": _capi.lib().peclr_wgrad3w_h_slabs(cout, cin, nb, h, w), "rel_diff_between_the_two": round(rel, 6)}
            med = {}
            for name in fns:
                med[name] = statistics.median(samples[name])
                rows.append(dict(base, what=name, median_us=round(med[name], 1), min_us=round(min(samples[name]), 1),
                                 max_us=round(max(samples[name]), 1)))
                print(json.dumps(rows[-1]), flush=True)
            a, b = (med[name] for name in fns)
            verdict = verdict and a <= b
            print(json.dumps(dict(base, what="in-tree / MIOpen, medians", ratio=round(a / b, 3))), flush=True)
    print(json.dumps({"what": "in-tree median not above MIOpen's at every shape and format", "holds": verdict}), flush=True)
    return rows


if __name__ == "__main__":
    main()
