"""Time of the 16-bit 3x3 / stride-2 weight gradient (the convolutions that open layers 2 - 4), the two routes `bn2d._wgrad_h`
chooses between with `ROUTING.wgrad16_s2`: in-tree (`_capi.wgrad3_s2_h`: wgrad3_h_s2_kernel + the fixed-order slab reduction, fp32
out) against MIOpen (`bn2d._conv_wgrad`: the 16-bit weight gradient + its cast to fp32), same process, same operands.  Warm; a
window is ITERS back-to-back calls between two device events; the two routes alternate window by window, one window of each is
thrown away; median, minimum and maximum over the windows.  The field defaults on only if, in both formats, the in-tree medians
summed over the three shapes of config C2 are not above MIOpen's sum -- and the bf16 step is not slower with it
(profiles/wgrad3_s2_timing.txt and profiles/wgrad3_s2_step_ab.txt keep the runs that decided it).

    python tools/wgrad3_s2_timing.py [--iters 200] [--windows 9] [--shapes 256x128x128x28x28,...]
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

# (images, Cout, Cin, Ho, Wo) of ResNet-50's layer2.0 / layer3.0 / layer4.0 conv2: config C2 (2 x 128 views @224), then C5 (2 x 64 views @448)
C2 = "256x128x128x28x28,256x256x256x14x14,256x512x512x7x7"
C5 = "128x128x128x56x56,128x256x256x28x28,128x512x512x14x14"


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
    ap.add_argument("--shapes", default=C2 + "," + C5)
    args = ap.parse_args(argv)
    if args.windows < 7:
        ap.error("at least 7 windows")

    import torch

    from peclr_amd import _capi
    from peclr_amd import bn2d as B

    assert torch.cuda.is_available(), "a timing needs the GPU"
    ours_name, theirs_name = "in-tree (wgrad3_h_s2_kernel + slab reduce)", "MIOpen (16-bit weight gradient + cast to fp32)"
    rows, sums = [], {}
    for shape in args.shapes.split(","):
        nb, cout, cin, ho, wo = (int(v) for v in shape.split("x"))
        for dtype in (torch.bfloat16, torch.float16):
            g = torch.Generator(device="cuda").manual_seed(nb + ho + wo)
            x = torch.randn(nb, cin, 2 * ho, 2 * wo, device="cuda", generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
            gy = torch.randn(nb, cout, ho, wo, device="cuda", generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
            weight = torch.zeros(cout, cin, 3, 3, device="cuda").contiguous(memory_format=torch.channels_last)
            assert _capi.wgrad3_s2_h_ok(gy, x), shape
            fns = {ours_name: lambda: _capi.wgrad3_s2_h(gy, x),
                   theirs_name: lambda: B._conv_wgrad(gy, x, weight, (2, 2), (1, 1), weight)}
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
            fmt = str(dtype).split(".")[1]
            base = {"shape": shape, "dtype": fmt, "iters": args.iters, "windows": args.windows,
                    "slabs": _capi.lib().peclr_wgrad3s2_h_slabs(cout, cin, nb, ho, wo), "rel_diff_between_the_two": round(rel, 6)}
            med = {}
            for name in fns:
                med[name] = statistics.median(samples[name])
                rows.append(dict(base, what=name, median_us=round(med[name], 1), min_us=round(min(samples[name]), 1),
                                 max_us=round(max(samples[name]), 1)))
                print(json.dumps(rows[-1]), flush=True)
                if shape in C2.split(","):
                    sums[(fmt, name)] = sums.get((fmt, name), 0.0) + med[name]
            print(json.dumps(dict(base, what="in-tree / MIOpen, medians", ratio=round(med[ours_name] / med[theirs_name], 3))), flush=True)
    verdict = bool(sums)
    for fmt in sorted({f for f, _ in sums}):
        a, b = sums[(fmt, ours_name)], sums[(fmt, theirs_name)]
        verdict = verdict and a <= b
        print(json.dumps({"what": "sum of the medians over the C2 shapes of this run", "dtype": fmt, "in_tree_us": round(a, 1),
                          "miopen_us": round(b, 1), "ratio": round(a / b, 3)}), flush=True)
    print(json.dumps({"what": "in-tree sum over the C2 shapes not above MIOpen's in both formats", "holds": verdict}), flush=True)
    return rows


if __name__ == "__main__":
    main()
