"""Two-pass FreiHAND prediction throughput (peclr_amd.pose.FreiHANDPredictor) on synthetic images, eager vs hipGraph,
timed with device events; and, with --kernels, the share of the crop and head launches in one predict's GPU time.

    python tools/pose_timing.py [--backends rn50 rn152] [--batches 1 32 128] [--iters 10] [--precision bf16 --fold 1]
    python tools/pose_timing.py --backends rn50 --arms fp32 bf16:0 bf16:1 fp16:1 --windows 5     # same-run A/B, alternated
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/pose_timing.py --backends rn50 --batches 128 --iters 3 --no-graph

The per-launch numbers of the crop and head kernels come from the rocprofv3 run (its kernel_stats table: pose_crop_kernel,
pose_head_kernel, and the total of every kernel of the run).

An arm is `precision[:fold]` (fold: the eval-mode BatchNorm layers in the convolution epilogues, 16-bit only).  With several
arms or --windows > 1 every (arm, eager | graph) is timed in `windows` windows of `iters` calls, the arms taking turns inside a
window (drift of the device hits all of them alike), and the row gives the median window: whole-predict device time.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters):
    import torch

    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--backends", nargs="+", default=["rn50", "rn152"])
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 32, 128])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--precision", choices=("fp32", "bf16", "fp16"), default="fp32")
    ap.add_argument("--fold", type=int, choices=(0, 1), default=None, help="16-bit: BatchNorm folded into the epilogues (default: the predictor's)")
    ap.add_argument("--arms", nargs="+", default=None, help="precision[:fold] ..., timed alternately (overrides --precision / --fold)")
    ap.add_argument("--windows", type=int, default=1)
    args = ap.parse_args(argv)
    arms = []
    for a in args.arms or [args.precision + ("" if args.fold is None else f":{args.fold}")]:
        p, _, f = a.partition(":")
        arms.append((a, p, None if f == "" else bool(int(f))))

    import torch

    from peclr_amd.pose import K_DEFAULT, FreiHANDPredictor, RN25DwMLPref

    rows = []
    for backend in args.backends:
        torch.manual_seed(0)
        model = RN25DwMLPref(backend).eval().to("cuda").enable_hip()
        with torch.no_grad():   # keypoints spread over the crop, so that the re-crop is a real crop
            model.backend_model.fc.weight.mul_(0.05)
            model.backend_model.fc.bias.copy_(torch.tensor([112.0, 112.0, 0.0] * 21 + [0.0]))
            for blk in model.backend_model.modules():   # damped residual branches: 50 random blocks of RN-152 stay finite
                if hasattr(blk, "bn3"):
                    blk.bn3.weight.fill_(0.2)
        preds = {name: FreiHANDPredictor(model, precision=p, fold_bn=f) for name, p, f in arms}
        for b in args.batches:
            rng = np.random.default_rng(b)
            imgs = torch.from_numpy(rng.integers(0, 256, (b, 224, 224, 3), dtype=np.uint8)).cuda()
            K = torch.tensor(K_DEFAULT, dtype=torch.float64).expand(b, 3, 3).contiguous().cuda()
            scale = torch.full((b,), 0.03, dtype=torch.float64).cuda()
            # two phases, as the single-arm form of this tool always ran: every eager window first, then the captures and the
            # replay windows (no eager predict between a predictor's capture and its replays)
            eager = {(name, "eager"): (lambda pred=pred: pred.predict(imgs, K, scale)) for name, pred in preds.items()}
            times = {k: [] for k in eager}
            for _ in range(args.windows):
                for k, fn in eager.items():
                    times[k].append(_time(fn, args.iters))
            if not args.no_graph:
                graph = {}
                for name, pred in preds.items():
                    pred.capture(b)
                    graph[(name, "graph")] = lambda pred=pred: pred.replay(imgs, K, scale)
                times.update({k: [] for k in graph})
                for _ in range(args.windows):
                    for k, fn in graph.items():
                        times[k].append(_time(fn, args.iters))
            for name, pred in preds.items():
                row = {"backend": backend, "batch": b}
                if args.arms or args.precision != "fp32":
                    row.update(arm=name, fold_bn=pred.fold_bn)
                if args.windows > 1:
                    row["windows"] = args.windows
                for mode in ("eager", "graph"):
                    if (name, mode) in times:
                        ms = float(np.median(times[(name, mode)]))
                        row.update({f"{mode}_ms": round(ms, 3), f"{mode}_img_s": round(b / ms * 1e3, 1)})
                rows.append(row)
                print(json.dumps(row), flush=True)
        del preds, model
        torch.cuda.empty_cache()
    return rows


if __name__ == "__main__":
    main()
