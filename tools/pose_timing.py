"""Two-pass FreiHAND prediction throughput (peclr_amd.pose.FreiHANDPredictor) on synthetic images, eager vs hipGraph,
timed with device events; and, with --kernels, the share of the crop and head launches in one predict's GPU time.

    python tools/pose_timing.py [--backends rn50 rn152] [--batches 1 32 128] [--iters 10]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/pose_timing.py --backends rn50 --batches 128 --iters 3 --no-graph

The per-launch numbers of the crop and head kernels come from the rocprofv3 run (its kernel_stats table: pose_crop_kernel,
pose_head_kernel, and the total of every kernel of the run).
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
    args = ap.parse_args(argv)

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
        pred = FreiHANDPredictor(model)
        for b in args.batches:
            rng = np.random.default_rng(b)
            imgs = torch.from_numpy(rng.integers(0, 256, (b, 224, 224, 3), dtype=np.uint8)).cuda()
            K = torch.tensor(K_DEFAULT, dtype=torch.float64).expand(b, 3, 3).contiguous().cuda()
            scale = torch.full((b,), 0.03, dtype=torch.float64).cuda()
            eager = _time(lambda: pred.predict(imgs, K, scale), args.iters)
            row = {"backend": backend, "batch": b, "eager_ms": round(eager, 3), "eager_img_s": round(b / eager * 1e3, 1)}
            if not args.no_graph:
                pred.capture(b)
                graph = _time(lambda: pred.replay(imgs, K, scale), args.iters)
                row.update(graph_ms=round(graph, 3), graph_img_s=round(b / graph * 1e3, 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del pred, model
        torch.cuda.empty_cache()
    return rows


if __name__ == "__main__":
    main()
