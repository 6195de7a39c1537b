"""Time of one supervised fine-tuning step of the 2.5D pose model (ResNet-50, B = 128, 224 x 224, fp32): forward, the four
losses, the step metrics, backward and the fused Adam step -- `SupervisedPose` on the HIP kernels, issued eagerly and replayed
from the one hipGraph `Trainer.capture_step_graph` records, against the stock-torch step of the same model (tools/
stock_pose_step.py: no `enable_hip*`, same optimiser) in the same run on the same machine.  And the step-metrics launch
(`peclr_pose_step_metrics_f32`, both pairs) against the torch composition of calculate_metrics for two pairs.

Warm; a run is ITERS back-to-back steps timed by device events and, around the same steps, by the wall clock with the device
waited for; the arms alternate run by run; median, minimum and maximum over the runs.  What the figures are: for the whole
step the device is busy for tens of milliseconds per step, so every figure is DEVICE TIME (eager and replayed differ by what
the host cannot issue fast enough).  For the metrics the eager figures are LAUNCH-ISSUE RATES -- the device finishes each launch
before the host has issued the next -- and only the figures from a hipGraph (each composition captured once) are device time.

    python tools/pose_finetune_timing.py [--batch 128] [--size 224] [--iters 10] [--runs 5]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time_once(fn, iters):
    """`iters` back-to-back calls -> (microseconds per call by device events, by the wall clock with the device waited for)."""
    import torch

    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3, (time.perf_counter() - t0) / iters * 1e6


def _report(title, fns, iters, runs, base):
    """The arms alternate within every run, so that whatever else the machine does meets all of them; one run of each is thrown away."""
    samples = {name: [] for name in fns}
    for run in range(runs + 1):
        for name, fn in fns.items():
            t = _time_once(fn, iters)
            if run:
                samples[name].append(t)
    for name in fns:
        for i, clock in enumerate(("device events", "wall clock")):
            us = [t[i] for t in samples[name]]
            print(json.dumps(dict(base, what=f"{title}: {name}, {clock}", iters=iters, runs=runs, median_us=round(statistics.median(us), 1),
                                  min_us=round(min(us), 1), max_us=round(max(us), 1))), flush=True)
    return {name: statistics.median(t[0] for t in samples[name]) for name in fns}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from peclr_amd import SupervisedAugmenter, SupervisedPose, Trainer, step_metrics, supervised_config
    from stock_pose_step import StockPose, metrics as torch_metrics

    b, size, dev = args.batch, args.size, "cuda"
    g = np.random.default_rng(0)
    focal = 480.0 * size / 224
    k = np.repeat(np.array([[focal, 0, size / 2], [0, focal, size / 2], [0, 0, 1]], dtype=np.float32)[None], b, 0)
    z = 0.6 + 0.05 * g.standard_normal((b, 21))
    uv = g.uniform(0.35, 0.65, (b, 1, 2)) * size + size / 9 * g.standard_normal((b, 21, 2))
    j3d = np.concatenate([(uv - size / 2) * z[..., None] / focal, z[..., None]], axis=2).astype(np.float32)
    images = torch.randint(0, 256, (b, size, size, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    batch = SupervisedAugmenter({"resize": True}, {"resize_shape": [size, size]})(images, torch.from_numpy(k), torch.from_numpy(j3d))
    cfg = supervised_config(batch_size=b, num_samples=b * 1000)
    base = dict(batch=b, size=size, backbone="rn50")

    side = torch.cuda.Stream()            # everything on one side stream, as Trainer.fit runs a graph-mode loop
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.manual_seed(0)
        hip = SupervisedPose(cfg).to(dev).train()
        stock = StockPose(cfg).to(dev).to(memory_format=torch.channels_last).train()
        stock.load_state_dict(hip.state_dict())
        graph_m = copy.deepcopy(hip).enable_hip()
        hip.enable_hip()
        t_graph = Trainer(max_epochs=1).attach(graph_m)
        t_graph.zero_grad()
        t_graph.capture_step_graph(batch, warmup=2)
        t_hip, t_stock = Trainer(max_epochs=1).attach(hip), Trainer(max_epochs=1).attach(stock)
        for t in (t_hip, t_stock):
            t.zero_grad()
        count = [0]

        def eager(trainer):
            def step():
                count[0] += 1
                return trainer.training_micro_step(batch, count[0])
            return step

        med = _report("fine-tuning step", {"HIP kernels, eager": eager(t_hip), "HIP kernels, hipGraph replay": t_graph.replay_step,
                                           "stock torch operators, eager": eager(t_stock)}, args.iters, args.runs, base)
        for name in ("HIP kernels, eager", "HIP kernels, hipGraph replay"):
            print(json.dumps(dict(base, what=f"fine-tuning step: stock torch operators, eager / {name}, medians by device events",
                                  ratio=round(med["stock torch operators, eager"] / med[name], 2))), flush=True)
        t_graph.close()

        # ---- the metrics launch against the torch composition, two pairs
        p1, t1 = batch["joints"] + torch.randn_like(batch["joints"]) * 4, batch["joints"]
        p2, t2 = batch["joints3D"] + torch.randn_like(batch["joints3D"]) * 0.01, batch["joints3D"]
        out = torch.empty(4, device=dev)
        fns = {"one launch, eager": lambda: step_metrics(p1, t1, p2, t2, out=out),
               "torch composition, eager": lambda: torch_metrics(p1, t1, p2, t2)}

        def captured(fn):
            fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                graph.keep = fn()
            return graph.replay

        fns["one launch, hipGraph"] = captured(fns["one launch, eager"])
        try:
            fns["torch composition, hipGraph"] = captured(fns["torch composition, eager"])
        except Exception as exc:  # noqa: BLE001 -- reported, not hidden
            print(json.dumps(dict(base, what="step metrics: the torch composition cannot be captured", error=str(exc)[:200])), flush=True)
        a, c = step_metrics(p1, t1, p2, t2).tolist(), [float(v) for v in torch_metrics(p1, t1, p2, t2)]
        med = _report("step metrics, two pairs", fns, 20 * args.iters, args.runs, dict(base, ours=a, torch=c))
        for mode in ("eager", "hipGraph"):
            if f"torch composition, {mode}" in med:
                print(json.dumps(dict(base, what=f"step metrics: torch composition / one launch, {mode}, medians by device events",
                                      ratio=round(med[f"torch composition, {mode}"] / med[f"one launch, {mode}"], 2))), flush=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
