"""Time of one supervised fine-tuning step of the 2.5D pose model (ResNet-50, B = 128, 224 x 224): forward, the four losses, the
step metrics, backward and the fused Adam step -- `SupervisedPose` on the HIP kernels in fp32, bf16 and fp16 (the backbone under
the trainer's autocast on the 16-bit convolution kernels; fp16 with the `DeviceLossScaler` inside the optimiser launch), each
issued eagerly and replayed from the one hipGraph `Trainer.capture_step_graph` records, against the stock-torch step of the same
model (tools/stock_pose_step.py: no `enable_hip*`, same optimiser) in fp32 and under torch's autocast (fp16: with
`torch.amp.GradScaler`), all in the same run on the same machine.  Then one `validation_step` at the same batch: fp32, and
16-bit with the eval BatchNorm layers as passes of their own and folded into the convolution epilogues.  And the step-metrics
launch (`peclr_pose_step_metrics_f32`, both pairs) against the torch composition of calculate_metrics for two pairs.

Warm; a run is ITERS back-to-back steps timed by device events and, around the same steps, by the wall clock with the device
waited for; the arms alternate run by run; median, minimum and maximum over the runs.  What the figures are: for the whole
step the device is busy for tens of milliseconds per step, so every figure is DEVICE TIME (eager and replayed differ by what
the host cannot issue fast enough).  For the metrics the eager figures are LAUNCH-ISSUE RATES -- the device finishes each launch
before the host has issued the next -- and only the figures from a hipGraph (each composition captured once) are device time.

    python tools/pose_finetune_timing.py [--precision fp32 bf16 fp16] [--batch 128] [--size 224] [--iters 10] [--runs 5]
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
    ap.add_argument("--precision", nargs="+", choices=("fp32", "bf16", "fp16"), default=["fp32", "bf16", "fp16"],
                    help="the precisions whose arms are timed (fp32 is the comparison base of the 16-bit ones: keep it)")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from peclr_amd import SupervisedAugmenter, SupervisedPose, Trainer, step_metrics, supervised_config
    from stock_pose_step import StockPose, metrics as torch_metrics, use_torch_grad_scaler

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
        first = SupervisedPose(cfg).to(dev).train()
        count = [0]

        def eager(trainer):
            def step():
                count[0] += 1
                return trainer.training_micro_step(batch, count[0])
            return step

        # every graph is captured before the first eager step of the process (Trainer.capture_step_graph)
        fns, graphs, eager_arms = {}, [], []
        for p in args.precision:
            graph_m = copy.deepcopy(first).enable_hip()
            t_graph = Trainer(max_epochs=1, precision=p).attach(graph_m)
            t_graph.zero_grad()
            t_graph.capture_step_graph(batch, warmup=2)
            graphs.append(t_graph)
            fns[f"HIP kernels {p}, hipGraph replay"] = t_graph.replay_step
        for p in args.precision:
            hip = copy.deepcopy(first).enable_hip()
            stock = StockPose(cfg).to(dev).to(memory_format=torch.channels_last).train()
            stock.load_state_dict(first.state_dict())
            t_hip = Trainer(max_epochs=1, precision=p).attach(hip)
            t_stock = use_torch_grad_scaler(Trainer(max_epochs=1, precision=p).attach(stock))
            for t in (t_hip, t_stock):
                t.zero_grad()
            fns[f"HIP kernels {p}, eager"] = eager(t_hip)
            fns[f"stock torch operators {p}, eager"] = eager(t_stock)
        med = _report("fine-tuning step", fns, args.iters, args.runs, base)
        for p in args.precision:
            for other in dict.fromkeys(("fp32", p)):
                for base_arm in (f"stock torch operators {other}, eager", f"HIP kernels {other}, eager", f"HIP kernels {other}, hipGraph replay"):
                    for name in (f"HIP kernels {p}, eager", f"HIP kernels {p}, hipGraph replay"):
                        if base_arm in med and base_arm != name and (other != p or base_arm.startswith("stock")):
                            print(json.dumps(dict(base, what=f"fine-tuning step: {base_arm} / {name}, medians by device events",
                                                  ratio=round(med[base_arm] / med[name], 2))), flush=True)
        for t in graphs:
            t.close()
        del fns, graphs

        # ---- one validation step: fp32, and 16-bit with the eval BatchNorm layers unfolded and folded
        vals = {}
        for p in args.precision:
            for fold in ((False,) if p == "fp32" else (False, True)):
                vm = SupervisedPose(cfg, fold_bn=fold).to(dev).enable_hip()
                vm.load_state_dict(first.state_dict())
                Trainer(max_epochs=1, precision=p).attach(vm.eval())
                name = "HIP kernels fp32" if p == "fp32" else f"HIP kernels {p}, BatchNorm {'folded' if fold else 'unfolded'}"
                vals[name] = (lambda m: lambda: m.validation_step(batch, 0))(vm)
        med = _report("validation step", vals, args.iters, args.runs, base)
        for name in vals:
            if name != "HIP kernels fp32" and "HIP kernels fp32" in med:
                print(json.dumps(dict(base, what=f"validation step: HIP kernels fp32 / {name}, medians by device events",
                                      ratio=round(med["HIP kernels fp32"] / med[name], 2))), flush=True)
        del vals

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
