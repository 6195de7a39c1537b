"""Time of the 2.5D pose head in train mode, forward plus backward, from pooled features to the gradients of the features, of fc
and of the MLP: the HIP training head (`RN25DwMLPref.enable_hip_training()`: four forward and six backward launches plus the
few torch ops of the test loss) against the stock-torch composition on the same device in the same run (`_head_stock` on
`fc(features)` in train mode -- what the model runs without the switch).  Warm; a run is ITERS back-to-back steps timed by
device events and, around the same steps, by the wall clock with the device waited for: eager figures contain the rate at which
the host can issue the launches, the figures from a hipGraph (each step captured once, replayed ITERS times) do not.  The
stock path's `K.inverse()` cannot be captured (hipErrorStreamCaptureUnsupported), so its graph gets K^-1 computed once outside
-- the stock train step as it stands is not capturable at all.  The two compositions alternate run by run; median, minimum and
maximum over the runs.

    python tools/pose_head_train_timing.py [--batch 128] [--iters 300] [--runs 9]
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
    """`iters` back-to-back steps -> (microseconds per step by device events, by the wall clock with the device waited for)."""
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


class _KnownInverse:
    """Stands in for K in `_head_stock` under capture: `inverse()` hands out the matrix computed beforehand."""

    def __init__(self, K):
        self.device, self._inv = K.device, K.inverse()

    def inverse(self):
        return self._inv


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--runs", type=int, default=9)
    args = ap.parse_args(argv)

    import torch

    from peclr_amd.pose import RN25DwMLPref

    b = args.batch
    torch.manual_seed(0)
    hip = RN25DwMLPref("rn50").to("cuda").enable_hip().train()
    with torch.no_grad():       # keypoints spread over the image, so that the closed form is on its regular branch
        centre = torch.tensor([112.0, 112.0, 0.0]).repeat(21) + torch.randn(63) * torch.tensor([30.0, 30.0, 0.2]).repeat(21)
        hip.backend_model.fc.bias.copy_(torch.cat([centre, torch.zeros(1)]))
    stock = copy.deepcopy(hip)
    hip.enable_hip_training()
    feat = torch.randn(b, 2048, device="cuda").relu_().requires_grad_(True)
    g3 = torch.randn(b, 21, 3, device="cuda")
    g25 = torch.randn(b, 21, 3, device="cuda")

    def params(m):
        return [feat, *m.backend_model.fc.parameters(), *m.zroot_ref.zroot_ref.parameters()]

    def ours():
        out = hip.head(feat, None)
        return torch.autograd.grad((out["kp3d"] * g3).sum() + (out["kp25d"] * g25).sum() + out["zroot"].sum(), params(hip))

    def theirs(K=None):
        out = stock._head_stock(stock.backend_model.fc(feat), stock.K_default if K is None else K)
        return torch.autograd.grad((out["kp3d"] * g3).sum() + (out["kp25d"] * g25).sum() + out["kp3d"][:, 0, 2].sum(), params(stock))

    a, c = ours(), theirs()
    rel = max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(a[:3] + a[3:4] + a[5:6], c[:3] + c[3:4] + c[5:6]))

    def captured(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            keep = fn()
        graph.keep = keep
        return graph.replay

    # the two alternate within every run, so that whatever else the machine does meets both; one run of each is thrown away
    fns = {"HIP training head, eager": ours, "stock-torch composition, eager": theirs,
           "HIP training head, hipGraph": captured(ours), "stock-torch composition (K^-1 outside), hipGraph": captured(lambda K=_KnownInverse(stock.K_default): theirs(K))}
    samples = {name: [] for name in fns}
    for run in range(args.runs + 1):
        for name, fn in fns.items():
            t = _time_once(fn, args.iters)
            if run:
                samples[name].append(t)
    rows = []
    base = {"batch": b, "iters": args.iters, "runs": args.runs, "grad_max_rel_diff_between_the_two": rel}
    for name in fns:
        for i, clock in enumerate(("device events", "wall clock")):
            us = [t[i] for t in samples[name]]
            rows.append(dict(base, what=f"{name}, forward + backward, {clock}", median_us=round(statistics.median(us), 2),
                             min_us=round(min(us), 2), max_us=round(max(us), 2)))
            print(json.dumps(rows[-1]), flush=True)
    med = {name: statistics.median(t[0] for t in samples[name]) for name in fns}
    for mode, theirs_name in (("eager", "stock-torch composition, eager"), ("hipGraph", "stock-torch composition (K^-1 outside), hipGraph")):
        print(json.dumps(dict(base, what=f"stock-torch composition / HIP training head, {mode}, medians by device events",
                              ratio=round(med[theirs_name] / med[f"HIP training head, {mode}"], 2))), flush=True)
    return rows


if __name__ == "__main__":
    main()
