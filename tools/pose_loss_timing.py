"""Time of the supervised pose losses, forward plus backward: `peclr_amd.pose_losses` and `(w . losses).sum().backward()` (two
forward launches, one backward launch, plus the few torch ops of the weighted sum) against the stock-torch composition of the
same formulas on the same device -- cal_l1_loss and cal_3d_loss over convert_2_5D_to_3D with a batched torch.inverse, two
clamps in the autograd graph -- in float32, as the reference runs them.  Warm; a run is ITERS back-to-back steps timed by device
events and, around the same steps, by the wall clock with the device waited for, so the rate at which the host can issue the
launches is part of every figure; the two compositions alternate run by run; median, minimum and maximum over the runs.

    python tools/pose_loss_timing.py [--batch 128] [--iters 300] [--runs 9]
"""
import argparse
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


def torch_losses(pred, joints, joints3d, scale, K, valid):
    """The stock-torch composition: the formulas of cal_l1_loss / cal_3d_loss / convert_2_5D_to_3D / get_root_depth, batched."""
    import torch

    weight = valid / valid.sum()
    loss_2d = ((pred[..., :2] - joints[..., :2]).abs() * weight).sum() / 2
    loss_z = (pred[..., 2:] - joints[..., 2:]).abs() * weight
    loss_zu = (loss_z * scale.view(-1, 1, 1)).sum()
    k_inv = torch.inverse(K)
    ones = torch.ones_like(pred[:, 0, 2:])
    n = torch.bmm(k_inv, torch.cat((pred[:, 0, :2], ones), 1).unsqueeze(2)).squeeze(2)
    m = torch.bmm(k_inv, torch.cat((pred[:, 2, :2], ones), 1).unsqueeze(2)).squeeze(2)
    xn, yn, xm, ym, zn, zm = n[:, 0], n[:, 1], m[:, 0], m[:, 1], pred[:, 0, 2], pred[:, 2, 2]
    a = (xn - xm) ** 2 + (yn - ym) ** 2
    b = 2 * (zn * (xn ** 2 + yn ** 2 - xn * xm - yn * ym) + zm * (xm ** 2 + ym ** 2 - xn * xm - yn * ym))
    c = (xn * zn - xm * zm) ** 2 + (yn * zn - ym * zm) ** 2 + (zn - zm) ** 2 - 1
    z_root = 0.5 * (-b + torch.clamp(b ** 2 - 4 * a * c, min=1e-6) ** 0.5) / torch.clamp(a, min=1e-6)
    depth = (pred[:, :, 2:] + z_root.view(-1, 1, 1)) * scale.view(-1, 1, 1)
    hom = pred.clone()
    hom[:, :, 2] = 1.0
    lifted = torch.bmm(hom, k_inv.transpose(1, 2)) * depth
    loss_3d = ((lifted - joints3d).abs() * weight).sum() / 3
    return loss_2d, loss_z.sum(), loss_zu, loss_3d


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--runs", type=int, default=9)
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from peclr_amd import _capi, pose_losses

    b = args.batch
    g = np.random.default_rng(0)
    k1 = np.array([[480.0, 0, 112], [0, 480.0, 112], [0, 0, 1]], dtype=np.float32)
    z = 0.6 + 0.05 * g.standard_normal((b, 21))
    u, v = 112 + 25 * g.standard_normal((b, 21)), 112 + 25 * g.standard_normal((b, 21))
    J = torch.from_numpy(np.stack([(u - 112) * z / 480, (v - 112) * z / 480, z], axis=2).astype(np.float32)).cuda()
    K = torch.from_numpy(np.repeat(k1[None], b, 0)).cuda()
    joints, scale = _capi.joints3d_to_25d(K, J)
    noise = torch.from_numpy((g.standard_normal((b, 21, 3)) * np.array([4.0, 4.0, 0.15])).astype(np.float32)).cuda()
    pred = (joints + noise).requires_grad_(True)
    valid = torch.from_numpy((g.uniform(size=(b, 21, 1)) >= 0.2).astype(np.float32)).cuda()
    w = (1.0, 1.0, 0.0, 1.0)

    def ours():
        out = pose_losses(pred, joints, J, scale, K, valid)
        pred.grad = None
        (w[0] * out["loss_2d"] + w[1] * out["loss_z"] + w[3] * out["loss_3d"]).backward()

    def stock():
        l2d, lz, lzu, l3d = torch_losses(pred, joints, J, scale, K, valid)
        pred.grad = None
        (w[0] * l2d + w[1] * lz + w[3] * l3d).backward()

    ours()
    ours_grad = pred.grad.clone()
    stock()
    rel = float((pred.grad - ours_grad).abs().max() / ours_grad.abs().max())
    # the two alternate within every run, so that whatever else the machine does meets both; one run of each is thrown away
    fns = {"pose_losses": ours, "stock-torch composition": stock}
    samples = {name: [] for name in fns}
    for run in range(args.runs + 1):
        for name, fn in fns.items():
            t = _time_once(fn, args.iters)
            if run:
                samples[name].append(t)
    rows = []
    base = {"batch": b, "weights": list(w), "iters": args.iters, "runs": args.runs, "grad_max_rel_diff_between_the_two": rel}
    for name in fns:
        for i, clock in enumerate(("device events", "wall clock")):
            us = [t[i] for t in samples[name]]
            rows.append(dict(base, what=f"{name}, forward + backward, {clock}", median_us=round(statistics.median(us), 2),
                             min_us=round(min(us), 2), max_us=round(max(us), 2)))
            print(json.dumps(rows[-1]), flush=True)
    med = {name: statistics.median(t[0] for t in samples[name]) for name in fns}
    print(json.dumps(dict(base, what="stock-torch composition / pose_losses, medians by device events",
                          ratio=round(med["stock-torch composition"] / med["pose_losses"], 2))), flush=True)
    return rows


if __name__ == "__main__":
    main()
