"""Time of one `peclr_pose_eval` launch (raw distances, Procrustes alignment, PCK counts of 100 thresholds) at a given batch,
warm, with device events: the median over repeated runs of ITERS back-to-back launches.  Next to it, the same quantities from
stock torch ops (torch.linalg.svd and one comparison per threshold, the reference's composition without its .cpu() calls).

    python tools/pose_eval_timing.py [--batch 128] [--iters 50] [--runs 9] [--dtype float64]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters, runs):
    import torch

    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) / iters * 1e3)
    return statistics.median(out), min(out), max(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float64")
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from peclr_amd import _capi

    dtype = getattr(torch, args.dtype)
    torch.manual_seed(0)
    b = args.batch
    gt = (torch.randn(b, 21, 3, dtype=dtype) * 0.04 + torch.tensor([0.05, -0.03, 0.6], dtype=dtype)).cuda()
    pred = gt + torch.randn(b, 21, 3, dtype=dtype).cuda() * 0.02
    thr_np = np.arange(0.0, 0.5, 0.005)
    thr = torch.from_numpy(thr_np).to(dtype).cuda()
    counts = torch.zeros((2, 21, len(thr_np)), dtype=torch.int64, device="cuda")
    dist, dist_al = (torch.empty((b, 21), dtype=dtype, device="cuda") for _ in range(2))
    status = torch.zeros((b,), dtype=torch.int32, device="cuda")

    def hip():
        _capi.pose_eval(pred, gt, thr=thr, counts=counts, status=status, dist=dist, dist_aligned=dist_al, want_transform=False)

    def composed():
        d = ((pred - gt) ** 2).sum(2) ** 0.5
        muX, muY = gt.mean(1, keepdim=True), pred.mean(1, keepdim=True)
        X0, Y0 = gt - muX, pred - muY
        nX, nY = (torch.linalg.norm(t, dim=[1, 2], ord="fro", keepdim=True) for t in (X0, Y0))
        X0, Y0 = X0 / nX, Y0 / nY
        U, s, Vh = torch.linalg.svd(torch.bmm(X0.transpose(2, 1), Y0))
        V = Vh.transpose(2, 1).clone()
        sg = torch.sign(torch.det(torch.bmm(V, U.transpose(2, 1))))
        V[:, :, -1] *= sg.view(-1, 1)
        s = s.clone()
        s[:, -1] *= sg
        yt = nX * s.sum(1).view(-1, 1, 1) * torch.matmul(Y0, torch.matmul(V, U.transpose(2, 1))) + muX
        da = ((yt - gt) ** 2).sum(2) ** 0.5
        return [torch.mean((x < t) * 1.0, axis=0) for x in (d, da) for t in thr_np]

    def hip_no_counts():
        _capi.pose_eval(pred, gt, status=status, dist=dist, dist_aligned=dist_al, want_transform=False)

    def hip_dist_only():
        _capi.pose_eval(pred, gt, procrustes=False, status=status, dist=dist)

    rows = []
    for name, fn in (("peclr_pose_eval", hip), ("peclr_pose_eval without PCK counts", hip_no_counts),
                     ("peclr_pose_eval raw distances only", hip_dist_only),
                     ("torch composition (linalg.svd, 200 reductions)", composed)):
        med, lo, hi = _time(fn, args.iters, args.runs)
        rows.append({"what": name, "batch": b, "dtype": args.dtype, "median_us": round(med, 2), "min_us": round(lo, 2),
                     "max_us": round(hi, 2), "iters": args.iters, "runs": args.runs})
        print(json.dumps(rows[-1]), flush=True)
    return rows


if __name__ == "__main__":
    main()
