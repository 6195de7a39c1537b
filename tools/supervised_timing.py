"""Time of the label side of a supervised batch: ONE `peclr_supervised_labels` launch (warm, device events: the median over
repeated runs of ITERS back-to-back launches, so the rate at which the host can issue them is part of the figure) against the
per-sample host composition of the same functions -- convert_to_2_5D, the matrix applied to the joints, T @ K,
convert_2_5D_to_3D with torch.inverse, per sample in float32 torch ops on the CPU as a dataset's __getitem__ runs them, then
stacked and copied to the device (wall clock, the copy waited for).  Also the two
conversion launches alone, and the launch as the caller sees it (allocations and ctypes marshalling included, wall clock).

    python tools/supervised_timing.py [--batch 128] [--iters 50] [--runs 9] [--use-palm]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time_device(fn, iters, runs):
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


def _time_wall(fn, iters, runs):
    import torch

    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e6)
    return statistics.median(out), min(out), max(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--use-palm", action="store_true")
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from peclr_amd import _capi
    from peclr_amd.augment import convert_to_2_5d

    b, palm = args.batch, args.use_palm
    g = np.random.default_rng(0)
    k1 = np.array([[480.0, 0, 112], [0, 480.0, 112], [0, 0, 1]], dtype=np.float32)
    z = 0.6 + 0.05 * g.standard_normal((b, 21))
    u, v = 112 + 25 * g.standard_normal((b, 21)), 112 + 25 * g.standard_normal((b, 21))
    j_host = torch.from_numpy(np.stack([(u - 112) * z / 480, (v - 112) * z / 480, z], axis=2).astype(np.float32))
    k_host = torch.from_numpy(np.repeat(k1[None], b, 0))
    ang = g.uniform(-0.7, 0.7, b)
    t_host = torch.from_numpy(np.array([[[1.1 * np.cos(a), 1.1 * np.sin(a), -20.0], [-1.1 * np.sin(a), 1.1 * np.cos(a), 15.0],
                                         [0, 0, 1]] for a in ang]))
    K, J, T = k_host.cuda(), j_host.cuda(), t_host.cuda()

    def launch():
        _capi.supervised_labels(K, J, T, palm)

    j25, scale = _capi.joints3d_to_25d(K, J)

    def to_25d():
        _capi.joints3d_to_25d(K, J)

    def to_3d():
        _capi.joints25d_to_3d(j25, scale, K)

    def host_sample(k, j3d, t):
        """prepare_supervised_sample's label side for one sample, float32 torch ops on the CPU."""
        joints, s = convert_to_2_5d(k, j3d)
        t32 = t.float()
        hom = joints.clone()
        hom[:, 2] = 1.0
        joints[:, :2] = (hom @ t32.T)[:, :2]
        k_new = t32 @ k
        if palm:
            j3d = j3d.clone()
            j3d[0] = (j3d[0] + j3d[2]) / 2
            joints, s = convert_to_2_5d(k_new, j3d)
        k_inv = torch.inverse(k_new)
        xn, yn, _ = k_inv @ torch.cat((joints[0, :2], torch.tensor([1.0])))
        xm, ym, _ = k_inv @ torch.cat((joints[2, :2], torch.tensor([1.0])))
        zn, zm = joints[0, 2], joints[2, 2]
        a = (xn - xm) ** 2 + (yn - ym) ** 2
        bb = 2 * (zn * (xn ** 2 + yn ** 2 - xn * xm - yn * ym) + zm * (xm ** 2 + ym ** 2 - xn * xm - yn * ym))
        c = (xn * zn - xm * zm) ** 2 + (yn * zn - ym * zm) ** 2 + (zn - zm) ** 2 - 1
        z_root = 0.5 * (-bb + torch.clamp(bb ** 2 - 4 * a * c, min=1e-6) ** 0.5) / torch.clamp(a, min=1e-6)
        hom = joints.clone()
        hom[:, 2] = 1.0
        rec = (hom @ k_inv.T) * ((joints[:, 2:] + z_root) * s)
        return joints, k_new, s, j3d, rec, t32

    def host_batch():
        rows = [host_sample(k_host[i], j_host[i], t_host[i]) for i in range(b)]
        return [torch.stack(col).cuda(non_blocking=True) for col in zip(*rows)]

    torch.set_num_threads(1)  # a DataLoader worker's setting
    rows = []
    base = {"batch": b, "use_palm": palm}
    for name, fn, timer, iters in (("peclr_supervised_labels, back-to-back launches, device events", launch, _time_device, args.iters),
                                   ("peclr_joints3d_to_25d, back-to-back launches, device events", to_25d, _time_device, args.iters),
                                   ("peclr_joints25d_to_3d, back-to-back launches, device events", to_3d, _time_device, args.iters),
                                   ("peclr_supervised_labels as called (allocations + ctypes), wall clock", launch, _time_wall, args.iters),
                                   ("per-sample host composition + stack + copy, wall clock, 1 thread", host_batch, _time_wall, 3)):
        med, lo, hi = timer(fn, iters, args.runs)
        rows.append(dict(base, what=name, median_us=round(med, 2), min_us=round(lo, 2), max_us=round(hi, 2), iters=iters,
                         runs=args.runs))
        print(json.dumps(rows[-1]), flush=True)
    return rows


if __name__ == "__main__":
    main()
