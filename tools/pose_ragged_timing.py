"""What the any-size predictor costs next to the FreiHAND one: whole-predict device time of three arms, same run, alternated.

    python tools/pose_ragged_timing.py [--batch 128] [--windows 7] [--iters 10] [--precisions fp32 bf16] [--out FILE]

    freihand     pose.FreiHANDPredictor on B images of 224 x 224 (one uint8 tensor on the device)
    hand_dense   predict.HandPosePredictor on the same tensor (the uniform case of the packed crop kernel, plus the unmap launch)
    hand_ragged  predict.HandPosePredictor on a `RaggedImages` of B images of mixed sizes with the same total pixel count (on the
                 device, as the tensor of the other two arms is)

rn50, synthetic images, K_DEFAULT, no boxes, no left hands; 16-bit arms with the BatchNorm folding that is their default.  Every
(arm, precision) is timed in `windows` windows of `iters` calls from device events, the arms taking turns inside a window, and
the row gives the median window with the smallest and the largest: every eager window first, then the captures and the replay
windows, as tools/pose_timing.py does.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# eight shapes of 8 x 224 x 224 pixels in all: the same area four ways, half and one and a half times the area, two transposes
SHAPES = [(224, 224), (196, 256), (128, 392), (448, 112), (112, 224), (336, 224), (256, 196), (392, 128)]


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
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=128, help="a multiple of 8 (the cycle of shapes)")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--precisions", nargs="+", choices=("fp32", "bf16", "fp16"), default=["fp32", "bf16"])
    ap.add_argument("--out", default=None, help="also write the table there")
    args = ap.parse_args(argv)
    b = args.batch
    if b < 8 or b % len(SHAPES):
        raise SystemExit(f"--batch must be a multiple of {len(SHAPES)}")

    import torch

    from peclr_amd.augment import RaggedImages
    from peclr_amd.pose import K_DEFAULT, FreiHANDPredictor, RN25DwMLPref
    from peclr_amd.predict import HandPosePredictor

    torch.manual_seed(0)
    model = RN25DwMLPref("rn50").eval().to("cuda").enable_hip()
    with torch.no_grad():   # keypoints spread over the crop, so that the re-crop is a real crop (as tools/pose_timing.py)
        model.backend_model.fc.weight.mul_(0.05)
        model.backend_model.fc.bias.copy_(torch.tensor([112.0, 112.0, 0.0] * 21 + [0.0]))
        for blk in model.backend_model.modules():
            if hasattr(blk, "bn3"):
                blk.bn3.weight.fill_(0.2)
    rng = np.random.default_rng(b)
    dense = torch.from_numpy(rng.integers(0, 256, (b, 224, 224, 3), dtype=np.uint8)).cuda()
    sizes = [SHAPES[i % len(SHAPES)] for i in range(b)]
    ragged = RaggedImages.from_list([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes], dense.device)
    assert ragged.data.numel() == dense.numel()
    K = torch.tensor(K_DEFAULT, dtype=torch.float64).expand(b, 3, 3).contiguous().cuda()
    scale = torch.full((b,), 0.03, dtype=torch.float64).cuda()

    lines, eager, graph, preds = [], {}, {}, {}
    for p in args.precisions:
        old, new_d, new_r = FreiHANDPredictor(model, precision=p), HandPosePredictor(model, precision=p), HandPosePredictor(model, precision=p)
        preds[p] = (old, new_d, new_r)
        eager[(p, "freihand")] = lambda old=old: old.predict(dense, K, scale)
        eager[(p, "hand_dense")] = lambda new=new_d: new.predict(dense, K, scale)
        eager[(p, "hand_ragged")] = lambda new=new_r: new.predict(ragged, K, scale)
    times = {(k, "eager"): [] for k in eager}
    for _ in range(args.windows):
        for k, fn in eager.items():
            times[(k, "eager")].append(_time(fn, args.iters))
    for p, (old, new_d, new_r) in preds.items():
        old.capture(b)
        new_d.capture(b, dense.numel())
        new_r.capture(b, ragged.data.numel())
        graph[(p, "freihand")] = lambda old=old: old.replay(dense, K, scale)
        graph[(p, "hand_dense")] = lambda new=new_d: new.replay(dense, K, scale)
        graph[(p, "hand_ragged")] = lambda new=new_r: new.replay(ragged, K, scale)
    times.update({(k, "graph"): [] for k in graph})
    for _ in range(args.windows):
        for k, fn in graph.items():
            times[(k, "graph")].append(_time(fn, args.iters))
    for (p, arm) in eager:
        row = {"backend": "rn50", "batch": b, "precision": p, "fold_bn": preds[p][0].fold_bn, "arm": arm, "windows": args.windows,
               "iters": args.iters}
        for mode in ("eager", "graph"):
            t = times[((p, arm), mode)]
            row.update({f"{mode}_ms": round(float(np.median(t)), 3), f"{mode}_min_ms": round(min(t), 3), f"{mode}_max_ms": round(max(t), 3)})
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    for p in args.precisions:
        for mode in ("eager", "graph"):
            base = times[((p, "freihand"), mode)]
            med = float(np.median(base))
            parts = [f"{p} {mode}: freihand {med:.3f} ms (windows {min(base):.3f} .. {max(base):.3f})"]
            for arm in ("hand_dense", "hand_ragged"):
                m = float(np.median(times[((p, arm), mode)]))
                parts.append(f"{arm} {m:.3f} ms ({(m - med) / med * 100:+.2f} %, {'inside' if min(base) <= m <= max(base) else 'outside'} that spread)")
            lines.append(" | ".join(parts))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
