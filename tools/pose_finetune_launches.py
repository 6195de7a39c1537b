"""Launch inventory of one supervised fine-tuning step of the 2.5D pose model (ResNet-50, B = 128, 224 x 224) at a 16-bit
precision: what `Trainer.training_micro_step` launches on the present GPU, from both sides --

- the in-tree launches: `_capi.EVENT_LOG` (tag, kernel, number of launches, device time by the events around each launch);
- everything else: every aten operator a TorchDispatchMode sees during the same step (forward, backward through the autograd
  engine, optimiser), with the number of calls and the largest output; views are left out.  An operator whose largest output
  has 2^20 elements or more is a tensor-sized pass and is marked `<-- tensor-sized`.  aten convolution_backward entries are
  listed with their shapes: they are the weight gradients that stay with MIOpen.

The step is run eagerly, after two warm-up steps, under the default routing -- what a user's run launches.

    python tools/pose_finetune_launches.py [--precision bf16 fp16] [--batch 128] [--size 224] [OUT.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

TENSOR_SIZED = 1 << 20


class _AtenOps(TorchDispatchMode):
    """name -> [calls, elements of the largest output, its shape and dtype]; convolution_backward calls with their shapes."""

    def __init__(self):
        super().__init__()
        self.ops, self.conv_backward = {}, []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if getattr(func, "is_view", False):
            return out
        name = str(func)
        outs = [t for t in (out if isinstance(out, (tuple, list)) else (out,)) if isinstance(t, torch.Tensor)]
        big = max(outs, key=lambda t: t.numel(), default=None)
        entry = self.ops.setdefault(name, [0, 0, None])
        entry[0] += 1
        if big is not None and big.numel() >= entry[1]:
            entry[1], entry[2] = big.numel(), f"{list(big.shape)} {str(big.dtype).replace('torch.', '')}"
        if getattr(func, "_overloadpacket", None) is torch.ops.aten.convolution_backward:
            self.conv_backward.append(f"grad {list(args[0].shape)} input {list(args[1].shape)} weight {list(args[2].shape)} "
                                      f"stride {list(args[4])} mask {list(args[10])} {str(args[0].dtype).replace('torch.', '')}")
        return out


def make_batch(b, size, dev):
    from peclr_amd import SupervisedAugmenter

    g = np.random.default_rng(0)
    focal = 480.0 * size / 224
    k = np.repeat(np.array([[focal, 0, size / 2], [0, focal, size / 2], [0, 0, 1]], dtype=np.float32)[None], b, 0)
    z = 0.6 + 0.05 * g.standard_normal((b, 21))
    uv = g.uniform(0.35, 0.65, (b, 1, 2)) * size + size / 9 * g.standard_normal((b, 21, 2))
    j3d = np.concatenate([(uv - size / 2) * z[..., None] / focal, z[..., None]], axis=2).astype(np.float32)
    images = torch.randint(0, 256, (b, size, size, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    return SupervisedAugmenter({"resize": True}, {"resize_shape": [size, size]})(images, torch.from_numpy(k), torch.from_numpy(j3d))


def inventory(precision, b, size, dev="cuda"):
    """One logged step -> the lines of its inventory."""
    from peclr_amd import SupervisedPose, Trainer, _capi, supervised_config

    batch = make_batch(b, size, dev)
    torch.manual_seed(0)
    m = SupervisedPose(supervised_config(batch_size=b, num_samples=b * 1000)).to(dev).train().enable_hip()
    tr = Trainer(max_epochs=1, precision=precision).attach(m)
    tr.zero_grad()
    for i in range(2):
        tr.training_micro_step(batch, i)
    torch.cuda.synchronize()
    ops = _AtenOps()
    _capi.EVENT_LOG, _capi.LAUNCH_ORDER = {}, []
    try:
        with ops:
            tr.training_micro_step(batch, 2)
        torch.cuda.synchronize()
        log, order = _capi.EVENT_LOG, _capi.LAUNCH_ORDER
    finally:
        _capi.EVENT_LOG, _capi.LAUNCH_ORDER = None, None
    lines = [f"== one fine-tuning step, rn50, B = {b}, {size} x {size}, precision {precision}: "
             f"{len(order)} in-tree entries, {sum(v[0] for v in ops.ops.values())} aten operator calls (views left out)", "",
             "in-tree launches (EVENT_LOG): tag | kernel | entries | device ms"]
    total = 0.0
    for tag, events in log.items():
        ms = sum(s.elapsed_time(e) for s, e, *_ in events)
        total += ms
        kernels = sorted({str(ev[4]) for ev in events})
        lines.append(f"  {tag:28s} | {', '.join(kernels):44s} | {len(events):4d} | {ms:8.3f}")
    lines += [f"  sum of the in-tree entries: {total:.3f} ms", "", "aten operators: name | calls | largest output"]
    for name, (calls, numel, what) in sorted(ops.ops.items(), key=lambda kv: -kv[1][1]):
        lines.append(f"  {name:44s} | {calls:4d} | {what}{'   <-- tensor-sized' if numel >= TENSOR_SIZED else ''}")
    lines += ["", f"aten convolution_backward calls (MIOpen): {len(ops.conv_backward)}"] + ["  " + c for c in ops.conv_backward] + [""]
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", nargs="+", choices=("fp32", "bf16", "fp16"), default=["bf16", "fp16"])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("out", nargs="?")
    args = ap.parse_args(argv)
    lines = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for p in args.precision:
            lines += inventory(p, args.batch, args.size)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
