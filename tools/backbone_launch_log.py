"""Record what one forward + backward of the fused backbone launches, and what it computes, on the present GPU:

    python tools/backbone_launch_log.py OUT.json [label of the tree, e.g. its commit] [OTHER.json ...]

Per case (a ResNet, a routing, an autocast dtype; batch 2 of 3 x 64 x 64 channels_last images, train mode, HIP BatchNorm on):
`_capi.LAUNCH_ORDER` (the tags of the in-tree launches, in order), every aten convolution / convolution_backward a
TorchDispatchMode sees (the MIOpen arms: shapes, dtype, stride, output mask) and the sha256 of the output, of the input
gradient and of every parameter gradient.  64 x 64 is the smallest image that still has both weight-gradient routes (layer1 / 2
at 16 and 8 columns, layer3 / 4 at 4 and 2) with every width at 64 channels or more.

OTHER.json: earlier recordings of the same tree -- a hash that differs between any of them and this run is dropped from OUT
(and named under "dropped_hashes"): it belongs to an arm that is not fixed-order; so does every weight gradient MIOpen computed,
whose hash is dropped even where the runs agreed (`drop_unstable`).  Launch order and the aten list always stay.
tests/golden/backbone_launch_log.json is that log of the commit named in its first key;
tests/test_backbone_launch_log_gpu.py compares the working tree with it.  Only names that commit has are used."""
import contextlib
import hashlib
import json
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from peclr_amd import _capi, bn2d, resnet  # noqa: E402

DEV = "cuda"
FORCE = dict(force=True)
# name -> (resnet constructor, routing overrides, autocast dtype, side-stream weight gradients, checkpointed layer)
CASES = {
    "rn50_force": ("resnet50", FORCE, None, False, None),
    "rn50_force_no_pair": ("resnet50", dict(force=True, x6_pair=False), None, False, None),
    "rn50_force_bf16": ("resnet50", FORCE, torch.bfloat16, False, None),
    "rn50_force_fp16": ("resnet50", FORCE, torch.float16, False, None),
    "rn18_force": ("resnet18", FORCE, None, False, None),
    "rn50_default": ("resnet50", {}, None, False, None),
    "rn50_force_no_x6p": ("resnet50", dict(force=True, gemm_x6p=False), None, False, None),
    "rn50_force_no_x6t": ("resnet50", dict(force=True, gemm_x6t=False), None, False, None),
    "rn50_force_no_s2_compact": ("resnet50", dict(force=True, s2_dgrad_compact=False), None, False, None),
    "rn50_force_no_s2_dgrad": ("resnet50", dict(force=True, conv_s2_dgrad_x6=False), None, False, None),
    "rn50_force_side_stream": ("resnet50", FORCE, None, True, None),
    "rn50_force_checkpoint_layer2": ("resnet50", FORCE, None, False, "layer2"),
}


class _AtenConvs(TorchDispatchMode):
    """The aten convolutions that run under it: [name, dtype, operand shapes ..., stride, (output mask)]."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        packet = getattr(func, "_overloadpacket", None)
        if packet is torch.ops.aten.convolution:
            self.seen.append(["convolution", str(args[0].dtype), list(args[0].shape), list(args[1].shape), list(args[3])])
        elif packet is torch.ops.aten.convolution_backward:
            self.seen.append(["convolution_backward", str(args[0].dtype), list(args[0].shape), list(args[1].shape), list(args[2].shape),
                              list(args[4]), list(args[10])])
        return func(*args, **(kwargs or {}))


def _sha(t):
    """sha256 of the elements in logical (row-major) order, whatever the strides."""
    return hashlib.sha256(t.detach().cpu().reshape(-1).contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def record_case(name):
    """One forward + backward of case `name`: {"case", "launches", "aten", "hashes"}."""
    arch, overrides, half, side_stream, ckpt = CASES[name]
    torch.manual_seed(7)
    net = getattr(resnet, arch)().to(DEV).to(memory_format=torch.channels_last).train()
    bn2d.enable_hip_batchnorm(net)
    for block in (getattr(net, ckpt) if ckpt else ()):
        block.checkpoint = True
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 3, 64, 64, generator=g).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    gy = torch.randn(2, 1000, generator=g).to(DEV)
    torch.cuda.synchronize()
    saved = (_capi.EVENT_LOG, _capi.LAUNCH_ORDER)
    _capi.EVENT_LOG, _capi.LAUNCH_ORDER = {}, []
    convs = _AtenConvs()
    autocast = torch.autocast("cuda", dtype=half) if half is not None else contextlib.nullcontext()
    try:
        if side_stream:
            bn2d.enable_wgrad_overlap(True)
            bn2d.arm_wgrad_overlap()
        with bn2d.routing(**overrides), convs:
            with autocast:
                y = net(x)
            y.backward(gy.to(y.dtype))
            if side_stream:
                bn2d.wgrad_join()
            bn2d.end_backward()
        torch.cuda.synchronize()
        launches = list(_capi.LAUNCH_ORDER)
    finally:
        _capi.EVENT_LOG, _capi.LAUNCH_ORDER = saved
        if side_stream:
            bn2d.enable_wgrad_overlap(False)
    hashes = {"output": _sha(y), "input.grad": _sha(x.grad)}
    for pname, p in net.named_parameters():
        hashes[pname + ".grad"] = _sha(p.grad)
    return {"case": name, "launches": launches, "aten": convs.seen, "hashes": hashes}


def record(label="working tree"):
    return {"recorded_from": label, "dropped_hashes": [], "cases": [record_case(name) for name in CASES]}


def drop_unstable(log, others):
    """Remove from `log` every hash that another recording of the same tree does not reproduce, and -- MIOpen's weight gradients
    are not fixed-order: two runs that agree prove nothing -- the hash of every weight gradient shaped like one MIOpen computed
    in that case (aten convolution_backward with the weight's output mask); a case whose output differed keeps no hash at all.
    They are listed as "case:key"."""
    for case in log["cases"]:
        shapes = {name + ".grad": list(p.shape) for name, p in getattr(resnet, CASES[case["case"]][0])().named_parameters()}
        miopen = [a[4] for a in case["aten"] if a[0] == "convolution_backward" and a[6][1]]
        drop = {k for k in case["hashes"] if shapes.get(k) in miopen}
        for other in others:
            theirs = next(c for c in other["cases"] if c["case"] == case["case"])
            assert theirs["launches"] == case["launches"] and theirs["aten"] == case["aten"], case["case"]
            drop |= {k for k, v in case["hashes"].items() if theirs["hashes"].get(k) != v}
        if "output" in drop:                     # the forward itself is not reproducible: nothing behind it is
            drop = set(case["hashes"])
        for key in [k for k in case["hashes"] if k in drop]:
            del case["hashes"][key]
            log["dropped_hashes"].append(f"{case['case']}:{key}")
    return log


def write(log, path):
    with open(path, "w") as f:
        f.write('{"recorded_from": %s,\n"dropped_hashes": %s,\n"cases": [\n' % (json.dumps(log["recorded_from"]), json.dumps(log["dropped_hashes"])))
        f.write(",\n".join(json.dumps(c) for c in log["cases"]))
        f.write("\n]}\n")


def main(argv):
    log = record(argv[1] if len(argv) > 1 else "working tree")
    others = []
    for path in argv[2:]:
        with open(path) as f:
            others.append(json.load(f))
    write(drop_unstable(log, others), argv[0])
    print(f"{len(log['cases'])} cases, {sum(len(c['launches']) for c in log['cases'])} launches, "
          f"{sum(len(c['aten']) for c in log['cases'])} aten convolutions, {len(log['dropped_hashes'])} hashes dropped")


if __name__ == "__main__":
    main(sys.argv[1:])
