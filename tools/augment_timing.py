#!/usr/bin/env python
"""Two-view augmentation: where the time goes (host parameter draws vs the two HIP launches) and how it
compares with the CPU restatement of the reference's per-sample pipeline.  The last row turns on all ten of
the reference's flags (TwoViewAugmenter(extended=True)): stage 0 ("augment_pre"), one warp per view, and the
noise / colour-drop form of stage 2.  kernel_us: device-event time per call, summed over a name's launches.
With a second file name it also times batches whose images differ in size (`RaggedImages`, recipe flags, B = 128,
128 x 128 out): five repeats of the uniform 224 x 224 row (their spread is the yardstick), (a) the same images through
the ragged path, (b) half 224 x 224 and half 480 x 640 through the ragged path, (c) the same mixed images as two
uniform calls, one per size -- the only way to process them without the ragged path.
With `--left OUT.txt` it times left hands instead (`is_left`, the mirrored read): B = 128, 128 x 128 out, a dense 224 x 224
batch and a mixed-size one (64 x 224^2 + 64 x 480 x 640), recipe flags (the warp mirrors) and all ten flags (stage 0 mirrors);
per case six windows that ALTERNATE the batch without left hands and the same batch with every second sample left, so that the
window-to-window spread of either arm is the yardstick for the difference between them.
With `--device-draws OUT.txt` it times the parameter side on the device (TwoViewAugmenter(device_draws=True)) against the host
draws: B = 128, 128 x 128 out, the dense 224 x 224 batch and the mixed-size one, recipe flags, six windows per case that ALTERNATE
the two arms.  host_param_ms is what the host spends on the parameters of one batch: `sample_batch` in the host arm, issuing the
one draw launch (joints already on the device) in the device arm.  In the mixed-size case the device arm's windows sit in
whole-image slots under a grid of the largest image, the host arm's are packed: the rows of the two pixel launches show what
that costs.
Usage: python tools/augment_timing.py [out.json [ragged_out.json]] | --left OUT.txt | --device-draws OUT.txt"""
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from oracle import augment_oracle as A
from peclr_amd import RaggedImages, TwoViewAugmenter, _capi
from peclr_amd.augment import RECIPE_FLAGS

ALL_TEN = dict(RECIPE_FLAGS, sobel_filter=True, cut_out=True, gaussian_blur=True, gaussian_noise=True, color_drop=True)

DEV = torch.device("cuda:0")


def timed(calls, draw):
    """calls: the augmenter calls of one batch; draw: its host parameter draws alone.  Three warm-up batches, then the
    same measurement as main()'s rows."""
    for _ in range(3):
        calls()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        draw()
    host_ms = (time.perf_counter() - t0) / 5 * 1e3
    _capi.EVENT_LOG = {}
    t0 = time.perf_counter()
    for _ in range(10):
        calls()
    torch.cuda.synchronize()
    total_ms = (time.perf_counter() - t0) / 10 * 1e3
    ev = {k: round(sum(s.elapsed_time(e) for s, e, *_ in v) / 10 * 1e3, 1) for k, v in _capi.EVENT_LOG.items()}
    _capi.EVENT_LOG = None
    return {"host_param_ms": round(host_ms, 2), "kernel_us": ev, "kernel_total_us": round(sum(ev.values()), 1),
            "end_to_end_ms": round(total_ms, 2)}


def ragged_rows():
    b, size = 128, 128
    g = np.random.default_rng(0)
    small = [g.integers(0, 256, (224, 224, 3), dtype=np.uint8) for _ in range(b)]
    big = [g.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(b // 2)]

    def joints(sizes):
        return torch.from_numpy(np.stack([np.concatenate([g.normal((w / 2, h / 2 - 4), min(h, w) / 9, (21, 2)),
                                                          g.normal(0, 1, (21, 1))], 1) for h, w in sizes])).float()

    def aug():
        return TwoViewAugmenter(params={"resize_shape": [size, size]}, rng=random.Random(1))

    rows = []
    j224 = joints([(224, 224)] * b)
    uniform = torch.from_numpy(np.stack(small)).to(DEV)
    for rep in range(5):
        a = aug()
        rows.append(dict(row=f"uniform 224 (repeat {rep})", batch=b, out=size,
                         **timed(lambda: a(uniform, j224), lambda: a.sample_batch(j224, (224, 224)))))
    tot = [r["kernel_total_us"] for r in rows]
    e2e = [r["end_to_end_ms"] for r in rows]
    spread = {"row": "spread of the five uniform repeats", "kernel_total_us": [min(tot), max(tot)],
              "end_to_end_ms": [min(e2e), max(e2e)]}
    # (a) the same images, ragged path (the device buffer is built once, like `uniform` above)
    a, ragged = aug(), RaggedImages.from_list(small, DEV)
    rows.append(dict(row="(a) ragged path, 128 x 224^2", batch=b, out=size,
                     **timed(lambda: a(ragged, j224), lambda: a.sample_batch(j224, ragged.sizes))))
    # (b) half 224^2, half 480 x 640, interleaved, ragged path
    mixed = [im for pair in zip(small[:b // 2], big) for im in pair]
    sizes = [im.shape[:2] for im in mixed]
    jmix = joints(sizes)
    a, ragged = aug(), RaggedImages.from_list(mixed, DEV)
    rows.append(dict(row="(b) ragged path, 64 x 224^2 + 64 x 480x640", batch=b, out=size,
                     **timed(lambda: a(ragged, jmix), lambda: a.sample_batch(jmix, sizes))))
    # (c) the same images as two uniform calls, one per size
    a = aug()
    u_small, u_big = torch.from_numpy(np.stack(mixed[0::2])).to(DEV), torch.from_numpy(np.stack(mixed[1::2])).to(DEV)
    j_small, j_big = jmix[0::2].contiguous(), jmix[1::2].contiguous()
    rows.append(dict(row="(c) two uniform calls, 64 x 224^2 then 64 x 480x640", batch=b, out=size,
                     **timed(lambda: (a(u_small, j_small), a(u_big, j_big)),
                             lambda: (a.sample_batch(j_small, (224, 224)), a.sample_batch(j_big, (480, 640))))))
    rows.append(spread)
    for r in rows:
        print(r, flush=True)
    return rows


def left_rows(path):
    b, size, windows = 128, 128, 6
    g = np.random.default_rng(0)
    small = [g.integers(0, 256, (224, 224, 3), dtype=np.uint8) for _ in range(b)]
    big = [g.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(b // 2)]
    mixed = [im for pair in zip(small[:b // 2], big) for im in pair]
    half = [i % 4 < 2 for i in range(b)]      # every second PAIR: half of either size in the mixed batch
    lines = [f"is_left timing: B = {b}, out {size} x {size}, {windows} alternating windows per case (10 batches each after 3 warm-up "
             "batches); kernel_us = device-event time per batch, summed per launch name", ""]
    for flags_name, flags in (("recipe", None), ("all ten", ALL_TEN)):
        for case, images in (("dense 128 x 224^2", torch.from_numpy(np.stack(small)).to(DEV)),
                             ("mixed 64 x 224^2 + 64 x 480x640", RaggedImages.from_list(mixed, DEV))):
            sizes = images.sizes if isinstance(images, RaggedImages) else [(224, 224)] * b
            joints = torch.from_numpy(np.stack([np.concatenate([g.normal((w / 2, h / 2 - 4), min(h, w) / 9, (21, 2)),
                                                                g.normal(0, 1, (21, 1))], 1) for h, w in sizes])).float()
            arms = {"no left": [], "half left": []}
            for win in range(windows):
                arm = "half left" if win % 2 else "no left"
                is_left = half if win % 2 else None
                a = TwoViewAugmenter(flags, params={"resize_shape": [size, size]}, rng=random.Random(1), extended=flags is not None,
                                     np_rng=np.random.RandomState(1) if flags else None)
                r = timed(lambda: a(images, joints, is_left=is_left), lambda: a.sample_batch(joints, sizes, is_left))
                arms[arm].append(r)
                lines.append(f"{flags_name:8s} {case:34s} window {win} {arm:9s} kernel_us {r['kernel_us']} total {r['kernel_total_us']}"
                             f" end_to_end_ms {r['end_to_end_ms']} host_param_ms {r['host_param_ms']}")
                print(lines[-1], flush=True)
            for name in sorted({k for rs in arms.values() for r in rs for k in r["kernel_us"]}) + ["kernel_total_us"]:
                get = (lambda r: r["kernel_total_us"]) if name == "kernel_total_us" else (lambda r: r["kernel_us"].get(name, 0.0))
                no, yes = [get(r) for r in arms["no left"]], [get(r) for r in arms["half left"]]
                lines.append(f"  {name:32s} no left {min(no):8.1f} .. {max(no):8.1f}   half left {min(yes):8.1f} .. {max(yes):8.1f}   "
                             f"difference of the means {sum(yes) / len(yes) - sum(no) / len(no):+8.1f} us, spread within an arm "
                             f"{max(max(no) - min(no), max(yes) - min(yes)):.1f} us")
                print(lines[-1], flush=True)
            lines.append("")
    with open(path, "w") as f:
        f.write("\n".join(lines))


def device_draw_rows(path):
    b, size, windows = 128, 128, 6
    g = np.random.default_rng(0)
    small = [g.integers(0, 256, (224, 224, 3), dtype=np.uint8) for _ in range(b)]
    big = [g.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(b // 2)]
    mixed = [im for pair in zip(small[:b // 2], big) for im in pair]
    lines = [f"device draws timing: B = {b}, out {size} x {size}, recipe flags, {windows} alternating windows per case (10 batches each "
             "after 3 warm-up batches); kernel_us = device-event time per batch, summed per launch name", ""]
    for case, images in (("dense 128 x 224^2", torch.from_numpy(np.stack(small)).to(DEV)),
                         ("mixed 64 x 224^2 + 64 x 480x640", RaggedImages.from_list(mixed, DEV))):
        ragged = isinstance(images, RaggedImages)
        sizes = images.sizes if ragged else [(224, 224)] * b
        joints = torch.from_numpy(np.stack([np.concatenate([g.normal((w / 2, h / 2 - 4), min(h, w) / 9, (21, 2)),
                                                            g.normal(0, 1, (21, 1))], 1) for h, w in sizes])).float()
        joints_dev = joints.to(DEV)
        geom_dev = TwoViewAugmenter.ragged_slot_tables(sizes, images.offsets, images.data.numel())[0].to(DEV) if ragged else None
        arms = {"host draws": [], "device draws": []}
        for win in range(windows):
            if win % 2:
                arm, a = "device draws", TwoViewAugmenter(params={"resize_shape": [size, size]}, device_draws=True, draw_seed=1)
                r = timed(lambda: a(images, joints_dev), lambda: a.draw_batch(joints_dev, None if ragged else (224, 224), geom_dev))
                assert a.bad_windows() == 0
            else:
                arm, a = "host draws", TwoViewAugmenter(params={"resize_shape": [size, size]}, rng=random.Random(1))
                r = timed(lambda: a(images, joints), lambda: a.sample_batch(joints, sizes))
            arms[arm].append(r)
            lines.append(f"{case:34s} window {win} {arm:12s} kernel_us {r['kernel_us']} total {r['kernel_total_us']}"
                         f" end_to_end_ms {r['end_to_end_ms']} host_param_ms {r['host_param_ms']}")
            print(lines[-1], flush=True)
        names = sorted({k for rs in arms.values() for r in rs for k in r["kernel_us"]})
        for name in names + ["kernel_total_us", "host_param_ms", "end_to_end_ms"]:
            get = (lambda r: r["kernel_us"].get(name, 0.0)) if name in names else (lambda r: r[name])
            host, devc = [get(r) for r in arms["host draws"]], [get(r) for r in arms["device draws"]]
            unit = "ms" if name.endswith("_ms") else "us"
            lines.append(f"  {name:28s} host draws {min(host):9.2f} .. {max(host):9.2f}   device draws {min(devc):9.2f} .. {max(devc):9.2f}   "
                         f"difference of the means {sum(devc) / len(devc) - sum(host) / len(host):+9.2f} {unit}, spread within an arm "
                         f"{max(max(host) - min(host), max(devc) - min(devc)):.2f} {unit}")
            print(lines[-1], flush=True)
        e_host, e_dev = (sum(r["end_to_end_ms"] for r in arms[k]) / len(arms[k]) for k in ("host draws", "device draws"))
        lines.append(f"  end_to_end_ms, host draws / device draws: {e_host / e_dev:.1f} x   ({2 * b / e_host * 1e3:.0f} -> "
                     f"{2 * b / e_dev * 1e3:.0f} images/s per process)")
        print(lines[-1], flush=True)
        lines.append("")
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--left":
        return left_rows(sys.argv[2])
    if len(sys.argv) > 2 and sys.argv[1] == "--device-draws":
        return device_draw_rows(sys.argv[2])
    rows = []
    g = np.random.default_rng(0)
    for b, size, all_ten in ((128, 128, False), (128, 224, False), (512, 128, False), (128, 128, True)):
        images_np = g.integers(0, 256, (b, 224, 224, 3), dtype=np.uint8)
        images = torch.from_numpy(images_np).to(DEV)
        joints = torch.from_numpy(np.concatenate([g.normal((112, 108), 25, (b, 21, 2)), g.normal(0, 1, (b, 21, 1))], 2)).float()
        aug = TwoViewAugmenter(ALL_TEN if all_ten else None, params={"resize_shape": [size, size]}, rng=random.Random(1),
                               extended=all_ten, np_rng=np.random.RandomState(1) if all_ten else None)
        for _ in range(3):
            aug(images, joints)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            params, views = aug.sample_batch(joints, (224, 224))
        host_ms = (time.perf_counter() - t0) / 5 * 1e3
        _capi.EVENT_LOG = {}
        t0 = time.perf_counter()
        for _ in range(10):
            aug(images, joints)
        torch.cuda.synchronize()
        total_ms = (time.perf_counter() - t0) / 10 * 1e3
        ev = {k: round(sum(s.elapsed_time(e) for s, e, *_ in v) / 10 * 1e3, 1) for k, v in _capi.EVENT_LOG.items()}
        _capi.EVENT_LOG = None
        row = {"batch": b, "out": size, "flags": "all ten" if all_ten else "recipe", "host_param_ms": round(host_ms, 2),
               "kernel_us": ev, "kernel_total_us": round(sum(ev.values()), 1), "end_to_end_ms": round(total_ms, 2),
               "images_per_s": round(2 * b / total_ms * 1e3)}
        if not all_ten:
            # CPU restatement: one sample, both views (what one DataLoader worker does per item)
            rng = random.Random(1)
            t0 = time.perf_counter()
            n_cpu = 8
            for i in range(n_cpu):
                A.prepare_hybrid2_sample(images_np[i], joints[i].numpy(), aug.flags, aug.params, rng)
            cpu_ms = (time.perf_counter() - t0) / n_cpu * 1e3
            row.update(cpu_restatement_ms_per_sample=round(cpu_ms, 1), cpu_images_per_s_per_core=round(2 / cpu_ms * 1e3, 1))
        print(row, flush=True)
        rows.append(row)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(ragged_rows(), f, indent=1)


if __name__ == "__main__":
    main()
