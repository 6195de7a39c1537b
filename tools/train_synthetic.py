#!/usr/bin/env python
"""End-to-end functional run: uint8 source images + 2.5D joints -> GPU two-view augmentation -> Hybrid2Model
(ResNet-18, crop+rotate alignment) -> NT-Xent -> LARS(Adam), through Trainer.fit with hipGraph replay.
The "dataset" is a fixed set of structured synthetic images, so instance discrimination is learnable and
the loss must fall.  --mixed-sizes: every second image is a 240 x 320 one, so that each batch mixes sizes and fit() runs
from the augmenter's ragged path (`RaggedImages`).  --left-frac F: that share of the images (chosen once, seeded) is marked as
left hands, so that every batch mixes mirrored and plain reads (`is_left`).  --device-draws: the augmentation parameters are drawn
on the device (TwoViewAugmenter(device_draws=True)); joints and `is_left` then live there too and no batch reads them on the host.
Usage: python tools/train_synthetic.py [--mixed-sizes] [--left-frac F] [--device-draws] [out.json]"""
import json
import os
import random
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
warnings.simplefilter("ignore")
import numpy as np
import torch

from peclr_amd import Hybrid2Model, RaggedImages, Trainer, TwoViewAugmenter, hybrid2_config
from peclr_amd.bn2d import enable_hip_batchnorm

DEV = torch.device("cuda:0")
N_IMAGES, PAIRS, EPOCHS, SIZE = 512, 64, 12, 128


def make_dataset(mixed=False):
    g = np.random.default_rng(0)
    imgs, centres = [], []
    for i in range(N_IMAGES):
        h, w = (240, 320) if mixed and i % 2 else (224, 224)
        yy, xx = np.mgrid[0:h, 0:w]
        centres.append((w / 2, h / 2 - 4))
        f = g.uniform(5, 40, 3)
        ph = g.uniform(0, 6.28, 3)
        base = np.stack([127 + 100 * np.sin(xx / f[0] + ph[0]), 127 + 100 * np.cos(yy / f[1] + ph[1]),
                         127 + 100 * np.sin((xx + yy) / f[2] + ph[2])], axis=2)
        imgs.append(np.clip(base + g.normal(0, 10, base.shape), 0, 255).astype(np.uint8))
    joints = np.concatenate([g.normal(np.array(centres)[:, None], 25, (N_IMAGES, 21, 2)), g.normal(0, 1, (N_IMAGES, 21, 1))], axis=2)
    if mixed:  # a list of device tensors: a batch is packed on the device
        return [torch.from_numpy(im).to(DEV) for im in imgs], torch.from_numpy(joints).float()
    return torch.from_numpy(np.stack(imgs)).to(DEV), torch.from_numpy(joints).float()


def main():
    args = [a for a in sys.argv[1:] if a not in ("--mixed-sizes", "--device-draws")]
    mixed, device_draws = "--mixed-sizes" in sys.argv[1:], "--device-draws" in sys.argv[1:]
    left_frac = 0.0
    if "--left-frac" in args:
        at = args.index("--left-frac")
        left_frac = float(args[at + 1])
        del args[at:at + 2]
    images, joints = make_dataset(mixed)
    is_left = torch.from_numpy(np.random.default_rng(2).random(N_IMAGES) < left_frac)
    cfg = hybrid2_config(resnet_size="18", projection_head_input_dim=512, augmentation=["crop", "rotate"],
                         batch_size=PAIRS, num_samples=N_IMAGES, warmup_epochs=2, pretrained=False)
    torch.manual_seed(0)
    model = Hybrid2Model(cfg).to(DEV).train()
    model.encoder = model.encoder.to(memory_format=torch.channels_last)
    enable_hip_batchnorm(model.encoder)
    if device_draws:
        aug = TwoViewAugmenter(params={"resize_shape": [SIZE, SIZE]}, device_draws=True, draw_seed=0)
        joints, is_left = joints.to(DEV), is_left.to(DEV)
    else:
        aug = TwoViewAugmenter(params={"resize_shape": [SIZE, SIZE]}, rng=random.Random(0))
    order = random.Random(1)

    def batches(epoch):
        idx = list(range(N_IMAGES))
        order.shuffle(idx)
        for s in range(0, N_IMAGES, PAIRS):
            sel = torch.tensor(idx[s:s + PAIRS])
            rows = sel.to(DEV) if device_draws else sel
            left = {"is_left": is_left[rows]} if left_frac > 0 else {}
            if mixed:
                yield aug(RaggedImages.from_list([images[i] for i in sel.tolist()], DEV), joints[rows], **left)
            else:
                yield aug(images[sel.to(DEV)], joints[rows], **left)

    curve = []
    orig = model.training_epoch_end

    def epoch_end(outputs):
        orig(outputs)
        curve.append(round(float(model.train_metrics_epoch["loss"]), 4))
        print(f"epoch {len(curve) - 1}: mean loss {curve[-1]}", flush=True)

    model.training_epoch_end = epoch_end
    tr = Trainer(max_epochs=EPOCHS, hip_graph=True)
    t0 = time.perf_counter()
    tr.fit(model, batches)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"device_draws": device_draws, "empty_windows": aug.bad_windows() if device_draws else 0,
           "last_over_first_epoch_mean_loss": round(curve[-1] / curve[0], 3), "mixed_sizes": mixed, "left_frac": left_frac, "left_images": int(is_left.sum()), "epochs": EPOCHS, "steps": tr.global_step, "pairs_per_step": PAIRS, "seconds": round(dt, 1),
           "images_per_s_incl_augmentation_and_capture": round(2 * PAIRS * tr.global_step / dt), "epoch_mean_loss": curve}
    print(json.dumps(out))
    assert curve[-1] < 0.8 * curve[0], "the loss did not fall"
    if args:
        with open(args[0], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
