#!/usr/bin/env python
"""End-to-end functional run of supervised fine-tuning: uint8 images + camera matrices + 3D joints -> `SupervisedAugmenter`
(crop and resize; --augment full adds rotation and colour jitter) -> `SupervisedPose` (ResNet-50, randomly initialised) -> the four losses and the step
metrics -> Adam under the cosine schedule, through `Trainer.fit` with hipGraph replay and a validation pass per epoch.

The "dataset" is a fixed set of synthetic hands drawn the way tests/test_supervised_gpu.py draws them (`hands`); each image
shows its hand -- one coloured blob per joint on a noisy background -- so the pose is learnable and `loss_3d` must fall: the
run asserts the criterion of tools/train_synthetic.py, last epoch's mean below 0.8 x the first's.  It is a functional run of the
loop, not a training recipe: a randomly initialised ResNet-50 memorises 64 hands in 200 steps and does not generalise, so the
validation pass exercises `validation_step` / `PoseEvaluator` and its figures mean nothing more.

--stock runs the SAME model, seed, data and optimiser without `enable_hip*` (tools/stock_pose_step.py: stock torch operators,
eagerly -- the stock step's `K.inverse()` cannot be captured); the learning rate and epoch count are chosen so that this arm
meets the criterion too.  --precision bf16 | fp16 runs either arm in 16 bits: the HIP arm with the backbone under autocast on the
16-bit convolution kernels (fp16: the `DeviceLossScaler` inside the one graph), the stock arm under torch's autocast with
`torch.amp.GradScaler`; every arm must end below its first epoch's loss_3d (fp32: below 0.8 x, as before).
Usage: python tools/finetune_synthetic.py [--stock] [--precision fp32|bf16|fp16] [--images N] [--epochs E] [--lr LR]
[--augment full|plain] [out.json]  (out.json: the run is stored under its arm's name -- "hip" / "stock", with "_bf16" / "_fp16" in
16 bits -- next to what the file already holds; plain: crop and resize only)."""
import argparse
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

from peclr_amd import PoseEvaluator, SupervisedAugmenter, SupervisedPose, Trainer, supervised_config
from peclr_amd.finetune import EVALUATE_KEYS

DEV = torch.device("cuda:0")
N_VAL, BATCH, SIZE = 64, 32, 128
# the defaults of --images, --epochs, --lr, --augment: two batches an epoch, few enough hands to memorise in 200 steps, and a learning
# rate (2e-4 x sqrt(32) at the optimiser) at which the stock arm ends at 0.48 of its first epoch's loss_3d -- well inside the 0.8 asserted
N_TRAIN, EPOCHS, LR, AUGMENT = 64, 100, 2e-4, "plain"
HW, FOCAL = (224, 224), 480.0


def hands(n, seed):
    """n synthetic hands -> (K [n,3,3], joints3D [n,21,3]) float32."""
    g = np.random.default_rng(seed)
    k = np.array([[FOCAL, 0, HW[1] / 2], [0, FOCAL, HW[0] / 2], [0, 0, 1]], dtype=np.float32)
    out = []
    for _ in range(n):
        z = 0.6 + 0.05 * g.standard_normal(21)
        u = g.uniform(0.35, 0.65) * HW[1] + min(HW) / 9 * g.standard_normal(21)
        v = g.uniform(0.35, 0.65) * HW[0] + min(HW) / 9 * g.standard_normal(21)
        out.append(np.stack([(u - k[0, 2]) * z / FOCAL, (v - k[1, 2]) * z / FOCAL, z], axis=1))
    return np.repeat(k[None], n, 0), np.array(out, dtype=np.float32)


def make_dataset(n, seed):
    """Images that show their labels: a blob per joint (its colour names the joint, its size the depth) over noise."""
    k, j3d = hands(n, seed)
    g = np.random.default_rng(seed + 1)
    yy, xx = np.mgrid[0:HW[0], 0:HW[1]].astype(np.float32)
    colours = 255 * np.stack([0.5 + 0.5 * np.sin(np.arange(21) * f + p) for f, p in ((0.9, 0.0), (1.7, 1.0), (2.9, 2.0))], axis=1)
    images = np.empty((n, HW[0], HW[1], 3), dtype=np.uint8)
    for i in range(n):
        u = j3d[i, :, 0] / j3d[i, :, 2] * FOCAL + k[i, 0, 2]
        v = j3d[i, :, 1] / j3d[i, :, 2] * FOCAL + k[i, 1, 2]
        radius = 3.0 * 0.6 / j3d[i, :, 2]
        blobs = np.exp(-((xx[None] - u[:, None, None]) ** 2 + (yy[None] - v[:, None, None]) ** 2) / (2 * radius[:, None, None] ** 2))
        top = blobs.max(0)
        picture = np.einsum("jhw,jc->hwc", blobs / np.maximum(blobs.sum(0), 1e-6), colours) * top[..., None]
        images[i] = np.clip(picture + (1 - top[..., None]) * g.normal(60, 12, (HW[0], HW[1], 3)), 0, 255).astype(np.uint8)
    return torch.from_numpy(images).to(DEV), torch.from_numpy(k), torch.from_numpy(j3d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stock", action="store_true")
    ap.add_argument("--precision", choices=("fp32", "bf16", "fp16"), default="fp32")
    ap.add_argument("--images", type=int, default=N_TRAIN)
    ap.add_argument("--epochs", type=int, default=EPOCHS)
    ap.add_argument("--lr", type=float, default=LR)
    ap.add_argument("--augment", choices=("full", "plain"), default=AUGMENT)
    ap.add_argument("--left-frac", type=float, default=0.0,
                    help="share of the training images marked as left hands (is_left: mirrored read, mirrored-camera labels)")
    ap.add_argument("out", nargs="?")
    opt = ap.parse_args()
    stock, args = opt.stock, [opt.out] if opt.out else []
    n_train, epochs, lr = opt.images, opt.epochs, opt.lr
    images, K, j3d = make_dataset(n_train, 0)
    v_images, v_K, v_j3d = make_dataset(N_VAL, 100)
    cfg = supervised_config(batch_size=BATCH, num_samples=n_train, lr=lr)
    evaluator = PoseEvaluator(capacity=N_VAL)
    torch.manual_seed(0)
    if stock:
        from stock_pose_step import StockPose, use_torch_grad_scaler

        model = StockPose(cfg, evaluator=evaluator).to(DEV).to(memory_format=torch.channels_last).train()
    else:
        model = SupervisedPose(cfg, evaluator=evaluator).to(DEV).train().enable_hip()
    params = {"resize_shape": [SIZE, SIZE]}
    flags = {"color_jitter": True, "rotate": True, "crop": True, "resize": True} if opt.augment == "full" else {"crop": True, "resize": True}
    aug = SupervisedAugmenter(flags, params, rng=random.Random(0))
    val_aug = SupervisedAugmenter({"crop": True, "resize": True}, params, rng=random.Random(2))
    order = random.Random(1)
    is_left = torch.from_numpy(np.random.default_rng(3).random(n_train) < opt.left_frac)

    def batches(epoch):
        idx = list(range(n_train))
        order.shuffle(idx)
        for s in range(0, n_train, BATCH):
            sel = torch.tensor(idx[s:s + BATCH])
            left = {"is_left": is_left[sel]} if opt.left_frac > 0 else {}
            yield aug(images[sel.to(DEV)], K[sel], j3d[sel], **left)

    def val_batches(epoch):
        for s in range(0, N_VAL, BATCH):
            yield val_aug(v_images[s:s + BATCH], v_K[s:s + BATCH], v_j3d[s:s + BATCH])

    curve, val_curve = [], []
    train_end, val_end = model.training_epoch_end, model.validation_epoch_end

    def epoch_end(outputs):
        train_end(outputs)
        curve.append(round(float(model.train_metrics_epoch["loss_3d"]), 4))
        print(f"epoch {len(curve) - 1}: mean loss_3d {curve[-1]}, mean loss {float(model.train_metrics_epoch['loss']):.4f}", flush=True)

    def validation_end(outputs):
        val_end(outputs)
        val_curve.append(round(float(model.validation_metrics_epoch["loss_3d_val"]), 4))

    model.training_epoch_end, model.validation_epoch_end = epoch_end, validation_end
    tr = Trainer(max_epochs=epochs, hip_graph=not stock, precision=opt.precision).attach(model)
    if stock:
        use_torch_grad_scaler(tr)
    t0 = time.perf_counter()
    tr.fit(model, batches, val_batches)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    final = {k: round(float(model.validation_metrics_epoch[k]), 5) for k in EVALUATE_KEYS}
    half = opt.precision != "fp32"
    arm = ("stock torch operators, eager" + (f", torch.autocast {opt.precision}" + (" + torch.amp.GradScaler" if opt.precision == "fp16" else "")
                                             if half else "")) if stock else \
        ("HIP kernels, one hipGraph per step" + (f", backbone under {opt.precision} autocast" + (" + DeviceLossScaler" if opt.precision == "fp16" else "")
                                                 if half else ""))
    ratio = round(curve[-1] / curve[0], 3)
    out = {"arm": arm, "precision": opt.precision, "last_over_first_epoch_mean_loss_3d": ratio, "backbone": "rn50", "epochs": epochs,
           "steps": tr.global_step, "batch": BATCH, "crop": SIZE, "lr": lr, "train_images": n_train, "augment": opt.augment, "left_frac": opt.left_frac, "seconds": round(dt, 1),
           "images_per_s_incl_augmentation_validation_and_capture": round(BATCH * tr.global_step / dt),
           "epoch_mean_loss_3d": curve, "epoch_mean_loss_3d_val": val_curve, "evaluate": final}
    print(json.dumps(out))
    if args:
        doc = {}
        if os.path.exists(args[0]):
            with open(args[0]) as f:
                doc = json.load(f)
        if tr._scaler is not None:
            out["final_loss_scale"] = float(tr._scaler.get_scale())
        doc[("stock" if stock else "hip") + (f"_{opt.precision}" if half else "")] = out
        with open(args[0], "w") as f:
            json.dump(doc, f, indent=1)
    assert curve[-1] < (1.0 if half else 0.8) * curve[0], "loss_3d did not fall"


if __name__ == "__main__":
    main()
