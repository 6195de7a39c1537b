"""Fine-tuning the 2.5D hand-pose model on labelled hands: the module that composes the supervised pieces.

`SupervisedPose` is a `BaseModel` with the surface the reference's supervised model classes had (`training_step`,
`validation_step`, `configure_optimizers`, the epoch-end hooks; `BaseModel.training_epoch_end` monitors `loss_3d` for it):

    batch  = SupervisedAugmenter(...)(images_u8, K, joints3d)          # peclr_amd/supervised.py
    out    = RN25DwMLPref(batch["image"], batch["K"])                  # backbone on the in-tree kernels, head in 4 + 6 launches
    total, losses = PoseLoss(out["kp25d"], batch, z_root_calc=out["zroot"])     # 2 + 1 launches
    metrics = calculate_metrics on (kp25d, joints) and (kp3d, joints3D)          # 1 launch for both pairs

    model = SupervisedPose(supervised_config(batch_size=128, num_samples=N)).to("cuda").enable_hip()
    model.load_encoder("pretraining.ckpt")
    Trainer(max_epochs=E, hip_graph=True).fit(model, train_batches, val_batches)
    model.export("rn50_finetuned.pth")                                 # tools/pred_freihand.py --model_path loads it

Nothing in a step synchronises with the host, so `Trainer(hip_graph=True)` records forward, backward and the fused optimiser
as one hipGraph.  Single process only.  Precision is the trainer's: fp32, or bf16 / fp16 (16) with the precision split of
`FreiHANDPredictor` -- the backbone up to the pooled fp32 features under `torch.autocast` on the 16-bit convolution kernels,
head, losses, metrics and lifting in fp32 / float64 as before; fp16 adds the trainer's `DeviceLossScaler`, which decides a
skipped step inside the fused optimiser launch, so the 16-bit step is one hipGraph too.  `setup()` refuses anything else.
"""
from __future__ import annotations

import contextlib
import os
from typing import Dict, List, Optional

import torch
from torch import Tensor

from . import _capi
from . import bn2d as _bn2d
from .module import BaseModel
from .pose import FreiHANDPredictor, RN25DwMLPref
from .pose_loss import LOSS_NAMES, PoseLoss
from .pose_metrics import step_metrics
from .port import encoder_entries, get_latest_checkpoint
from .supervised import joints25d_to_3d

METRIC_NAMES = ("EPE_mean", "EPE_median", "EPE_mean_3d", "EPE_median_3d")
TRAIN_KEYS = LOSS_NAMES + tuple(f"{n}_train" for n in METRIC_NAMES) + ("loss",)
VAL_KEYS = tuple(f"{n}_val" for n in LOSS_NAMES + METRIC_NAMES) + ("loss",)
EVALUATE_KEYS = ("Mean_EPE_3D", "Median_EPE_3D", "AUC", "Mean_EPE_3D_procrustes", "Median_EPE_3D_procrustes", "auc_procrustes")
# encoder.features[i] of a pretraining checkpoint -> the torchvision name the pose model's backbone uses (encoder.py)
_FEATURES = {"0": "conv1", "1": "bn1", "4": "layer1", "5": "layer2", "6": "layer3", "7": "layer4"}
# the trainer's spellings of a precision -> ours; the autocast dtype of the 16-bit ones
_PRECISIONS = {"fp32": "fp32", 32: "fp32", "32": "fp32", "bf16": "bf16", "fp16": "fp16", 16: "fp16", "16": "fp16"}
_AUTOCAST = {"bf16": torch.bfloat16, "fp16": torch.float16}


class SupervisedPose(BaseModel):
    """config: `supervised_config()` -- backend_model ("rn50" / "rn152"), lr, optimizer ("adam"; "LARS" takes the inherited
    warm-up branch), opt_weight_decay, warmup_epochs, batch_size, num_of_mini_batch, num_samples, lr_max_epochs,
    loss_weights.  There is no `resnet_size`, so `BaseModel` builds no `encoder`: the network is `self.model`, an
    `RN25DwMLPref`, and the state_dict keys are "model." + the reference's `RN_25D_wMLPref` keys, in its order.

    evaluator: an optional `PoseEvaluator`; `validation_step` then also feeds it (`update_25d`) and `validation_epoch_end`
    adds the reference's evaluate() metrics to `validation_metrics_epoch` and resets it.

    fold_bn (16-bit precisions only; always off in fp32): `validation_step` applies the eval-mode BatchNorm layers of the
    bottleneck blocks in the convolution epilogues (`bn2d.fold_plan`), as `FreiHANDPredictor` does; None = its
    `FOLD_BN_DEFAULT`.

    precision: "fp32" until `setup()` has read the trainer's, then "fp32" | "bf16" | "fp16"."""

    def __init__(self, config, evaluator=None, fold_bn=None):
        super().__init__(config)
        self.model = RN25DwMLPref(config.backend_model)
        self.loss = PoseLoss(config.loss_weights)
        self.evaluator = evaluator
        self._fold_bn_arg = fold_bn
        self.precision = "fp32"

    @property
    def fold_bn(self) -> bool:
        """What `validation_step` folds at the present precision."""
        if self.precision == "fp32":
            return False
        return FreiHANDPredictor.FOLD_BN_DEFAULT if self._fold_bn_arg is None else bool(self._fold_bn_arg)

    # ---- paths
    def enable_hip(self) -> "SupervisedPose":
        """channels_last weights, the backbone and the evaluation head on the HIP kernels, and the train-mode head on its
        forward / backward kernels.  Call after .to(device); `training_step` refuses a HIP model without it."""
        self.model.to(memory_format=torch.channels_last)
        self.model.enable_hip().enable_hip_training()
        return self

    def _need_hip_kernels(self, what: str):
        """On a HIP device the step runs on the in-tree kernels or not at all (on the CPU `PoseLoss` raises its own error)."""
        m = self.model
        if m.backend_model.fc.weight.is_cuda and not (m.backend_model.bn1.hip and m.hip_training):
            raise _capi.PeclrHipError(f"SupervisedPose.{what}: the model is on a HIP device but its HIP kernels are off -- call "
                                      "enable_hip() after .to(device); there is no fallback to stock torch operators")

    def forward(self, img: Tensor, K: Optional[Tensor] = None) -> Dict[str, Tensor]:
        return self.model(img, K)

    # ---- steps
    def training_step(self, batch: Dict[str, Tensor], batch_idx: int) -> Dict[str, Tensor]:
        """One step on a `SupervisedAugmenter` batch.  Returns `self.train_metrics`, in this order: `loss_2d`, `loss_z`,
        `loss_z_unscaled`, `loss_3d` (cal_l1_loss, cal_3d_loss with the refined root depth `zroot`), `EPE_mean_train`,
        `EPE_median_train` (calculate_metrics on the 2.5D joints), `EPE_mean_3d_train`, `EPE_median_3d_train` (on the 3D
        joints), then `loss`, the weighted sum -- the only entry that carries a gradient.  No host synchronisation."""
        self._need_hip_kernels("training_step")
        out = self.model(batch["image"], batch["K"])
        # (on the CPU the stock forward has no refined depth to hand over, and `PoseLoss` refuses CPU tensors: "no CPU path")
        total, losses = self.loss(out["kp25d"], batch, z_root_calc=out["zroot"] if out["kp25d"].is_cuda else None)
        with torch.no_grad():
            metrics = step_metrics(out["kp25d"], batch["joints"], out["kp3d"], batch["joints3D"])
        self.train_metrics = {**{n: losses[n].detach() for n in LOSS_NAMES},
                              **{f"{n}_train": m for n, m in zip(METRIC_NAMES, metrics.unbind(0))}, "loss": total}
        self.plot_params = {"prediction": out["kp25d"].detach(), "ground_truth": batch["joints"], "input": batch["image"]}
        return self.train_metrics

    def validation_step(self, batch: Dict[str, Tensor], batch_idx: int) -> Dict[str, Tensor]:
        """Eval mode, no gradient: the one-launch evaluation head.  Returns the training keys with the `_val` suffix
        (`loss_2d_val` ... `EPE_median_3d_val`), then `loss`.  In a 16-bit run the backbone runs under the run's autocast, with
        eval BatchNorm folded into the convolution epilogues when `fold_bn` says so; `Trainer.fit` calls this outside its own
        autocast, so the module enters both itself.  In fp32 it enters neither: the launches are those of before.
        The 3D joints are lifted from the 2.5D prediction with the
        CLOSED-FORM root depth (`z_root_calc=None`), as the reference's evaluate() lifts them: validation `loss_3d_val` and
        the 3D metrics use that depth, while the training step uses the MLP-refined `zroot`."""
        self._need_hip_kernels("validation_step")
        if self.model.training:
            raise RuntimeError("SupervisedPose.validation_step runs in eval mode (call .eval() first): in train mode the forward "
                               "pass would update the BatchNorm running statistics")
        with torch.no_grad():
            with self._eval_precision():
                kp25d = self.model(batch["image"], batch["K"])["kp25d"].contiguous()
            total, losses = self.loss(kp25d, batch, z_root_calc=None)
            kp3d = joints25d_to_3d(kp25d, batch["scale"], batch["K"])
            metrics = step_metrics(kp25d, batch["joints"], kp3d, batch["joints3D"])
            if self.evaluator is not None:
                self.evaluator.update_25d(kp25d, batch["scale"], batch["K"], batch["joints3D"])
        self.plot_params = {"prediction": kp25d, "ground_truth": batch["joints"], "input": batch["image"]}
        return {**{f"{n}_val": losses[n] for n in LOSS_NAMES},
                **{f"{n}_val": m for n, m in zip(METRIC_NAMES, metrics.unbind(0))}, "loss": total}

    def _eval_precision(self):
        """Context of the validation forward: nothing in fp32; the autocast dtype and the fold switch of a 16-bit run."""
        if self.precision == "fp32":
            return contextlib.nullcontext()
        stack = contextlib.ExitStack()
        stack.enter_context(torch.autocast("cuda", dtype=_AUTOCAST[self.precision]))
        stack.enter_context(_bn2d.routing(fold_eval_bn=self.fold_bn))
        return stack

    def validation_epoch_end(self, outputs: List[dict]):
        """The epoch means of the step dicts and, with an evaluator, the metrics of evaluate() over everything it was fed
        this epoch (its one host synchronisation); the evaluator starts the next epoch empty."""
        super().validation_epoch_end(outputs)
        if self.evaluator is not None:
            scores = self.evaluator.compute()
            self.validation_metrics_epoch.update({k: scores[k] for k in EVALUATE_KEYS})
            self.evaluator.reset()

    # ---- trainer hooks
    def setup(self, stage: str):
        if self.trainer.world_size > 1:
            raise RuntimeError("SupervisedPose is single-process only: the trainer's data-parallel path reads the pretraining "
                               f"batch keys (world_size = {self.trainer.world_size})")
        asked = getattr(self.trainer, "precision", "fp32")
        precision = None if isinstance(asked, bool) or not isinstance(asked, (str, int)) else _PRECISIONS.get(asked)
        if precision is None:
            raise RuntimeError(f"SupervisedPose trains in fp32, bf16 or fp16 (16), the trainer asks for precision {asked!r}; "
                               "without the HIP kernels it trains in fp32 only")
        m = self.model
        if precision != "fp32" and not (m.backend_model.bn1.hip and m.hip_training):
            raise RuntimeError(f"the trainer asks for precision {asked!r}, but without the HIP kernels SupervisedPose trains in fp32 "
                               "only: the 16-bit step runs on the in-tree 16-bit convolution kernels and has no stock-torch arm -- "
                               "call .to(device).enable_hip() before Trainer.attach / fit")
        self.precision = precision
        super().setup(stage)

    # ---- weights in, weights out
    def load_encoder(self, path: str, checkpoint: str = "") -> "SupervisedPose":
        """Initialise `model.backend_model` from a PeCLR pretraining checkpoint: `path` is a checkpoint file (what
        `peclr_to_torchvision` takes) or an experiment whose newest / named `checkpoint` `get_latest_checkpoint` resolves, as
        `get_encoder_state_dict` does.
        The encoder's `features.{0,1,4,5,6,7}.*` entries become conv1, bn1, layer1..4; `fc` and the refinement MLP keep their
        initial values.  Unlike `peclr_to_torchvision`, which prints and stops, a checkpoint that does not fill every backbone
        tensor exactly (another ResNet size, a missing or an unknown entry) raises, before anything is copied."""
        state = encoder_entries(path if os.path.isfile(path) else get_latest_checkpoint(path, checkpoint))
        mapped, unexpected = {}, []
        for key, value in state.items():
            part, _, rest = key.partition(".")
            index, _, tail = rest.partition(".")
            if part == "features" and index in _FEATURES:
                mapped[f"{_FEATURES[index]}.{tail}"] = value
            elif part != "final_layer":                   # the pretraining encoder's unused Linear: not a backbone tensor
                unexpected.append(key)
        own = self.model.backend_model.state_dict()
        missing = [k for k in own if k not in mapped and not k.startswith("fc.")]
        unexpected += [k for k in mapped if k not in own]
        wrong = [k for k in mapped if k in own and tuple(mapped[k].shape) != tuple(own[k].shape)]
        if missing or unexpected or wrong:
            raise RuntimeError(f"load_encoder: {path} does not match the {self.model.backend_type} backbone: {len(missing)} missing "
                               f"{missing[:3]}, {len(unexpected)} unexpected {unexpected[:3]}, {len(wrong)} of another shape {wrong[:3]}")
        self.model.backend_model.load_state_dict(mapped, strict=False)
        return self

    def export(self, path: str) -> str:
        """Write the bare `RN_25D_wMLPref` weights in the format of the published `rn50_peclr_yt3d-fh_pt_fh_ft.pth`:
        {"state_dict": <the reference's keys, without the "model." prefix>} on the CPU.  `tools/pred_freihand.py
        --model_path` (which reads the backbone size from "rn50" / "rn152" in the file name) loads it unchanged."""
        state = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save({"state_dict": state}, path)
        return path
