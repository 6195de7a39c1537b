"""Host side of the fine-tuning module (peclr_amd/finetune.py): keys, weights in and out, the optimiser and its schedule, the
guards and the epoch-end hook.  No device."""
import math
import os
import types

import pytest
import torch
from torch.optim.lr_scheduler import CosineAnnealingLR

from peclr_amd import (Hybrid2Model, SupervisedPose, Trainer, hybrid2_config, save_checkpoint, supervised_config)
from peclr_amd.finetune import TRAIN_KEYS, VAL_KEYS
from peclr_amd.optim import LinearWarmupCosineAnnealingLR
from peclr_amd.pose import RN25DwMLPref


@pytest.fixture(scope="module")
def module():
    torch.manual_seed(3)
    return SupervisedPose(supervised_config(batch_size=8, num_samples=64))


def test_config_has_the_documented_keys_and_no_encoder(module):
    cfg = supervised_config()
    assert sorted(cfg) == sorted(["backend_model", "lr", "optimizer", "opt_weight_decay", "warmup_epochs", "batch_size", "num_of_mini_batch",
                                  "num_samples", "lr_max_epochs", "loss_weights"])
    assert cfg.optimizer == "adam" and cfg.backend_model == "rn50" and "resnet_size" not in cfg
    assert supervised_config(lr=3e-4, backend_model="rn152").lr == 3e-4
    assert not hasattr(module, "encoder") and isinstance(module.model, RN25DwMLPref)
    assert module.loss.weights == {"loss_2d": 1.0, "loss_z": 1.0, "loss_z_unscaled": 0.0, "loss_3d": 1.0}


def test_documented_key_orders():
    assert TRAIN_KEYS == ("loss_2d", "loss_z", "loss_z_unscaled", "loss_3d", "EPE_mean_train", "EPE_median_train", "EPE_mean_3d_train",
                          "EPE_median_3d_train", "loss")
    assert VAL_KEYS == ("loss_2d_val", "loss_z_val", "loss_z_unscaled_val", "loss_3d_val", "EPE_mean_val", "EPE_median_val",
                        "EPE_mean_3d_val", "EPE_median_3d_val", "loss")


def test_state_dict_keys_are_the_pose_models_under_one_prefix(module):
    assert list(module.state_dict()) == ["model." + k for k in RN25DwMLPref("rn50").state_dict()]


def test_export_round_trips_bit_for_bit(module, tmp_path):
    path = module.export(str(tmp_path / "out" / "rn50_finetuned.pth"))
    fresh = RN25DwMLPref("rn50")
    fresh.load_state_dict(torch.load(path, map_location="cpu")["state_dict"], strict=True)
    theirs, ours = fresh.state_dict(), module.model.state_dict()
    assert list(theirs) == list(ours)
    for k in ours:
        assert torch.equal(theirs[k], ours[k]) and theirs[k].dtype == ours[k].dtype, k


def test_load_encoder_fills_the_backbone_and_nothing_else(tmp_path):
    torch.manual_seed(4)
    pre = Hybrid2Model(hybrid2_config(resnet_size="50", pretrained=False, num_samples=64))
    with torch.no_grad():                                  # running statistics and counters that differ from a fresh model's
        for name, buf in pre.encoder.named_buffers():
            buf.copy_(torch.full_like(buf, 7) if buf.dtype == torch.int64 else torch.rand_like(buf) + 0.5)
    ckpt = str(tmp_path / "epoch=3.ckpt")
    save_checkpoint(ckpt, pre, epoch=3)
    torch.manual_seed(5)
    m = SupervisedPose(supervised_config())
    before = {k: v.clone() for k, v in m.model.state_dict().items()}
    assert m.load_encoder(ckpt) is m
    src = pre.encoder.state_dict()
    names = {"0": "conv1", "1": "bn1", "4": "layer1", "5": "layer2", "6": "layer3", "7": "layer4"}
    filled = set()
    for key, value in src.items():
        if key.startswith("features."):
            _, index, tail = key.split(".", 2)
            dst = f"backend_model.{names[index]}.{tail}"
            assert torch.equal(m.model.state_dict()[dst], value), dst
            filled.add(dst)
    after = m.model.state_dict()
    rest = set(after) - filled
    assert rest == {k for k in after if k.startswith(("backend_model.fc.", "zroot_ref."))}
    for k in rest:
        assert torch.equal(after[k], before[k]), k
    # through an experiment's checkpoint directory, as get_encoder_state_dict resolves it
    exp = tmp_path / "exp" / "checkpoints"
    os.makedirs(exp)
    save_checkpoint(str(exp / "epoch=1.ckpt"), pre, epoch=1)
    m2 = SupervisedPose(supervised_config()).load_encoder(str(tmp_path / "exp"))
    assert torch.equal(m2.model.backend_model.conv1.weight, pre.encoder.features[0].weight)


def test_load_encoder_raises_on_another_resnet(tmp_path):
    small = Hybrid2Model(hybrid2_config(resnet_size="18", projection_head_input_dim=512, pretrained=False, num_samples=64))
    ckpt = str(tmp_path / "rn18.ckpt")
    save_checkpoint(ckpt, small)
    m = SupervisedPose(supervised_config())
    before = {k: v.clone() for k, v in m.model.state_dict().items()}
    with pytest.raises(RuntimeError, match="does not match the rn50 backbone"):
        m.load_encoder(ckpt)
    for k, v in m.model.state_dict().items():
        assert torch.equal(v, before[k]), k               # nothing was copied
    state = torch.load(ckpt, map_location="cpu")
    state["state_dict"]["encoder.extra.weight"] = torch.zeros(1)
    torch.save(state, ckpt)
    with pytest.raises(RuntimeError, match="unexpected"):
        m.load_encoder(ckpt)


def _attached(accum=1, epochs=5, **cfg):
    m = SupervisedPose(supervised_config(batch_size=8, num_samples=80, num_of_mini_batch=accum, **cfg))
    tr = Trainer(max_epochs=epochs, accumulate_grad_batches=accum).attach(m)
    return m, tr


def test_optimiser_groups_follow_the_substring_rule():
    m, tr = _attached()
    groups = tr.optimizer.param_groups
    assert len(groups) == 2 and groups[0]["weight_decay"] == m.config.opt_weight_decay and groups[1]["weight_decay"] == 0.0
    name_of = {id(p): n for n, p in m.named_parameters()}
    decayed = [name_of[id(p)] for p in groups[0]["params"]]
    plain = [name_of[id(p)] for p in groups[1]["params"]]
    assert sorted(decayed + plain) == sorted(name_of.values())
    assert all(("bias" in n or "bn" in n) for n in plain) and not any(("bias" in n or "bn" in n) for n in decayed)
    # the substring rule, not the module type: BatchNorm weights whose name has no "bn" stay decayed
    for n in ("model.zroot_ref.zroot_ref.1.weight", "model.zroot_ref.zroot_ref.4.weight", "model.backend_model.layer1.0.downsample.1.weight",
              "model.backend_model.conv1.weight", "model.backend_model.fc.weight"):
        assert n in decayed, n
    for n in ("model.backend_model.bn1.weight", "model.backend_model.layer1.0.bn3.weight", "model.zroot_ref.zroot_ref.1.bias",
              "model.backend_model.fc.bias"):
        assert n in plain, n


@pytest.mark.parametrize("accum", [1, 2])
def test_learning_rate_and_cosine_horizon(accum):
    m, tr = _attached(accum=accum, epochs=5, lr=2e-4)
    assert m.train_iters_per_epoch == 10
    assert isinstance(tr.scheduler, CosineAnnealingLR)
    assert tr.scheduler.base_lrs == [pytest.approx(2e-4 * math.sqrt(8 * accum), rel=1e-15)] * 2
    assert tr.scheduler.T_max == (5 * 10) // accum
    m, tr = _attached(accum=accum, epochs=5, lr_max_epochs=7)
    assert tr.scheduler.T_max == (7 * 10) // accum


def test_lars_gives_the_warm_up_schedule():
    m, tr = _attached(epochs=5, optimizer="LARS", warmup_epochs=2)
    assert isinstance(tr.scheduler, LinearWarmupCosineAnnealingLR)
    assert tr.scheduler.warmup_epochs == 20 and tr.scheduler.max_epochs == 50
    assert tr.optimizer.param_groups[0]["lr"] == 0.0       # warm-up starts at 0


def test_world_size_and_precision_guards():
    m = SupervisedPose(supervised_config(batch_size=8, num_samples=64))
    m.trainer = types.SimpleNamespace(world_size=2, precision="fp32", max_epochs=1)
    with pytest.raises(RuntimeError, match="single-process"):
        m.setup("fit")
    for precision in ("bf16", 16):
        with pytest.raises(RuntimeError, match="fp32 only"):
            Trainer(precision=precision).attach(SupervisedPose(supervised_config(batch_size=8, num_samples=64)))
    m.trainer = types.SimpleNamespace(world_size=1, precision=32, max_epochs=1)       # Lightning's spelling of fp32
    m.setup("fit")
    assert m.train_iters_per_epoch == 8
    with pytest.raises(RuntimeError, match="no peclr_amd.resnet blocks"):
        Trainer(activation_checkpointing=True).attach(SupervisedPose(supervised_config(batch_size=8, num_samples=64)))


def test_training_epoch_end_monitors_loss_3d(module):
    outs = [{k: torch.tensor(float(i + j)) for j, k in enumerate(TRAIN_KEYS)} for i in range(3)]
    module.training_epoch_end(outs)
    assert list(module.train_metrics_epoch) == list(TRAIN_KEYS)
    assert float(module.logged["checkpoint_saving_loss"]) == float(module.train_metrics_epoch["loss_3d"]) == 1.0 + 3.0
    assert float(module.train_metrics_epoch["loss"]) == 1.0 + 8.0


def test_cpu_module_has_no_training_path():
    from peclr_amd import _capi

    torch.manual_seed(6)
    m = SupervisedPose(supervised_config(batch_size=2, num_samples=8)).train()
    b = 2
    batch = {"image": torch.randn(b, 3, 64, 64), "K": torch.tensor([[200.0, 0, 32], [0, 200.0, 32], [0, 0, 1]]).repeat(b, 1, 1),
             "joints": torch.randn(b, 21, 3), "joints3D": torch.randn(b, 21, 3), "scale": torch.ones(b),
             "joints_valid": torch.ones(b, 21, 1)}
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        m.training_step(batch, 0)
    with pytest.raises(_capi.PeclrHipError, match="HIP device"):
        m.model.enable_hip_training()
