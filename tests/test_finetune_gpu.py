"""The fine-tuning module on the device (peclr_amd/finetune.py): one step against a float64 run of the same weights, the whole
step as one hipGraph against the eager loop, `Trainer.fit` end to end, learning, and the guards.

Sizes: those of test_pose_train_gpu.py::test_one_supervised_step_of_the_whole_model -- rn50, B = 8, 64 x 64 crops, every
convolution routed to the in-tree kernels (`bn2d.routing(force=True)`), so that every launch of a step has a fixed order.
Everything runs on one side stream, as `Trainer.fit` runs a graph-mode loop.

The bound of the one-step comparison is the project's calibration rule for whole-network comparisons: for each of the nine
values of a step, e = |value - gold64| / |gold64| against the float64 CPU run of the same weights on the stock path, and
e(HIP) <= max(6 x e(stock fp32 on the device), 1e-5) -- the stock path's own fp32 error, measured here, and the head tests' floor.
The `parity` lines this module prints are profiles/pose_finetune_parity.txt.
"""
import copy
import os
import random

import numpy as np
import pytest
import torch

from tests import pose_loss_ref, pose_metrics_ref
from tests.test_supervised_gpu import hands

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, HW = 8, (64, 64)
FLOOR, C = 1e-5, 6.0
SEQ = "model.zroot_ref.zroot_ref."
LEARN_STEPS, LEARN_LR = 30, 1e-3


def make_batches(n, seed, hw=HW):
    """n synthetic hands through `SupervisedAugmenter` (resize only: the augmentation flags are off) in batches of B."""
    from peclr_amd import SupervisedAugmenter

    k, j3d = hands(n, seed, hw, focal=200.0 * hw[0] / HW[0])
    images = torch.randint(0, 256, (n, hw[0], hw[1], 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(DEV)
    aug = SupervisedAugmenter({"resize": True}, {"resize_shape": list(hw)}, rng=random.Random(seed))
    return [aug(images[at:at + B], torch.from_numpy(k[at:at + B]), torch.from_numpy(j3d[at:at + B])) for at in range(0, n, B)]


def new_module(seed=5, evaluator=None, hip=True, **cfg):
    from peclr_amd import SupervisedPose, supervised_config

    torch.manual_seed(seed)
    m = SupervisedPose(supervised_config(batch_size=B, **cfg), evaluator=evaluator).to(DEV).train()
    return m.enable_hip() if hip else m.to(memory_format=torch.channels_last)      # (the fused optimiser wants the gradients' layout)


@pytest.fixture(autouse=True)
def forced_routing_on_a_side_stream():
    from peclr_amd import bn2d

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with bn2d.routing(force=True), torch.cuda.stream(side):
        yield
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    bn2d.end_backward()


# ------------------------------------------------------------------ the stock composition (any device, any dtype)
def stock_values(model, batch, weights):
    """One step of the stock path: the model's torch forward, the losses of tests/pose_loss_ref.py with the refined root depth
    (kp3d's wrist depth: zrel[0] = 0 and the ray's third component is 1) and calculate_metrics' formula -> the nine values."""
    out = model(batch["image"], batch["K"])
    zroot = out["kp3d"][:, 0, 2]
    losses = pose_loss_ref.losses(out["kp25d"], batch["joints"], batch["joints3D"], batch["scale"], batch["K"], batch["joints_valid"], zroot)
    values = dict(zip(pose_loss_ref.LOSS_NAMES, losses.unbind(0)))
    for name, (p, t) in (("", (out["kp25d"], batch["joints"])), ("_3d", (out["kp3d"], batch["joints3D"]))):
        d = ((p.detach() - t) ** 2).sum(2).sqrt()
        values[f"EPE_mean{name}_train"], values[f"EPE_median{name}_train"] = d.mean(), d.median()
    values["loss"] = sum(w * values[n] for n, w in weights.items() if w != 0.0)
    return values, out


def stock_module(**cfg):
    """The stock arm: the same module, same seed, with `training_step` on the stock composition (no HIP kernel in it)."""
    from peclr_amd import SupervisedPose

    class StockPose(SupervisedPose):
        def training_step(self, batch, batch_idx):
            values, _ = stock_values(self.model, batch, self.loss.weights)
            return {k: (v if k == "loss" else v.detach()) for k, v in values.items()}

    m = new_module(hip=False, **cfg)
    m.__class__ = StockPose
    return m


# ------------------------------------------------------------------ 1. one step against float64
def test_one_step_against_float64():
    from peclr_amd.finetune import TRAIN_KEYS

    batch = make_batches(B, 31)[0]
    m = new_module(num_samples=64)
    stock32 = copy.deepcopy(m.model).enable_hip(False).enable_hip_training(False)
    gold_model = copy.deepcopy(stock32).cpu().double()
    assert not stock32.backend_model.bn1.hip and stock32.training and gold_model.training
    out = m.training_step(batch, 0)
    assert tuple(out) == TRAIN_KEYS and out is m.train_metrics
    assert [k for k, v in out.items() if v.requires_grad] == ["loss"]
    assert sorted(m.plot_params) == ["ground_truth", "input", "prediction"]
    out["loss"].backward()
    with torch.no_grad():
        s32, _ = stock_values(stock32, batch, m.loss.weights)
        batch64 = {k: v.detach().cpu().double() for k, v in batch.items()}
        g64, out64 = stock_values(gold_model, batch64, m.loss.weights)
    torch.cuda.synchronize()
    # the float64 metrics: the NumPy restatement on the float64 run's outputs
    for name, (p, t) in (("", (out64["kp25d"], batch64["joints"])), ("_3d", (out64["kp3d"], batch64["joints3D"]))):
        mean, median = pose_metrics_ref.metrics64(p.numpy(), t.numpy())
        for key, value in ((f"EPE_mean{name}_train", mean), (f"EPE_median{name}_train", median)):
            assert abs(value - float(g64[key])) <= 1e-12 * value           # (torch's float64 composition agrees with it)
            g64[key] = value
    worst = 0.0
    for key in TRAIN_KEYS:
        gold = float(g64[key])
        if gold == 0.0:                      # (a loss whose weight the test does not use)
            assert float(out[key]) == 0.0
            continue
        e_dev, e_stock = abs(float(out[key]) - gold) / abs(gold), abs(float(s32[key]) - gold) / abs(gold)
        print(f"parity one step {key}: gold64 = {gold:.9g} e_hip = {e_dev:.3e} e_stock32 = {e_stock:.3e} "
              f"e_hip / max(6 e_stock32, 1e-5) = {e_dev / max(C * e_stock, FLOOR):.3f}")
        worst = max(worst, e_dev / max(C * e_stock, FLOOR))
    print(f"parity one step: worst e_hip / bound = {worst:.3f}")
    assert worst <= 1.0
    for name, p in m.named_parameters():
        g = p.grad
        assert g is not None and torch.isfinite(g).all(), name
        if name in (SEQ + "0.bias", SEQ + "3.bias"):          # in front of a train-mode BatchNorm: mathematically 0
            continue
        if name.startswith("model.backend_model.fc."):
            assert (g[[2, 63]] == 0).all() and (g[[i for i in range(64) if i not in (2, 63)]] != 0).any(), name
        else:
            assert (g != 0).any(), name


# ------------------------------------------------------------------ 2. / 3. the step as one hipGraph
STEPS, WARMUP = 9, 3


def _nbt(m):
    s = m.model.zroot_ref.zroot_ref
    return [int(s[1].num_batches_tracked), int(s[4].num_batches_tracked)]


def _graph_run(base, batch):
    """capture_step_graph(warmup=3) + 5 replays on a copy of `base` -> what the tests below look at."""
    from peclr_amd import Trainer

    m = copy.deepcopy(base)
    tr = Trainer(max_epochs=10).attach(m)
    tr.zero_grad()
    tr.capture_step_graph(batch, warmup=WARMUP)
    s = m.model.zroot_ref.zroot_ref
    nbt, means, losses = [_nbt(m)], [s[1].running_mean.clone()], []
    for _ in range(STEPS - WARMUP - 1):
        losses.append(tr.replay_step()["loss"].clone())
        nbt.append(_nbt(m))
        means.append(s[1].running_mean.clone())
    torch.cuda.synchronize()
    run = {"losses": torch.stack(losses), "params": [p.detach().clone() for p in m.parameters()], "nbt": nbt, "means": means,
           "buffers": [b.clone() for b in s.buffers()], "global_step": tr.global_step, "lr": tr.optimizer.param_groups[0]["lr"]}
    tr.close()
    return run


@pytest.fixture(scope="module")
def runs():
    """Nine steps on one fixed batch: the eager loop, and two independent graph-mode runs from the same weights."""
    from peclr_amd import Trainer, bn2d

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    miopen, conv_wgrad = [], bn2d._conv_wgrad
    bn2d._conv_wgrad = lambda gy, x, *a, **k: (miopen.append(tuple(x.shape)), conv_wgrad(gy, x, *a, **k))[1]
    with bn2d.routing(force=True), torch.cuda.stream(side):
        batch = make_batches(B, 41)[0]
        base = new_module(seed=11, num_samples=64)
        eager_m = copy.deepcopy(base)
        tr = Trainer(max_epochs=10).attach(eager_m)
        tr.zero_grad()
        eager = [float(tr.training_micro_step(batch, i)["loss"]) for i in range(STEPS)]
        out = {"eager": eager, "eager_nbt": _nbt(eager_m), "eager_step": tr.global_step, "eager_lr": tr.optimizer.param_groups[0]["lr"],
               "eager_buffers": [b.clone() for b in eager_m.model.zroot_ref.zroot_ref.buffers()],
               "a": _graph_run(base, batch), "b": _graph_run(base, batch), "miopen_wgrads": miopen}
    bn2d._conv_wgrad = conv_wgrad
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return out


def test_graph_replays_match_the_eager_loop(runs):
    graph = runs["a"]["losses"].tolist()
    print("eager", runs["eager"], "graph", graph)
    assert runs["a"]["global_step"] == runs["eager_step"] == STEPS
    assert runs["a"]["lr"] == pytest.approx(runs["eager_lr"], rel=1e-12)
    assert graph == pytest.approx(runs["eager"][WARMUP + 1:], rel=5e-2)


def _assert_bit_identical(a, b):
    assert torch.equal(a["losses"].view(torch.int32), b["losses"].view(torch.int32)), (a["losses"].tolist(), b["losses"].tolist())
    differ = [i for i, (x, y) in enumerate(zip(a["params"], b["params"])) if not torch.equal(x, y)]
    assert not differ, differ


def test_two_graph_runs_are_bit_identical(runs):
    """Two independent graph-mode runs from the same weights: bit-identical loss curves and final parameters.

    With 64 x 64 crops layer3 runs at 4 x 4 pixels and layer4 at 2 x 2, narrower than the 6 columns the weight-gradient kernels
    of the 3x3 and stride-2 convolutions need; under `routing(force=True)` those 11 gradients take the gathered form of the same
    GEMM (`bn2d._wgrad_narrow_x6`) instead of MIOpen, whose weight gradients differ in their last bit between identical runs at
    these sizes -- and Adam's first steps turn a last-bit difference of a near-zero gradient into a full step.  The fixture
    asserts that MIOpen's weight-gradient arm is never entered."""
    assert runs["miopen_wgrads"] == []
    _assert_bit_identical(runs["a"], runs["b"])


def test_two_graph_runs_are_bit_identical_where_every_weight_gradient_is_in_tree(monkeypatch):
    """192 x 192 crops: layer4 runs at 6 x 6 pixels, the smallest size at which the in-tree weight-gradient kernels take every
    convolution of the backbone (asserted: `_conv_wgrad`, the MIOpen arm, is never called)."""
    from peclr_amd import bn2d

    miopen, conv_wgrad = [], bn2d._conv_wgrad
    monkeypatch.setattr(bn2d, "_conv_wgrad", lambda gy, x, *a, **k: (miopen.append(tuple(x.shape)), conv_wgrad(gy, x, *a, **k))[1])
    batch = make_batches(B, 42, hw=(192, 192))[0]
    base = new_module(seed=12, num_samples=64)
    _assert_bit_identical(_graph_run(base, batch), _graph_run(base, batch))
    assert not miopen, miopen


def test_running_statistics_advance_once_per_replay(runs):
    a = runs["a"]
    first = a["nbt"][0]
    assert first == [WARMUP + 1] * 2                                   # the warm-up steps and the eager step of the capture routine
    assert a["nbt"] == [[first[0] + i] * 2 for i in range(STEPS - WARMUP)]
    for before, after in zip(a["means"], a["means"][1:]):
        assert not torch.equal(before, after)
    assert a["nbt"][-1] == runs["eager_nbt"] == [STEPS] * 2           # 5 replays later: the eager run's count
    # ... and the eager run's statistics: both are the same moving average (momentum 0.1) of the batch statistics of two
    # trajectories whose losses agree within 5e-2, so each tensor agrees within 5e-2 of its largest magnitude -- a replay that
    # used another momentum, or another batch, would be off by a multiple of that
    for x, y in zip(a["buffers"], runs["eager_buffers"]):
        assert x.shape == y.shape and torch.isfinite(x).all()
        if x.dtype.is_floating_point:
            worst = float((x - y).abs().max() / y.abs().max())
            print(f"running statistic {tuple(x.shape)}: graph against eager, max |d| / max |eager| = {worst:.3e}")
            assert worst <= 5e-2


# ------------------------------------------------------------------ 4. fit end to end
def test_fit_end_to_end(tmp_path):
    from peclr_amd import PoseEvaluator, Trainer
    from peclr_amd.finetune import EVALUATE_KEYS, TRAIN_KEYS, VAL_KEYS
    from peclr_amd.pose import RN25DwMLPref

    full = make_batches(24, 51)
    ragged = full[:2] + [{k: v[:4] for k, v in full[2].items()}]       # 20 samples: 8 + 8 + 4
    val = make_batches(B, 52)
    m = new_module(seed=21, evaluator=PoseEvaluator(capacity=B), num_samples=24)
    tr = Trainer(max_epochs=3, hip_graph=True, checkpoint_dir=str(tmp_path), save_top_k=3)
    calls = {"replay": 0, "eager": 0}
    replay_step, micro_step = tr.replay_step, tr.training_micro_step
    tr.replay_step = lambda *a, **k: (calls.__setitem__("replay", calls["replay"] + 1), replay_step(*a, **k))[1]
    tr.training_micro_step = lambda *a, **k: (calls.__setitem__("eager", calls["eager"] + 1), micro_step(*a, **k))[1]
    per_epoch = []

    def train_batches(epoch):
        per_epoch.append(dict(calls))
        return ragged if epoch == 1 else full

    tr.fit(m, train_batches, lambda epoch: val)
    torch.cuda.synchronize()
    assert tr.global_step == 9
    # epoch 0: capture (its own eager step) + 2 replays; epoch 1: 2 replays + the ragged batch eagerly; epoch 2: 3 replays again
    assert per_epoch == [{"replay": 0, "eager": 0}, {"replay": 2, "eager": 0}, {"replay": 4, "eager": 1}]
    assert calls == {"replay": 7, "eager": 1}
    assert tuple(m.train_metrics_epoch) == TRAIN_KEYS
    assert all(torch.isfinite(v) for v in m.train_metrics_epoch.values())
    assert tuple(m.validation_metrics_epoch) == VAL_KEYS + EVALUATE_KEYS
    assert all(np.isfinite(float(v)) for v in m.validation_metrics_epoch.values())
    assert float(m.logged["checkpoint_saving_loss"]) == float(m.train_metrics_epoch["loss_3d"])
    assert sorted(os.listdir(tmp_path)) == ["epoch=0.ckpt", "epoch=1.ckpt", "epoch=2.ckpt"]

    # the export, loaded into a fresh pose model, predicts what the module itself predicts -- bit for bit
    path = m.export(str(tmp_path / "rn50_finetuned.pth"))
    fresh = RN25DwMLPref("rn50")
    fresh.load_state_dict(torch.load(path, map_location="cpu")["state_dict"], strict=True)
    fresh = fresh.eval().to(DEV).enable_hip()
    m.eval()
    with torch.no_grad():
        theirs, ours = fresh(val[0]["image"], val[0]["K"]), m.model(val[0]["image"], val[0]["K"])
    for k in ("kp25d", "kp3d"):
        assert torch.equal(theirs[k], ours[k]), k
    tr.close()

    # resume from the last checkpoint and train one more epoch
    m2 = new_module(seed=22, evaluator=PoseEvaluator(capacity=B), num_samples=24)
    tr2 = Trainer(max_epochs=4, hip_graph=True, checkpoint_dir=str(tmp_path), save_top_k=4).attach(m2)
    tr2.resume(str(tmp_path / "epoch=2.ckpt"))
    assert tr2.global_step == 9 and tr2.current_epoch == 3
    for a, b in zip(m2.state_dict().values(), m.state_dict().values()):
        assert torch.equal(a, b)
    tr2.fit(m2, lambda epoch: full, lambda epoch: val)
    torch.cuda.synchronize()
    assert tr2.global_step == 12 and os.path.exists(tmp_path / "epoch=3.ckpt")
    assert tuple(m2.train_metrics_epoch) == TRAIN_KEYS and torch.isfinite(m2.train_metrics_epoch["loss"])
    tr2.close()


# ------------------------------------------------------------------ 5. learning
@pytest.mark.parametrize("arm", ["hip", "stock"])
def test_the_loss_falls_on_one_repeated_batch(arm):
    """One batch, augmentation off, LEARN_STEPS Adam steps under the cosine schedule: the last step's loss is below the first's,
    on the HIP kernels and on the stock path (same seed, same optimiser) alike."""
    from peclr_amd import Trainer

    batch = make_batches(B, 61)[0]
    cfg = dict(num_samples=B * LEARN_STEPS, lr=LEARN_LR)
    m = new_module(seed=31, **cfg) if arm == "hip" else stock_module(seed=31, **cfg)
    tr = Trainer(max_epochs=1).attach(m)
    tr.zero_grad()
    losses = [tr.training_micro_step(batch, i)["loss"] for i in range(LEARN_STEPS)]
    curve = torch.stack(losses).tolist()
    print(f"learning {arm}:", [round(v, 4) for v in curve])
    assert np.isfinite(curve).all() and curve[-1] < curve[0]


# ------------------------------------------------------------------ 6. guards
def test_a_hip_model_without_its_kernels_is_refused_before_any_launch():
    from peclr_amd import _capi

    batch = make_batches(B, 71)[0]
    m = new_module(hip=False, num_samples=64)
    _capi.EVENT_LOG = {}
    try:
        with pytest.raises(_capi.PeclrHipError, match="enable_hip"):
            m.training_step(batch, 0)
        m.eval()
        with pytest.raises(_capi.PeclrHipError, match="enable_hip"):
            m.validation_step(batch, 0)
        assert _capi.EVENT_LOG == {}
    finally:
        _capi.EVENT_LOG = None
    m.model.enable_hip()                                  # the backbone alone is not enough: the training head is still off
    with pytest.raises(_capi.PeclrHipError, match="enable_hip"):
        m.train().training_step(batch, 0)


def test_validation_step_changes_no_running_statistic():
    from peclr_amd import PoseEvaluator
    from peclr_amd.finetune import VAL_KEYS

    batch = make_batches(B, 72)[0]
    m = new_module(seed=41, evaluator=PoseEvaluator(capacity=2 * B), num_samples=64)
    with pytest.raises(RuntimeError, match="eval mode"):
        m.validation_step(batch, 0)
    m.eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    out = m.validation_step(batch, 0)
    torch.cuda.synchronize()
    assert tuple(out) == VAL_KEYS and not any(v.requires_grad for v in out.values())
    assert all(torch.isfinite(v) for v in out.values())
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    m.validation_epoch_end([out])
    assert float(m.validation_metrics_epoch["loss_3d_val"]) == float(out["loss_3d_val"])
    assert "Mean_EPE_3D" in m.validation_metrics_epoch
