"""Fine-tuning the 2.5D pose model in bf16 and fp16 on the device (peclr_amd/finetune.py): one step against a float64 run of the
same weights, the whole step as one hipGraph against the eager loop, fp16 overflow skipped by the replay itself, `Trainer.fit`
end to end, 16-bit validation with eval BatchNorm folded, learning, and the guard.

Sizes: rn50, B = 8, 224 x 224 crops -- the size at which tests/test_conv_h_gpu.py holds the whole 16-bit network, and the
smallest at which layer1-3 reach the in-tree 16-bit weight-gradient kernels and layer4 runs at 7 x 7.  Every convolution is
routed to the in-tree kernels (`bn2d.routing(force=True)`) and everything runs on one side stream, as in test_finetune_gpu.py.

The bound of the comparisons against a reference is the project's rule for 16-bit whole-network comparisons
(test_conv_h_gpu.py): with e = |value - gold| / |gold|,  e(in-tree) <= 1.5 x e(stock torch under the same autocast) + 4 ULP
of the 16-bit format.  The `parity` lines this module prints are profiles/pose_finetune_16bit_parity.txt.
"""
import copy
import os

import numpy as np
import pytest
import torch

from tests import pose_metrics_ref
from tests.test_finetune_gpu import make_batches, stock_values

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, HW = 8, (224, 224)
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}
PRECISIONS = ["bf16", "fp16"]
FP16_LOSS_SCALE = 2.0 ** 10          # test 1: both 16-bit arms scale the loss by it, so the stock fp16 backward does not underflow
SEQ = "model.zroot_ref.zroot_ref."
ZERO_GRAD = (SEQ + "0.bias", SEQ + "3.bias")     # in front of a train-mode BatchNorm1d: mathematically 0
CONV_TAGS = ("conv1x1_fwd", "conv1x1_dgrad", "conv1x1_dgrad_add", "conv3x3_fwd", "conv3x3_dgrad")
STEPS, WARMUP = 9, 3
LEARN_STEPS, LEARN_LR = 30, 1e-3


def new_module(seed=5, evaluator=None, hip=True, fold_bn=None, **cfg):
    from peclr_amd import SupervisedPose, supervised_config

    torch.manual_seed(seed)
    m = SupervisedPose(supervised_config(batch_size=B, **cfg), evaluator=evaluator, fold_bn=fold_bn).to(DEV).train()
    return m.enable_hip() if hip else m.to(memory_format=torch.channels_last)


def bound(e_stock, dtype):
    return 1.5 * e_stock + 4 * ULP[dtype]


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


class _launch_log:
    """`with _launch_log() as log:` -- log.tags (launch order) and log.kernels (tag -> kernel names) of what ran inside."""

    def __enter__(self):
        from peclr_amd import _capi

        _capi.EVENT_LOG, _capi.LAUNCH_ORDER = {}, []
        return self

    def __exit__(self, *exc):
        from peclr_amd import _capi

        torch.cuda.synchronize()
        self.tags = list(_capi.LAUNCH_ORDER)
        self.kernels = {}
        for k, v in _capi.EVENT_LOG.items():
            self.kernels.setdefault(k.split("~")[0], []).extend(e[4] for e in v)
        _capi.EVENT_LOG, _capi.LAUNCH_ORDER = None, None
        return False


def stock_under_autocast(model, dtype):
    """The stock 16-bit arm's network: torch's operators under `torch.autocast`, its outputs widened to float32 for the losses."""
    def call(img, K):
        with torch.autocast("cuda", dtype=dtype):
            out = model(img, K)
        return {k: v.float() for k, v in out.items()}
    return call


# ------------------------------------------------------------------ 1. one step against float64
@pytest.fixture(scope="module")
def gold():
    """One batch, one set of weights and the float64 stock step on them (values and gradients), computed once on the device."""
    from peclr_amd import bn2d

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with bn2d.routing(force=True), torch.cuda.stream(side):
        batch = make_batches(B, 31, hw=HW)[0]
        base = new_module(num_samples=64)
        model64 = copy.deepcopy(base.model).enable_hip(False).enable_hip_training(False).double()
        assert not model64.backend_model.bn1.hip and model64.training
        batch64 = {k: v.detach().double() for k, v in batch.items()}
        values, out64 = stock_values(model64, batch64, base.loss.weights)
        values["loss"].backward()
        g64 = {k: float(v) for k, v in values.items()}
        for name, (p, t) in (("", (out64["kp25d"], batch64["joints"])), ("_3d", (out64["kp3d"], batch64["joints3D"]))):
            mean, median = pose_metrics_ref.metrics64(p.detach().cpu().numpy(), t.cpu().numpy())
            for key, value in ((f"EPE_mean{name}_train", mean), (f"EPE_median{name}_train", median)):
                assert abs(value - g64[key]) <= 1e-12 * value
                g64[key] = value
        grads = {"model." + n: p.grad.clone() for n, p in model64.named_parameters()}
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    del model64
    return {"batch": batch, "base": base, "values": g64, "grads": grads}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_step_against_float64(gold, precision):
    """Figures of the run recorded in profiles/pose_finetune_16bit_parity.txt.

    What the gradient term can see: little.  At a fresh initialisation on noise images this step's gradient is ill conditioned --
    the fp32 arms, stock and in-tree alike, are already 2e-2 of a parameter's gradient norm away from float64 (fp32 rounding
    amplified ~1e5 times: the samples' predictions are nearly equal and the train-mode BatchNorm layers divide by their small
    spread), and BOTH 16-bit arms are of the order of the norm itself away from float64 and from each other (median parameter:
    1.4 in bf16, 0.8 in fp16; only `fc` stays at 0.15 / 0.08).  Moving the bias of `fc` to the batch's mean target, so that the
    L1 signs are mixed, did not change that (tried: medians 1.3 / 0.8).  So the term holds the in-tree arm to "no further off
    than stock autocast" and nothing finer; the backward arithmetic of the 16-bit kernels is held where it is well conditioned,
    by tests/test_conv_h_gpu.py (random upstream gradient), and this test adds the nine values, finiteness, the zero rows of
    `fc` and the launch log of the composed step."""
    from peclr_amd import Trainer
    from peclr_amd.finetune import TRAIN_KEYS

    dtype, batch, g64 = DTYPE[precision], gold["batch"], gold["values"]
    scale = FP16_LOSS_SCALE if precision == "fp16" else 1.0
    m = copy.deepcopy(gold["base"])
    stock = copy.deepcopy(m.model).enable_hip(False).enable_hip_training(False)
    assert not stock.backend_model.bn1.hip and stock.training
    tr = Trainer(precision=precision).attach(m)
    assert m.precision == precision
    with _launch_log() as log:
        with tr._autocast():
            out = m.training_step(batch, 0)
        (out["loss"] * scale).backward()
        tr._join_wgrad()
    assert tuple(out) == TRAIN_KEYS and [k for k, v in out.items() if v.requires_grad] == ["loss"]
    assert all(v.dtype == torch.float32 for v in out.values())
    for t in CONV_TAGS:
        assert t in log.kernels and all(k and k.startswith("conv_h_kernel") for k in log.kernels[t]), (t, log.kernels.get(t))
    assert "h_pack" in log.kernels
    x6 = sorted({k for ks in log.kernels.values() for k in ks if k and k.startswith("gemm_x6")})
    assert not x6, x6
    s16, _ = stock_values(stock_under_autocast(stock, dtype), batch, m.loss.weights)
    (s16["loss"] * scale).backward()
    torch.cuda.synchronize()

    worst = 0.0
    for key in TRAIN_KEYS:
        g = g64[key]
        if g == 0.0:
            assert float(out[key]) == 0.0
            continue
        e_hip, e_stock = abs(float(out[key]) - g) / abs(g), abs(float(s16[key]) - g) / abs(g)
        ratio = e_hip / bound(e_stock, dtype)
        print(f"parity one step {precision} {key}: gold64 = {g:.9g} e_hip = {e_hip:.3e} e_stock16 = {e_stock:.3e} "
              f"e_hip / (1.5 e_stock16 + 4 ulp) = {ratio:.3f}")
        worst = max(worst, ratio)

    rel = lambda a, b: float((a.double() - b).norm() / b.norm())   # noqa: E731
    stock_grads = {"model." + n: p.grad for n, p in stock.named_parameters()}
    per_param = []
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert torch.isfinite(stock_grads[name]).all(), name
        if name.startswith("model.backend_model.fc."):
            assert (p.grad[[2, 63]] == 0).all() and (p.grad[[i for i in range(64) if i not in (2, 63)]] != 0).any(), name
        if name in ZERO_GRAD:
            continue
        per_param.append((rel(p.grad / scale, gold["grads"][name]), rel(stock_grads[name] / scale, gold["grads"][name]), name))
    e_hip, e_stock = max(e[0] for e in per_param), max(e[1] for e in per_param)
    ratio = e_hip / bound(e_stock, dtype)
    print(f"parity one step {precision} gradients: max over parameters of |g - g64| / |g64|: e_hip = {e_hip:.3e} "
          f"e_stock16 = {e_stock:.3e} e_hip / (1.5 e_stock16 + 4 ulp) = {ratio:.3f}")
    print(f"parity one step {precision} gradients: the worst parameter is {max(per_param)[2]} (in-tree), {max(per_param, key=lambda e: e[1])[2]} "
          f"(stock); median over parameters e_hip = {np.median([e[0] for e in per_param]):.3e} e_stock16 = {np.median([e[1] for e in per_param]):.3e}")
    worst = max(worst, ratio)
    print(f"parity one step {precision}: worst e_hip / bound = {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ 2. the step as one hipGraph against the eager loop
def _nbt(m):
    s = m.model.zroot_ref.zroot_ref
    return [int(s[1].num_batches_tracked), int(s[4].num_batches_tracked)]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_graph_replays_match_the_eager_loop(precision):
    from peclr_amd import Trainer
    from peclr_amd.optim import DeviceLossScaler

    batch = make_batches(B, 41, hw=HW)[0]
    base = new_module(seed=11, num_samples=64)
    te = Trainer(max_epochs=10, precision=precision).attach(copy.deepcopy(base))
    te.zero_grad()
    eager = [float(te.training_micro_step(batch, i)["loss"]) for i in range(STEPS)]
    mg = copy.deepcopy(base)
    tg = Trainer(max_epochs=10, precision=precision).attach(mg)
    tg.zero_grad()
    tg.capture_step_graph(batch, warmup=WARMUP)
    nbt, graph = [_nbt(mg)], []
    for _ in range(STEPS - WARMUP - 1):
        graph.append(float(tg.replay_step()["loss"]))
        nbt.append(_nbt(mg))
    torch.cuda.synchronize()
    assert tg.global_step == te.global_step == STEPS
    assert tg.optimizer.param_groups[0]["lr"] == pytest.approx(te.optimizer.param_groups[0]["lr"], rel=1e-12)
    worst = max(abs(g - e) / abs(e) for g, e in zip(graph, eager[WARMUP + 1:]))
    print(f"graph against eager {precision}: eager {eager} graph {graph} worst |graph - eager| / |eager| = {worst:.3e} "
          f"= {worst / 6e-2:.3f} of the bound")
    assert np.isfinite(eager).all() and np.isfinite(graph).all()
    assert graph == pytest.approx(eager[WARMUP + 1:], rel=6e-2)
    assert nbt == [[WARMUP + 1 + i] * 2 for i in range(STEPS - WARMUP)]          # one per replay
    if precision == "fp16":
        assert isinstance(tg._scaler, DeviceLossScaler) and isinstance(te._scaler, DeviceLossScaler)
        assert tg._scaler.get_scale() == te._scaler.get_scale()
    else:
        assert tg._scaler is None and te._scaler is None
    tg.close()


# ------------------------------------------------------------------ 3. fp16 overflow is skipped by the replay itself
def test_fp16_overflow_is_skipped_by_the_replay():
    """An inf gradient (the loss scaled by 2^100), not a fault: the replayed optimiser launch sees it and leaves weights and
    moments alone; the forward ran, so the head's BatchNorm1d statistics advance, as torch's do on a skipped step."""
    from peclr_amd import Trainer

    batch = make_batches(B, 43, hw=HW)[0]
    m = new_module(seed=13, num_samples=64)
    tr = Trainer(max_epochs=10, precision=16).attach(m)
    tr.zero_grad()
    tr.capture_step_graph(batch, warmup=WARMUP)
    tr.replay_step()
    torch.cuda.synchronize()
    good, step, nbt, scale = tr._scaler.good_steps(), tr.global_step, _nbt(m), 2.0 ** 100
    tr._scaler._f[0] = scale
    w = [p.detach().clone() for p in m.parameters()]
    state = [p for p in m.parameters() if p in tr.optimizer.state]
    avg = [tr.optimizer.state[p]["exp_avg"].clone() for p in state]
    mean = m.model.zroot_ref.zroot_ref[1].running_mean.clone()
    for k in range(3):
        out = tr.replay_step()
        assert np.isfinite(float(out["loss"]))                          # the unscaled loss
        assert tr._scaler.get_scale() == scale / 2 ** (k + 1)
    assert all(torch.equal(a, b) for a, b in zip(w, m.parameters()))
    assert state and all(torch.equal(a, tr.optimizer.state[p]["exp_avg"]) for a, p in zip(avg, state))
    assert tr._scaler.good_steps() == good and tr.global_step == step + 3
    assert _nbt(m) == [n + 3 for n in nbt]
    assert not torch.equal(mean, m.model.zroot_ref.zroot_ref[1].running_mean)
    tr._scaler._f[0] = 1024.0
    tr.replay_step()
    torch.cuda.synchronize()
    assert tr._scaler.good_steps() == good + 1 and tr._scaler.get_scale() == 1024.0
    assert any(not torch.equal(a, b) for a, b in zip(w, m.parameters()))
    assert int(tr.optimizer.state_dict()["state"][0]["step"]) == good + 1
    tr.close()


# ------------------------------------------------------------------ 4. fit end to end
def test_fit_end_to_end_in_precision_16(tmp_path):
    from peclr_amd import PoseEvaluator, Trainer, bn2d
    from peclr_amd.finetune import EVALUATE_KEYS, TRAIN_KEYS, VAL_KEYS
    from peclr_amd.optim import DeviceLossScaler
    from peclr_amd.pose import RN25DwMLPref

    full = make_batches(24, 51, hw=HW)
    ragged = full[:2] + [{k: v[:4] for k, v in full[2].items()}]       # 20 samples: 8 + 8 + 4
    val = make_batches(B, 52, hw=HW)
    m = new_module(seed=21, evaluator=PoseEvaluator(capacity=B), num_samples=24)
    tr = Trainer(max_epochs=3, precision=16, hip_graph=True, checkpoint_dir=str(tmp_path), save_top_k=3)
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
    assert m.precision == "fp16" and isinstance(tr._scaler, DeviceLossScaler)
    assert tr.global_step == 9
    # epoch 0: capture (its own eager step) + 2 replays; epoch 1: 2 replays + the ragged batch eagerly; epoch 2: 3 replays again
    assert per_epoch == [{"replay": 0, "eager": 0}, {"replay": 2, "eager": 0}, {"replay": 4, "eager": 1}]
    assert calls == {"replay": 7, "eager": 1}
    assert tuple(m.train_metrics_epoch) == TRAIN_KEYS
    assert all(torch.isfinite(v) for v in m.train_metrics_epoch.values())
    assert tuple(m.validation_metrics_epoch) == VAL_KEYS + EVALUATE_KEYS
    assert all(np.isfinite(float(v)) for v in m.validation_metrics_epoch.values())
    assert sorted(os.listdir(tmp_path)) == ["epoch=0.ckpt", "epoch=1.ckpt", "epoch=2.ckpt"]
    scale = tr._scaler.get_scale()
    saved = torch.load(str(tmp_path / "epoch=2.ckpt"), map_location="cpu")["native_amp_scaling_state"]
    assert saved["scale"] == scale and saved["_growth_tracker"] == tr._scaler.state_dict()["_growth_tracker"]

    # the export, loaded into a fresh pose model, predicts what the module's model predicts under the same autocast and fold
    path = m.export(str(tmp_path / "rn50_finetuned.pth"))
    fresh = RN25DwMLPref("rn50")
    fresh.load_state_dict(torch.load(path, map_location="cpu")["state_dict"], strict=True)
    fresh = fresh.eval().to(DEV).enable_hip()
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16), bn2d.routing(fold_eval_bn=m.fold_bn):
        theirs, ours = fresh(val[0]["image"], val[0]["K"]), m.model(val[0]["image"], val[0]["K"])
    for k in ("kp25d", "kp3d"):
        assert torch.isfinite(ours[k]).all() and torch.equal(theirs[k], ours[k]), k
    tr.close()

    # resume from the last checkpoint: the scale and every entry of the state dict come back, and one more epoch trains
    m2 = new_module(seed=22, evaluator=PoseEvaluator(capacity=B), num_samples=24)
    tr2 = Trainer(max_epochs=4, precision=16, hip_graph=True, checkpoint_dir=str(tmp_path), save_top_k=4).attach(m2)
    tr2.resume(str(tmp_path / "epoch=2.ckpt"))
    assert tr2.global_step == 9 and tr2.current_epoch == 3
    assert isinstance(tr2._scaler, DeviceLossScaler) and tr2._scaler.get_scale() == scale
    for a, b in zip(m2.state_dict().values(), m.state_dict().values()):
        assert torch.equal(a, b)
    tr2.fit(m2, lambda epoch: full, lambda epoch: val)
    torch.cuda.synchronize()
    assert tr2.global_step == 12 and os.path.exists(tmp_path / "epoch=3.ckpt")
    assert tuple(m2.train_metrics_epoch) == TRAIN_KEYS and torch.isfinite(m2.train_metrics_epoch["loss"])
    tr2.close()


# ------------------------------------------------------------------ 5. validation
def _validation_tags(m, batch):
    m.validation_step(batch, 0)                    # (weight planes and tables exist after this one)
    with _launch_log() as log:
        out = m.validation_step(batch, 0)
    return log.tags, out


def _is_apply(tag):
    return tag.startswith("bn2d_") and "apply" in tag


@pytest.mark.parametrize("precision", PRECISIONS)
def test_validation_step_in_16_bit(precision):
    """The gold is the fp32 `validation_step` of the same weights.  The stock arm is the same model on torch's operators, in
    eval mode under the same autocast; its float32-widened prediction goes through the same fp32 losses, lifting and metrics,
    so the two arms differ in the network's kernels alone."""
    from peclr_amd import Trainer, step_metrics
    from peclr_amd.finetune import LOSS_NAMES, METRIC_NAMES, VAL_KEYS
    from peclr_amd.supervised import joints25d_to_3d

    dtype = DTYPE[precision]
    batch = make_batches(B, 72, hw=HW)[0]
    base = new_module(seed=41, num_samples=64)
    with torch.no_grad():                           # running statistics away from their initial 0 / 1, so a dropped table would show
        for name, buf in base.named_buffers():
            if name.endswith(("running_mean", "running_var")):
                buf.copy_(torch.rand_like(buf) * 0.2 + (0.9 if name.endswith("running_var") else -0.1))
    base.eval()
    m32, m16, m16u = copy.deepcopy(base), copy.deepcopy(base), new_module(seed=41, fold_bn=False, num_samples=64).eval()
    m16u.load_state_dict(base.state_dict())
    for m, p in ((m32, "fp32"), (m16, precision), (m16u, precision)):
        Trainer(precision=p).attach(m)
    assert m16.fold_bn is True and m16u.fold_bn is False and m32.fold_bn is False
    before = {k: v.clone() for k, v in m16.state_dict().items()}

    tags, out = _validation_tags(m16, batch)
    assert tuple(out) == VAL_KEYS and not any(v.requires_grad for v in out.values())
    assert {"conv1x1_bnact", "conv3x3_bnact", "conv_s2_bnact"} <= set(tags)
    assert [t for t in tags if _is_apply(t)] == ["bn2d_pool_apply", "bn2d_apply_avgpool"]      # the stem's and the tail's
    assert tags.count("bn2d_eval_tables") == 1
    for k, v in m16.state_dict().items():
        assert torch.equal(v, before[k]), k
    plain, out_u = _validation_tags(m16u, batch)
    assert not any(t.endswith("_bnact") or t == "bn2d_eval_tables" for t in plain)
    assert plain.count("bn2d_apply") >= 47 and {"conv1x1_fwd", "conv3x3_fwd"} <= set(plain)
    for k, v in m16u.state_dict().items():
        assert torch.equal(v, before[k]), k

    gold = m32.validation_step(batch, 0)
    stock = copy.deepcopy(base.model).enable_hip(False).enable_hip_training(False).eval()
    with torch.no_grad():
        kp25d = stock_under_autocast(stock, dtype)(batch["image"], batch["K"])["kp25d"].contiguous()
        total, losses = m32.loss(kp25d, batch, z_root_calc=None)
        metrics = step_metrics(kp25d, batch["joints"], joints25d_to_3d(kp25d, batch["scale"], batch["K"]), batch["joints3D"])
    s16 = {**{f"{n}_val": losses[n] for n in LOSS_NAMES}, **{f"{n}_val": v for n, v in zip(METRIC_NAMES, metrics.unbind(0))}, "loss": total}
    torch.cuda.synchronize()
    worst = 0.0
    for arm, got in (("folded", out), ("unfolded", out_u)):
        for key in VAL_KEYS:
            g = float(gold[key])
            assert np.isfinite(g) and g != 0.0, key
            e_hip, e_stock = abs(float(got[key]) - g) / abs(g), abs(float(s16[key]) - g) / abs(g)
            ratio = e_hip / bound(e_stock, dtype)
            print(f"parity validation {precision} {arm} {key}: fp32 = {g:.9g} e_hip = {e_hip:.3e} e_stock16 = {e_stock:.3e} "
                  f"e_hip / (1.5 e_stock16 + 4 ulp) = {ratio:.3f}")
            worst = max(worst, ratio)
    print(f"parity validation {precision}: worst e_hip / bound = {worst:.3f}")
    assert worst <= 1.0


def test_fp32_validation_launches_what_it_launched_before():
    """A module set up in fp32 -- whatever `fold_bn` it was given -- launches the tags of the validation step written out by
    hand without any precision context (the step as it was before `fold_bn` existed), in the same order."""
    from peclr_amd import PoseEvaluator, Trainer, step_metrics
    from peclr_amd.supervised import joints25d_to_3d

    batch = make_batches(B, 73, hw=HW)[0]
    m = new_module(seed=42, evaluator=PoseEvaluator(capacity=4 * B), fold_bn=True, num_samples=64).eval()
    Trainer(precision=32).attach(m)
    assert m.precision == "fp32" and m.fold_bn is False

    def by_hand():
        with torch.no_grad():
            kp25d = m.model(batch["image"], batch["K"])["kp25d"].contiguous()
            m.loss(kp25d, batch, z_root_calc=None)
            kp3d = joints25d_to_3d(kp25d, batch["scale"], batch["K"])
            step_metrics(kp25d, batch["joints"], kp3d, batch["joints3D"])
            m.evaluator.update_25d(kp25d, batch["scale"], batch["K"], batch["joints3D"])

    by_hand()
    with _launch_log() as before:
        by_hand()
    tags, _ = _validation_tags(m, batch)
    assert tags == before.tags and tags
    assert not any(t.endswith("_bnact") or t == "bn2d_eval_tables" for t in tags)


# ------------------------------------------------------------------ 6. learning
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_loss_falls_on_one_repeated_batch(precision):
    from peclr_amd import Trainer

    batch = make_batches(B, 61, hw=HW)[0]
    m = new_module(seed=31, num_samples=B * LEARN_STEPS, lr=LEARN_LR)
    tr = Trainer(max_epochs=1, precision=precision).attach(m)
    tr.zero_grad()
    losses = [tr.training_micro_step(batch, i)["loss"] for i in range(LEARN_STEPS)]
    curve = torch.stack(losses).tolist()
    skipped = LEARN_STEPS - tr._scaler.good_steps() if precision == "fp16" else 0
    print(f"learning {precision} ({skipped} steps skipped by the loss scaler):", [round(v, 4) for v in curve])
    assert np.isfinite(curve).all() and curve[-1] < curve[0]


# ------------------------------------------------------------------ 7. guards
def test_16_bit_without_the_hip_kernels_is_refused_before_any_launch():
    from peclr_amd import Trainer, _capi

    m = new_module(hip=False, num_samples=64)
    _capi.EVENT_LOG = {}
    try:
        for precision in ("bf16", 16):
            with pytest.raises(RuntimeError, match="fp32 only"):
                Trainer(precision=precision).attach(m)
        assert _capi.EVENT_LOG == {}
    finally:
        _capi.EVENT_LOG = None
    assert m.precision == "fp32"
