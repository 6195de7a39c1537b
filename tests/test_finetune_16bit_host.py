"""Host side of 16-bit fine-tuning (peclr_amd/finetune.py): which precisions `setup()` takes and how it names them, the
condition it puts on a 16-bit one, and how `fold_bn` resolves.  No device: the two flags `enable_hip()` sets are set by hand."""
import types

import pytest
import torch

from peclr_amd import SupervisedPose, supervised_config
from peclr_amd.pose import FreiHANDPredictor


def module(hip, **kw):
    m = SupervisedPose(supervised_config(batch_size=8, num_samples=64), **kw)
    if hip:                                   # what `.to(device).enable_hip()` leaves behind
        m.model.backend_model.bn1.hip = True
        m.model.hip_training = True
    return m


def attach(m, precision, world_size=1):
    m.trainer = types.SimpleNamespace(world_size=world_size, precision=precision, max_epochs=1)
    m.setup("fit")
    return m


@pytest.mark.parametrize("asked,normalised", [("bf16", "bf16"), ("fp16", "fp16"), (16, "fp16"), ("16", "fp16"),
                                              ("fp32", "fp32"), (32, "fp32"), ("32", "fp32")])
def test_setup_normalises_the_precision(asked, normalised):
    m = module(hip=True)
    assert m.precision == "fp32"              # before any trainer
    attach(m, asked)
    assert m.precision == normalised and m.train_iters_per_epoch == 8


@pytest.mark.parametrize("asked", ["bf16", "fp16", 16, "16"])
def test_a_16_bit_precision_needs_the_hip_kernels(asked):
    for flags in ((False, False), (True, False), (False, True)):
        m = module(hip=False)
        m.model.backend_model.bn1.hip, m.model.hip_training = flags
        with pytest.raises(RuntimeError, match="fp32 only") as err:
            attach(m, asked)
        assert "enable_hip()" in str(err.value)
        assert m.precision == "fp32"          # a refused precision is not stored


def test_fp32_needs_no_kernels_and_an_unknown_precision_is_refused():
    attach(module(hip=False), "fp32")
    for asked in ("fp64", 8, True, None, 16.0):
        with pytest.raises(RuntimeError, match="fp32 only"):
            attach(module(hip=True), asked)


@pytest.mark.parametrize("asked", ["fp32", "bf16", 16])
def test_more_than_one_process_is_still_refused(asked):
    with pytest.raises(RuntimeError, match="single-process"):
        attach(module(hip=True), asked, world_size=2)


def test_fold_bn_resolution():
    default = FreiHANDPredictor.FOLD_BN_DEFAULT
    for asked in ("bf16", "fp16", 16, "16"):
        assert attach(module(hip=True), asked).fold_bn is default
        assert attach(module(hip=True, fold_bn=False), asked).fold_bn is False
        assert attach(module(hip=True, fold_bn=True), asked).fold_bn is True
    for kw in ({}, {"fold_bn": None}, {"fold_bn": True}, {"fold_bn": False}):
        assert module(hip=True, **kw).fold_bn is False                     # no trainer yet: fp32
        assert attach(module(hip=True, **kw), "fp32").fold_bn is False     # always off in fp32
    m = attach(module(hip=True, fold_bn=True), "bf16")
    assert attach(m, 32).fold_bn is False and attach(m, "fp16").fold_bn is True     # follows a re-attach


def test_fp32_validation_enters_no_context():
    import contextlib

    m = attach(module(hip=True, fold_bn=True), "fp32")
    assert isinstance(m._eval_precision(), contextlib.nullcontext)
    assert not torch.is_autocast_enabled("cuda")
