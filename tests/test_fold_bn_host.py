"""16-bit prediction with the eval-mode BatchNorm layers folded into the convolution epilogues: everything that is decided on
the host -- the switch, which layers fold (`bn2d.fold_plan`), what the new entry points refuse before any launch, and the
predictor's `precision` argument.  No GPU."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT


def test_the_switch_is_off_without_the_environment_variable():
    env = {k: v for k, v in os.environ.items() if k != "PECLR_FOLD_EVAL_BN"}
    code = "from peclr_amd import bn2d; print(bn2d.ROUTING.fold_eval_bn, bn2d.Routing().fold_eval_bn)"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
    assert out.split() == ["False", "False"]
    env["PECLR_FOLD_EVAL_BN"] = "1"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
    assert out.split() == ["True", "True"]


@pytest.fixture(scope="module")
def rn50():
    from peclr_amd import pose

    return pose.RN25DwMLPref("rn50").backend_model


def _all_pairs(backbone):
    """Every (convolution, BatchNorm2d) pair of the backbone, by name, in module order."""
    names = [n for n, m in backbone.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]
    return {n: n.replace("bn", "conv") if "downsample" not in n else n[:-1] + "0" for n in names}


def test_rn50_plan_is_every_layer_but_the_stem_and_the_pooled_tail(rn50):
    from peclr_amd import bn2d

    plan = bn2d.fold_plan(rn50)
    assert len(plan) == 51 and len(set(plan)) == 51
    pairs = _all_pairs(rn50)
    assert len(pairs) == 53
    assert set(pairs) - {b for _, b in plan} == {"bn1", "layer4.2.bn3"}
    for conv, bn in plan:
        assert pairs[bn] == conv
    # in launch order inside a block: conv1, conv2, the shortcut, conv3
    assert plan[:4] == [("layer1.0.conv1", "layer1.0.bn1"), ("layer1.0.conv2", "layer1.0.bn2"),
                        ("layer1.0.downsample.0", "layer1.0.downsample.1"), ("layer1.0.conv3", "layer1.0.bn3")]
    assert plan[-2:] == [("layer4.2.conv1", "layer4.2.bn1"), ("layer4.2.conv2", "layer4.2.bn2")]


def test_rn152_and_resnet18_plans():
    from peclr_amd import bn2d, pose, resnet

    assert len(bn2d.fold_plan(pose.RN25DwMLPref("rn152").backend_model)) == 153
    assert bn2d.fold_plan(resnet.resnet18()) == []                      # BasicBlocks are never folded
    # without the pooled tail the last bn3 folds like any other
    assert len(bn2d.fold_plan(resnet.resnet50())) == 52


@pytest.mark.parametrize("block,entries", [("layer2.1", 3), ("layer3.0", 4)])
def test_a_layer_that_does_not_qualify_takes_its_whole_block_out_and_nothing_else(block, entries):
    from peclr_amd import bn2d, pose

    bb = pose.RN25DwMLPref("rn50").backend_model
    full = bn2d.fold_plan(bb)
    dict(bb.named_modules())[block + ".bn2"].affine = False
    plan = bn2d.fold_plan(bb)
    gone = [p for p in full if p not in plan]
    assert len(gone) == entries and all(c.startswith(block + ".") for c, _ in gone)
    assert plan == [p for p in full if not p[0].startswith(block + ".")]


def test_other_disqualifiers():
    from peclr_amd import bn2d, pose

    bb = pose.RN25DwMLPref("rn50").backend_model
    n = len(bn2d.fold_plan(bb))
    mods = dict(bb.named_modules())
    mods["layer1.1.bn1"].track_running_stats = False
    assert len(bn2d.fold_plan(bb)) == n - 3
    mods["layer1.2"].bn3 = torch.nn.BatchNorm2d(256)                    # not the fused class
    assert len(bn2d.fold_plan(bb)) == n - 6
    mods["layer2.0"].conv2.groups = 2                                   # a convolution no pack group takes
    assert len(bn2d.fold_plan(bb)) == n - 10


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    from peclr_amd import _capi

    L = _capi.lib()
    ALIGN, UNSUPPORTED = -3, -5                                        # PECLR_ERR_ALIGN / PECLR_ERR_UNSUPPORTED
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15                             # a non-null, 16-byte aligned host address: never dereferenced
    gemm = lambda n=128, k=64, ss=p, a=p: L.peclr_gemm_h_bnact(1, 256, n, k, a, k, p, p, n, None, n, ss, 1, 0, None)
    conv = lambda taps=9, cout=64, cin=64, ss=p, stride=1: L.peclr_conv_h_bnact(1, 1, 8, 8, cin, cout, taps, stride, p, p, p, 0, p, ss, 1, None)
    null_code = L.peclr_gemm_h(1, 256, 128, 64, None, 64, p, p, 128, None, 128, 0, 0, None, 0, None, None, None, None)
    shape_code = L.peclr_gemm_h(1, 256, 96, 64, p, 64, p, p, 96, None, 96, 0, 0, None, 0, None, None, None, None)
    assert (null_code, shape_code) == (-1, -2)                          # the unfused sibling's codes: PECLR_ERR_NULL / _SHAPE
    assert gemm(ss=None) == null_code and conv(ss=None) == null_code
    assert gemm(a=None) == null_code
    assert gemm(n=96) == shape_code and gemm(k=48) == shape_code
    assert conv(taps=4) == shape_code and conv(cout=96) == shape_code and conv(cin=48) == shape_code
    assert conv(taps=1, stride=1) == shape_code                         # (1x1 / stride 1 is peclr_gemm_h_bnact's)
    assert L.peclr_gemm_h_bnact(1, 256, 128, 64, p, 64, p, p, 128, None, 128, p + 4, 1, 0, None) == ALIGN       # the table: 16-byte reads
    assert L.peclr_conv_h_bnact(1, 1, 8, 8, 64, 64, 9, 1, p, p, p, 0, p, p + 4, 1, None) == ALIGN
    assert L.peclr_gemm_h_bnact(1, 256, 128, 64, p, 64, p, p, 128, None, 128, p, 1, 64, None) == UNSUPPORTED    # tile_rows
    assert L.peclr_gemm_h_bnact(7, 256, 128, 64, p, 64, p, p, 128, None, 128, p, 1, 0, None) == UNSUPPORTED     # dtype
    assert L.peclr_bn2d_eval_tables(None, 3, 192, None) == null_code
    assert L.peclr_bn2d_eval_tables(p, 0, 192, None) == shape_code and L.peclr_bn2d_eval_tables(p, 3, 2, None) == shape_code


def test_predictor_precision_argument():
    from peclr_amd import _capi, pose

    model = pose.RN25DwMLPref("rn50").eval()
    for bad in ("int8", "fp64", 8, None, True, 16.0):
        with pytest.raises(ValueError, match="precision"):
            pose.FreiHANDPredictor(model, precision=bad)
    for good in ("fp32", 32, "bf16", "fp16", 16):
        with pytest.raises(_capi.PeclrHipError, match="no CPU path"):   # a CPU model is still refused, whatever the precision
            pose.FreiHANDPredictor(model, precision=good)
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        pose.FreiHANDPredictor(model)
    assert pose.FreiHANDPredictor.PRECISIONS[16] is torch.float16 and pose.FreiHANDPredictor.PRECISIONS["fp32"] is None


def test_wrappers_refuse_cpu_tensors():
    from peclr_amd import _capi

    a = torch.zeros(256, 64, dtype=torch.bfloat16)
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        _capi.gemm_h_bnact(a, torch.zeros(1, dtype=torch.uint8), 128, torch.zeros(2, 128))
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        _capi.conv_h_bnact(torch.zeros(1, 64, 8, 8, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.uint8), 64, torch.zeros(2, 64))
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        _capi.bn2d_eval_tables([(torch.ones(64), torch.zeros(64), torch.zeros(64), torch.ones(64), 1e-5)])
