"""The 2.5D pose head in train mode, without a GPU: the float64 restatement (tests/pose_train_ref.py) against the reference's
own float64 run recorded in g15_pose_head_train.npz, the fixture's own conditions, and the argument checks."""
import os

import numpy as np
import pytest
import torch

from tests import pose_train_ref as ref
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
RECORDED = ("kp25d", "kp3d", "zroot", "do", "0.bias", "1.weight", "1.bias", "3.bias", "4.weight", "4.bias", "6.weight", "6.bias",
            "1.running_mean", "1.running_var", "4.running_mean", "4.running_var")


@pytest.fixture(scope="module")
def g15():
    return ref.load_fixture(GOLDEN)


def test_fixture_holds_the_cases_and_stays_small(g15):
    meta, npz, _ = g15
    assert meta["cases"] == [f"train_{b}_{k}" for b in (2, 5, 37, 67) for k in ("default", "per_sample")]
    assert os.path.getsize(os.path.join(GOLDEN, "g15_pose_head_train.npz")) < 748 * 1024
    for name in meta["cases"]:
        assert meta["margin"][name] >= 1e-4, name            # no LeakyReLU input close enough to 0 to flip in fp32
        assert not any(np.isnan(v).any() for k, v in npz.items() if k.startswith(name + "/") and v.dtype.kind == "f")


def test_restatement_matches_the_reference_in_float64(g15):
    meta, npz, g11 = g15
    for name in meta["cases"]:
        r = ref.restated_case(npz, g11, name, meta["momentum"][0])
        for key in RECORDED:
            gold = npz[f"{name}/{key}"]
            if key in ("0.bias", "3.bias"):      # mathematically 0: compare on the scale of that Linear's weight gradient
                scale = meta["max_abs"][name][key.replace("bias", "weight")]
            else:
                scale = np.abs(gold).max()
            assert np.abs(r[key].reshape(gold.shape) - gold).max() <= 1e-12 * scale, (name, key)
        for key in ("0.weight", "3.weight"):    # the matrix gradients through the recorded two-sided probes
            U, V = ref.probes(*r[key].shape)
            for side, got in (("left", U @ r[key]), ("right", r[key] @ V)):
                gold = npz[f"{name}/{key}/{side}"]
                assert np.abs(got - gold).max() <= 1e-12 * np.abs(gold).max(), (name, key, side)
            assert abs(np.abs(r[key]).max() / meta["max_abs"][name][key] - 1) <= 1e-12
        for y in ("y1", "y2"):
            np.testing.assert_array_equal(np.packbits(r[y] > 0, axis=1), npz[f"{name}/{y}_positive"], err_msg=name)
            assert np.abs(r[y]).min() >= 1e-4
        assert npz[f"{name}/1.num_batches_tracked"] == npz[f"{name}/4.num_batches_tracked"]
        if name.startswith("train_5_"):          # the special rows take the branches they were built for: clamp at 50, at 4
            assert r["zr"][2] == 50.0 and r["zr"][3] == 4.0


def test_fc_rows_without_a_gradient_are_exactly_zero(g15):
    meta, npz, g11 = g15
    for name in ("train_5_per_sample", "train_37_default"):
        c = ref.case_inputs(npz, g11, name)
        _, cache = ref.forward(c["feat"], c["K"], c["fc_w"], c["fc_b"], c["mlp"])
        g25 = c["G25"].copy()
        g25[:, 63] = 0
        g = ref.backward(cache, c["G3"], g25, c["Gz"])
        assert (g["dWfc"][[2, 63]] == 0).all() and (g["dbfc"][[2, 63]] == 0).all()
        assert np.abs(g["dWfc"][[0, 1, 3, 62]]).max(axis=1).min() > 0      # the other rows are not
        # and from the recorded `do` itself: row 2 is 0, row 63 is G25's
        do = npz[f"{name}/do"]
        assert (do[:, 2] == 0).all() and (do[:, 63] == c["G25"][:, 63]).all()


def test_argument_errors_of_the_training_head_without_gpu():
    """Argument validation happens before any launch, so it is checkable on CPU."""
    from peclr_amd import _capi

    L = _capi.lib()
    fwd, bwd = L.peclr_pose_head_train_fwd_f32, L.peclr_pose_head_train_bwd_f32
    assert fwd(None, 8, 2048, None, None, None, 1e-5, 1e-5, 0.1, 0.1, None, None, None, 0, 1e-8, None, None,
               None, None, None) == -1
    assert bwd(None, 8, 2048, None, None, None, 0, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    # shape and alignment with real (host) addresses: nothing is launched or dereferenced before the checks pass
    import ctypes

    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p16 = (p + 15) // 16 * 16
    arr14 = (ctypes.c_void_p * 14)(*[p16] * 14)
    arr10 = (ctypes.c_void_p * 10)(*[p16] * 10)
    a14, a10 = ctypes.cast(arr14, ctypes.c_void_p), ctypes.cast(arr10, ctypes.c_void_p)

    def f(b, nf=2048, feat=p16, save=p16):
        return fwd(feat, b, nf, p16, p16, a14, 1e-5, 1e-5, 0.1, 0.1, p16, p16, p16, 0, 1e-8, p16, p16, p16, save, None)

    def g(b, nf=2048, save=p16, ws=p16):
        return bwd(p16, b, nf, p16, a14, p16, 0, p16, p16, save, None, None, None, ws, None, p16, p16, a10, None)

    for b in (1, 0, -3, 1025):                                  # PECLR_ERR_SHAPE: B outside [2, 1024], before any launch
        assert f(b) == g(b) == -2
    assert f(8, nf=2047) == g(8, nf=2047) == -2
    assert f(8, feat=p16 + 4) == f(8, save=p16 + 4) == g(8, save=p16 + 4) == g(8, ws=p16 + 4) == -3   # PECLR_ERR_ALIGN
    arr14[5] = None
    assert f(8) == g(8) == -1                                   # a null entry of the parameter table
    assert L.peclr_pose_head_train_launches(0, 1) == 4 and L.peclr_pose_head_train_launches(1, 1) == 6
    assert L.peclr_pose_head_train_launches(1, 0) == 5


def test_a_batch_of_one_raises_value_error_as_torch_does():
    from peclr_amd import _capi

    mlp = [torch.zeros(1)] * 14
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        _capi.pose_head_train_fwd(torch.zeros(1, 2048), None, None, mlp, (1e-5, 1e-5), (0.1, 0.1), (None, None),
                                  torch.eye(3).reshape(1, 3, 3), 1e-8)
    with pytest.raises(ValueError, match="more than 1 value per channel"):     # torch's own, for comparison
        torch.nn.BatchNorm1d(4).train()(torch.zeros(1, 4))


def test_enable_hip_training_needs_a_hip_model_and_supported_batchnorm():
    from peclr_amd import _capi
    from peclr_amd.pose import RN25DwMLPref

    m = RN25DwMLPref("rn50")
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        m.enable_hip_training()
    assert m.hip_training is False and m.enable_hip_training(False) is m
    m.zroot_ref.zroot_ref[1].momentum = None
    with pytest.raises(_capi.PeclrHipError, match="momentum=None"):
        m._check_hip_training()
    # off by default: train mode on the CPU stays on the stock path and has no `zroot` key
    m = RN25DwMLPref("rn50").train()
    out = m.head(torch.randn(3, 2048))
    assert sorted(out) == ["kp25d", "kp2d", "kp3d", "zrel"]
