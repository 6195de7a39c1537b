"""Left hands in the augmenters, host side (no GPU): the draws of a left sample are the draws on the reference loader's
`x <- W - x` joints; `mirror_camera` is float32(F K M) and the X-negated joints, bit for bit; a bad `is_left` is refused
before the first native call; and the camera convention is the predictor's."""
import random

import numpy as np
import pytest
import torch

from tests import _capi_double_left as double

SIZES = [(37, 53), (64, 64), (129, 67), (96, 130)]
LEFT = [True, False, False, True]


def joints_for(sizes, seed):
    g = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([np.concatenate([g.normal((w * 0.45, h / 2), min(h, w) / 10, (21, 2)),
                                                      g.normal(0, 1, (21, 1))], axis=1) for h, w in sizes])).float()


def flipped_joints(joints, sizes, left):
    """The loader's rule, in float32: x <- W - x for the left samples."""
    out = joints.clone()
    for i, (l, (_, w)) in enumerate(zip(left, sizes)):
        if l:
            out[i, :, 0] = w - out[i, :, 0]
    return out


def camera(hw, focal=200.0, third=(0.0, 0.0, 1.0)):
    return np.array([[focal, 0.3, hw[1] / 2 + 1.25], [0, focal * 1.01, hw[0] / 2 - 0.5], third], dtype=np.float32)


def hand(hw, seed, focal=200.0):
    """21 joints in front of the camera that project around the image centre -> float32 [21,3]."""
    g = np.random.default_rng(seed)
    z = 0.6 + 0.05 * g.standard_normal(21)
    u = 0.45 * hw[1] + min(hw) / 9 * g.standard_normal(21)
    v = 0.5 * hw[0] + min(hw) / 9 * g.standard_normal(21)
    return np.stack([(u - hw[1] / 2) * z / focal, (v - hw[0] / 2) * z / focal, z], axis=1).astype(np.float32)


@pytest.mark.parametrize("extended", [False, True], ids=["recipe", "all_ten"])
def test_left_draws_are_the_draws_on_w_minus_x_joints(extended):
    from peclr_amd.augment import RECIPE_FLAGS, TwoViewAugmenter

    flags = dict(RECIPE_FLAGS, sobel_filter=True, cut_out=True, gaussian_blur=True, gaussian_noise=True,
                 color_drop=True) if extended else None
    joints = joints_for(SIZES, 3)

    def make():
        return TwoViewAugmenter(flags, {"resize_shape": [32, 32]}, rng=random.Random(7), np_rng=np.random.RandomState(7),
                                extended=extended)

    p_left, v_left = make().sample_batch(joints, SIZES, LEFT)
    p_flip, v_flip = make().sample_batch(flipped_joints(joints, SIZES, LEFT), SIZES)
    p_none, v_none = make().sample_batch(joints, SIZES)
    assert torch.equal(p_left, p_flip) and v_left == v_flip
    assert not torch.equal(p_left, p_none), "vacuous: the flag moved no window"
    # the right samples' windows do not depend on their neighbours' flags ...
    for i, l in enumerate(LEFT):
        if not l:
            assert v_left[0][i]["crop"] == v_none[0][i]["crop"] and v_left[1][i]["crop"] == v_none[1][i]["crop"]
    # ... and None, all false and integer zeros draw what a call without the argument draws
    for flagsless in (None, [False] * 4, np.zeros(4, dtype=np.int64), torch.zeros(4, dtype=torch.bool)):
        p, v = make().sample_batch(joints, SIZES, flagsless)
        assert torch.equal(p, p_none) and v == v_none
    p_int, _ = make().sample_batch(joints, SIZES, torch.tensor([1, 0, 0, 1]))
    assert torch.equal(p_int, p_left)


def test_supervised_left_draws_are_the_draws_on_the_mirrored_camera():
    from peclr_amd.supervised import SupervisedAugmenter, mirror_camera

    K = torch.from_numpy(np.stack([camera(hw) for hw in SIZES]))
    J = torch.from_numpy(np.stack([hand(hw, 10 + i) for i, hw in enumerate(SIZES)]))
    Kf, Jf = K.clone(), J.clone()
    for i, (l, (_, w)) in enumerate(zip(LEFT, SIZES)):
        if l:
            Kf[i], Jf[i] = mirror_camera(K[i], J[i], w)

    def make():
        return SupervisedAugmenter(params={"resize_shape": [32, 32]}, rng=random.Random(5))

    p_left, v_left, t_left = make().sample_batch(K, J, SIZES, LEFT)
    p_flip, v_flip, t_flip = make().sample_batch(Kf, Jf, SIZES)
    p_none, _, _ = make().sample_batch(K, J, SIZES)
    assert torch.equal(p_left, p_flip) and v_left == v_flip and torch.equal(t_left, t_flip)
    assert not torch.equal(p_left, p_none)


def numpy_mirror(K, J, width):
    """float64 NumPy restatement of the label kernel's rule, rounded once."""
    k = np.asarray(K, dtype=np.float32).astype(np.float64)
    out = k.copy()
    for c in range(3):
        out[0, c] = np.float64(width - 1) * k[2, c] - k[0, c]
    out[:, 0] = -out[:, 0]
    j = np.asarray(J, dtype=np.float32).copy()
    j[:, 0] = -j[:, 0]
    return out.astype(np.float32), j


def test_mirror_camera_is_the_float64_rule_rounded_once():
    from peclr_amd.supervised import mirror_camera

    cases = [((37, 53), (0.0, 0.0, 1.0)), ((129, 67), (0.0, 0.0, 1.0)), ((480, 640), (1e-4, -2e-4, 0.97)),
             ((96, 130), (0.003, 0.001, 1.02))]
    ks, js, ws = [], [], []
    for i, (hw, third) in enumerate(cases):
        g = np.random.default_rng(30 + i)
        k = camera(hw, focal=float(g.uniform(150, 700)), third=third)
        j = hand(hw, 40 + i)
        got_k, got_j = mirror_camera(k, j, hw[1])
        want_k, want_j = numpy_mirror(k, j, hw[1])
        assert got_k.dtype == torch.float32 and got_j.dtype == torch.float32
        assert np.array_equal(got_k.numpy().view(np.uint32), want_k.view(np.uint32)), hw
        assert np.array_equal(got_j.numpy().view(np.uint32), want_j.view(np.uint32)), hw
        # the rounding happened ONCE: it is the float32 of the exact float64 value, not of a float32 product
        exact = np.float64(hw[1] - 1) * np.float64(k[2, 2]) - np.float64(k[0, 2])
        assert float(got_k[0, 2]) == float(np.float32(exact))
        ks.append(k), js.append(j), ws.append(hw[1])
    assert any(c[1][0] != 0 for c in cases), "a K with a non-trivial third row"
    # batched, one width per sample, tensors or arrays alike
    bk, bj = mirror_camera(torch.from_numpy(np.stack(ks)), np.stack(js), torch.tensor(ws))
    for i in range(len(cases)):
        one_k, one_j = mirror_camera(ks[i], js[i], ws[i])
        assert torch.equal(bk[i], one_k) and torch.equal(bj[i], one_j)
    # the inputs are left alone, and mirroring twice at the same width returns the joints
    k0 = ks[0].copy()
    mirror_camera(ks[0], js[0], ws[0])
    assert np.array_equal(ks[0], k0)
    assert torch.equal(mirror_camera(bk, bj, torch.tensor(ws))[1], torch.from_numpy(np.stack(js)))


def test_mirror_camera_is_the_predictors_convention():
    """`predict.flip_camera` (what HandPosePredictor hands its crop kernel's check) and `mirror_camera` are the same matrix,
    and it does what the convention says: the X-negated point projects to (W - 1) - u."""
    from peclr_amd.predict import flip_camera
    from peclr_amd.supervised import mirror_camera

    g = np.random.default_rng(3)
    for hw, third in (((37, 53), (0.0, 0.0, 1.0)), ((480, 640), (1e-4, -2e-4, 0.97))):
        w = hw[1]
        k = camera(hw, focal=310.0, third=third)
        kf32, _ = mirror_camera(k, np.zeros((21, 3), np.float32), w)
        kf64 = flip_camera(k, w)
        assert np.array_equal(kf32.numpy(), kf64.astype(np.float32))
        k64 = k.astype(np.float64)
        pts = np.stack([g.uniform(-0.2, 0.2, 50), g.uniform(-0.2, 0.2, 50), g.uniform(0.4, 0.9, 50)], axis=1)
        neg = pts * np.array([-1.0, 1.0, 1.0])
        proj = lambda m, p: (p @ m.T)[:, :2] / (p @ m.T)[:, 2:]  # noqa: E731
        uv, uv_f = proj(k64, pts), proj(kf64, neg)
        assert np.max(np.abs(uv_f[:, 0] - ((w - 1) - uv[:, 0]))) < 1e-9 * w
        assert np.max(np.abs(uv_f[:, 1] - uv[:, 1])) < 1e-9 * w
        # ... and with the float32 matrix, within the rounding of its entries: 2^-24 relative each, through u = h0 / h2
        kf = kf32.numpy().astype(np.float64)
        h = neg @ kf.T
        got = h[:, 0] / h[:, 2]
        bound = 2.0 ** -24 * (np.abs(neg) @ np.abs(kf[0]) + np.abs(got) * (np.abs(neg) @ np.abs(kf[2]))) / np.abs(h[:, 2])
        assert np.all(np.abs(got - ((w - 1) - uv[:, 0])) <= 1.01 * bound + 1e-9 * w)


BAD = [([True, False, True], ValueError, "entries"), ([True] * 5, ValueError, "entries"),
       (np.zeros((2, 2), dtype=bool), ValueError, "entries"), ([0.0, 1.0, 0.0, 1.0], TypeError, "bools or integers"),
       ([0, 2, 0, 1], ValueError, "0 or 1"), (torch.tensor([0, -1, 0, 1]), ValueError, "0 or 1"),
       (["a", "b", "c", "d"], TypeError, "bools or integers")]


@pytest.mark.parametrize("bad, exc, match", BAD, ids=[str(i) for i in range(len(BAD))])
def test_a_bad_is_left_is_refused_before_any_native_call(monkeypatch, bad, exc, match):
    from peclr_amd import SupervisedAugmenter, TwoViewAugmenter

    calls = double.install(monkeypatch)
    images = [np.zeros((h, w, 3), dtype=np.uint8) for h, w in SIZES]
    joints = joints_for(SIZES, 1)
    K = torch.from_numpy(np.stack([camera(hw) for hw in SIZES]))
    J = torch.from_numpy(np.stack([hand(hw, 10 + i) for i, hw in enumerate(SIZES)]))
    two, sup = TwoViewAugmenter(rng=random.Random(1)), SupervisedAugmenter(rng=random.Random(1))
    state = two.rng.getstate()
    with pytest.raises(exc, match=match):
        two(images, joints, is_left=bad)
    with pytest.raises(exc, match=match):
        two(torch.zeros((4, 64, 64, 3), dtype=torch.uint8), joints, is_left=bad)      # the dense path
    with pytest.raises(exc, match=match):
        two.sample_batch(joints, SIZES, bad)
    with pytest.raises(exc, match=match):
        sup(images, K, J, is_left=bad)
    assert calls == [] and two.rng.getstate() == state, "refused before a draw and before a native call"


def test_the_double_sees_a_good_call(monkeypatch):
    """... so the empty list above means something: a well-formed call does reach the wrappers, with the table."""
    from peclr_amd import TwoViewAugmenter, _capi

    calls = double.install(monkeypatch)
    seen = {}

    def augment_views(*args, **kwargs):
        seen.clear()
        seen.update(kwargs)
        raise double.NativeCall("augment_views")

    monkeypatch.setattr(_capi, "augment_views", augment_views)
    images = torch.zeros((4, 64, 64, 3), dtype=torch.uint8)
    joints = joints_for([(64, 64)] * 4, 1)
    with pytest.raises(double.NativeCall):
        TwoViewAugmenter(rng=random.Random(1))(images, joints, is_left=[False] * 4)
    assert "mirror" not in seen, "all false: the call of before, without the table"
    with pytest.raises(double.NativeCall):
        TwoViewAugmenter(rng=random.Random(1))(images, joints, is_left=[True, False, False, True])
    assert seen["mirror"].tolist() == [64, 0, 0, 64] and seen["mirror"].dtype == torch.int32
    assert calls == []
