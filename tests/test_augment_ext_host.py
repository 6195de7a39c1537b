"""TwoViewAugmenter(extended=True), host side: the reference's draw order for sobel_filter, cut_out,
gaussian_blur, gaussian_noise and color_drop (pinned by tests/golden/g10_augment_ext_params.json, captured
from the reference's own code), the fixed-point Gaussian taps, the noise table, and known answers for the
NumPy restatement of the new pixel operations (tests/augment_ext_ref.py)."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

from tests import augment_ext_ref as R
from tests.conftest import GOLDEN as GOLDEN_DIR

ALL_FLAGS = ["color_drop", "color_jitter", "crop", "cut_out", "gaussian_blur", "random_crop", "resize", "rotate",
             "gaussian_noise", "sobel_filter"]

with open(os.path.join(GOLDEN_DIR, "g10_augment_ext_params.json")) as f:
    CASES = json.load(f)["cases"]


def draw_case(case):
    from peclr_amd.augment import TwoViewAugmenter, convert_to_2_5d

    flags = {k: k in case["flags_on"] for k in ALL_FLAGS}
    rng, np_rng = random.Random(case["seed"]), np.random.RandomState(case["seed"])
    aug = TwoViewAugmenter(flags, case["params"], rng=rng, np_rng=np_rng, extended=True)
    j25, _ = convert_to_2_5d(torch.tensor(case["K"], dtype=torch.float32), torch.tensor(case["joints3D"], dtype=torch.float32))
    params, views = aug.sample_batch(j25[None], tuple(case["image_hw"]))
    return aug, params, views, rng, np_rng


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_extended_parameters_equal_reference(case):
    aug, params, views, rng, np_rng = draw_case(case)
    for v, gv in enumerate(case["views"]):
        w = views[v][0]
        assert w["sobel"] == gv["sobel"] and w["noise"] == gv["noise"] and w["color_drop"] == gv["color_drop"]
        assert (w["cut_out"] is not None) == gv["cut_out"] and (w["sigma"] is not None) == gv["blur"]
        assert w["blur_flag"] == gv["blur"]
        if gv["cut_out"]:
            c = w["cut_out"]
            assert c["joint"] == gv["cut_out_joint"] and c["fill"] == gv["cut_out_fill"]
            assert list(c["rows"]) == gv["rows"] and list(c["cols"]) == gv["cols"]
        if gv["blur"]:
            assert list(w["ksize"]) == gv["blur_ksize"] and w["sigma"] == gv["blur_sigma"]
    # the emitted dict, every key, and nothing else
    got = aug.collate(views)
    assert set(got) == set(case["emitted"])
    for k, e in case["emitted"].items():
        assert got[k][0].item() == e["value"], k
        assert got[k].dtype == {"bool": torch.bool, "int": torch.int64, "float": torch.float64}[e["type"]], k
    # the same NUMBER of draws from both generators
    assert rng.random() == case["probes"]["random"]
    assert int(np_rng.randint(2 ** 31)) == case["probes"]["np_randint"]


def test_ext_records_point_at_the_right_taps():
    from peclr_amd.augment import EXT_INTS, TwoViewAugmenter, gaussian_kernel_q8

    case = next(c for c in CASES if c["name"] == "all_ten_480x640")
    aug, params, views, _, _ = draw_case(case)
    ext, coefs = TwoViewAugmenter.pack_ext(views)
    assert ext.shape == (2, 1, EXT_INTS) and ext.dtype == torch.int32
    for v in (0, 1):
        w, rec = views[v][0], ext[v, 0].tolist()
        assert rec[0] == TwoViewAugmenter.ext_flags(w)
        if w["cut_out"]:
            assert rec[1:6] == [*w["cut_out"]["rows"], *w["cut_out"]["cols"], w["cut_out"]["fill"]]
        kx, ky = w["ksize"]
        assert coefs[rec[6]:rec[6] + kx].tolist() == gaussian_kernel_q8(kx, w["sigma"])
        assert coefs[rec[6] + kx:rec[6] + kx + ky].tolist() == gaussian_kernel_q8(ky, w["sigma"])


def test_extended_false_still_rejects_the_five_flags():
    from peclr_amd.augment import TwoViewAugmenter

    for k in ("sobel_filter", "cut_out", "gaussian_blur", "gaussian_noise", "color_drop"):
        with pytest.raises(NotImplementedError, match=k):
            TwoViewAugmenter({"resize": True, k: True})
        TwoViewAugmenter({"resize": True, k: True}, extended=True)
    with pytest.raises(ValueError, match="sobel_kernel"):
        TwoViewAugmenter({"resize": True, "sobel_filter": True}, {"sobel_kernel": 5}, extended=True)


def test_blur_ksize_rule_and_swap():
    from peclr_amd.augment import blur_ksize

    assert blur_ksize((224, 224)) == (23, 23)
    assert blur_ksize((240, 320)) == (25, 33)      # horizontal length from H, vertical from W
    assert blur_ksize((480, 640)) == (49, 65)
    assert blur_ksize((9, 5)) == (1, 1)
    for h in range(1, 2049):
        k = blur_ksize((h, h))[0]
        assert k % 2 == 1 and k <= 257 and k // 2 < max(h, 2)


# ------------------------------------------------------------------ Gaussian taps, noise table
@pytest.mark.parametrize("n", [1, 3, 5, 7, 23, 25, 33, 49, 65, 205])
@pytest.mark.parametrize("sigma", [0.1, 0.37, 1.0, 1.55, 2.0])
def test_gaussian_taps(n, sigma):
    from peclr_amd.augment import gaussian_kernel_q8

    taps = gaussian_kernel_q8(n, sigma)
    assert len(taps) == n and sum(taps) == 256 and taps == taps[::-1] and min(taps) >= 0
    x = np.arange(n) - (n - 1) / 2
    g = np.exp(-x * x / (2 * sigma * sigma))
    g /= g.sum()
    assert np.abs(np.array(taps) / 256 - g).max() <= 1 / 256 + 1e-12
    if n == 1:
        assert taps == [256]


def test_noise_table_reproduces_the_clamped_rounded_normal():
    from peclr_amd.augment import noise_cdf_table

    for std in (25, 3.0, 90):
        t = noise_cdf_table(std)
        assert 0 < len(t) <= 255 and all(a <= b for a, b in zip(t, t[1:])) and t[-1] < 2 ** 32
        edges = [0] + t + [2 ** 32]
        for k in range(len(edges) - 1):
            lo = 0.0 if k == 0 else 0.5 * math.erfc(-(k - 0.5) / (std * math.sqrt(2)))
            hi = 1.0 if k == 255 else 0.5 * math.erfc(-(k + 0.5) / (std * math.sqrt(2)))
            p = (hi - lo) if k < len(t) else 1.0 - lo  # the last bin takes the whole upper tail
            assert abs((edges[k + 1] - edges[k]) / 2 ** 32 - p) <= 2 ** -32 + 1e-15, (std, k)
    assert 140 <= len(noise_cdf_table(25)) <= 170
    assert noise_cdf_table(0) == []


def test_philox_known_answers_and_noise_mapping():
    z = R.philox4x32_10(np.zeros((1, 4), np.uint32), (0, 0))[0]
    assert [int(v) for v in z] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = R.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0]
    assert [int(v) for v in f] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    table = [10, 20, 20, 30]
    assert R.noise_values(table, np.array([0, 9, 10, 19, 20, 29, 30, 2 ** 32 - 1])).tolist() == [0, 0, 1, 1, 3, 3, 4, 4]


# ------------------------------------------------------------------ restatement known answers
def test_gray_of_the_primaries():
    img = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]]], dtype=np.uint8)
    assert R.gray_u8(img).tolist() == [[29, 150, 76, 255, 0]]
    drop = R.color_drop_u8(img)
    assert drop[0, :, 0].tolist() == [29, 150, 76, 255, 0] and (drop == drop[..., :1]).all()


def test_sobel_ramp_reflect101_and_wrap():
    ramp = np.repeat(np.repeat(np.arange(20, dtype=np.uint8)[None, :, None], 9, 0), 3, 2)  # gray = x
    s = R.sobel_u8(ramp)
    assert (s[:, 1:-1] == 8).all() and (s[:, 0] == 0).all() and (s[:, -1] == 0).all()
    assert (s == s[..., :1]).all()
    assert R.sobel_sum(R.gray_u8(ramp))[0, 0] == 0
    # a negative sum stores its low byte: a bright pixel left of a dark one gives dx < 0
    img = np.zeros((3, 3, 3), np.uint8)
    img[:, 0] = 255
    v = int(R.sobel_sum(R.gray_u8(img))[1, 1])
    assert v == -1020 and int(R.sobel_u8(img)[1, 1, 0]) == v % 256
    assert -300 % 256 == 212


def test_blur_of_a_constant_is_the_constant():
    from peclr_amd.augment import gaussian_kernel_q8

    for value in (0, 1, 77, 254, 255):
        img = np.full((31, 47, 3), value, np.uint8)
        for kx, ky, sigma in ((23, 23, 0.3), (25, 33, 1.9), (3, 1, 1.0), (49, 65, 2.0)):
            out = R.gaussian_blur_u8(img, gaussian_kernel_q8(kx, sigma), gaussian_kernel_q8(ky, sigma))
            assert (out == value).all(), (value, kx, ky)


def test_blur_identity_taps_and_reflection():
    g = np.random.default_rng(0)
    img = g.integers(0, 256, (12, 9, 3), dtype=np.uint8)
    assert np.array_equal(R.gaussian_blur_u8(img, [256], [256]), img)
    # a single off-centre tap moves the image by one pixel with a reflect-101 border
    out = R.gaussian_blur_u8(img, [0, 0, 256], [256])
    assert np.array_equal(out[:, :-1], img[:, 1:]) and np.array_equal(out[:, -1], img[:, -2])
    assert R.reflect101(np.array([-3, -1, 0, 4, 5, 7]), 5).tolist() == [3, 1, 0, 4, 3, 1]
    assert R.reflect101(np.array([-2, 3]), 1).tolist() == [0, 0]


def test_cut_out_fills_the_box_only():
    img = np.zeros((10, 12, 3), np.uint8)
    out = R.cut_out_u8(img, (2, 5), (3, 10), 200)
    assert (out[2:5, 3:10] == 200).all() and out.sum() == 200 * 3 * 7 * 3 and img.sum() == 0
