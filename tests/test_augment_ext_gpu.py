"""TwoViewAugmenter(extended=True) on the GPU: the stage-0 sources, the crop windows and the final float32
tensors of csrc/augment.hip equal the NumPy restatement (tests/augment_ext_ref.py on top of
oracle/augment_oracle.py) bit for bit, noise included; the noise stream's determinism and distribution;
the recipe path unchanged; and an all-ten-flags batch driving a training step."""
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import augment_ext_ref as R
from tests.conftest import GOLDEN as GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL_FLAGS = ["color_drop", "color_jitter", "crop", "cut_out", "gaussian_blur", "random_crop", "resize", "rotate",
             "gaussian_noise", "sobel_filter"]
NEW = ("sobel_filter", "cut_out", "gaussian_blur", "gaussian_noise", "color_drop")

with open(os.path.join(GOLDEN_DIR, "g10_augment_ext_params.json")) as f:
    CASES = json.load(f)["cases"]


def synth_image(seed, hw):
    """Smooth structure + texture, so filtering and interpolation errors would show."""
    g = np.random.default_rng(seed)
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 120 * np.sin(xx / 17.0 + seed), 127 + 120 * np.cos(yy / 11.0), 60 + (xx + yy) % 190], axis=2)
    return np.clip(base + g.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def launch(aug, images_np, params, views, channels_last, call=0):
    from peclr_amd import _capi
    from peclr_amd.augment import IMAGENET_MEAN, IMAGENET_STD, blur_ksize

    b, h, w, _ = images_np.shape
    ext, coefs = aug.pack_ext(views)
    table, n_table = aug.noise_table()
    ops = int(np.bitwise_or.reduce(ext[..., 0].flatten().numpy()))
    rw, rh = aug.params["resize_shape"]
    return _capi.augment_views_ext(torch.from_numpy(images_np).to(DEV), params.to(DEV), ext.to(DEV), coefs.to(DEV),
                                   blur_ksize((h, w)), table.to(DEV), n_table, aug.noise_seed, call, ops, (rh, rw),
                                   IMAGENET_MEAN, IMAGENET_STD, channels_last=channels_last)


def check_against_restatement(aug, images_np, views, result, call=0):
    from peclr_amd.augment import noise_cdf_table

    out, srcs, crops = result
    b = images_np.shape[0]
    table = noise_cdf_table(float(aug.params["noise_std"]))
    for v in (0, 1):
        for i in range(b):
            w = views[v][i]
            ref = R.render_view_ext(images_np[i], w, tuple(aug.params["resize_shape"]),
                                    {"table": table, "seed": aug.noise_seed, "call": call, "view": v, "sample": i}, stages=True)
            if srcs is not None:
                assert np.array_equal(srcs[v, i].cpu().numpy(), ref["source"]), f"stage 0, view {v} sample {i}"
            x0, y0, cw, ch = w["crop"]
            assert np.array_equal(crops[v, i, :ch, :cw].cpu().numpy(), ref["window"]), f"window, view {v} sample {i}"
            got = out[v * b + i].cpu().numpy()
            assert np.array_equal(got, ref["tensor"]), f"view {v} sample {i}: max |d| = {np.abs(got - ref['tensor']).max()}"


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_pipeline_bit_exact_on_reference_parameter_sets(case):
    from peclr_amd.augment import TwoViewAugmenter, convert_to_2_5d

    flags = {k: k in case["flags_on"] for k in ALL_FLAGS}
    aug = TwoViewAugmenter(flags, case["params"], rng=random.Random(case["seed"]),
                           np_rng=np.random.RandomState(case["seed"]), extended=True, noise_seed=case["seed"])
    hw = tuple(case["image_hw"])
    image = synth_image(case["seed"], hw)[None]
    j25, _ = convert_to_2_5d(torch.tensor(case["K"], dtype=torch.float32), torch.tensor(case["joints3D"], dtype=torch.float32))
    params, views = aug.sample_batch(j25[None], hw)
    for nhwc in (True, False):
        res = launch(aug, image, params, views, nhwc, call=3)
        assert res[0].is_contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format)
        check_against_restatement(aug, image, views, res, call=3)


@pytest.mark.parametrize("hw", [(224, 224), (240, 320), (480, 640)], ids=["224", "240x320", "480x640"])
def test_synthetic_batches_all_ten_flags_bit_exact(hw):
    from peclr_amd.augment import RECIPE_FLAGS, TwoViewAugmenter, blur_ksize

    b = 4
    g = np.random.default_rng(hw[0])
    images = np.stack([synth_image(10 + i, hw) for i in range(b)])
    centre = (hw[1] / 2, hw[0] / 2)
    joints = torch.from_numpy(np.concatenate([g.normal(centre, hw[0] / 9, (b, 21, 2)), g.normal(0, 1, (b, 21, 1))], 2)).float()
    flags = dict(RECIPE_FLAGS, **{k: True for k in NEW})
    aug = TwoViewAugmenter(flags, {"cut_out_fraction": [0.1, 0.3]}, rng=random.Random(hw[1]),
                           np_rng=np.random.RandomState(hw[1]), extended=True, noise_seed=99)
    params, views = aug.sample_batch(joints, hw)
    for v in (0, 1):  # every operation on in every view: the synthetic batches cover each path at every sample
        for w in views[v]:
            w["sobel"] = w["noise"] = w["color_drop"] = True
            if w["sigma"] is None:
                w["sigma"], w["ksize"] = 1.3, blur_ksize(hw)
            if w["cut_out"] is None:
                w["cut_out"] = {"joint": 0, "ratio": 0.2, "rows": (hw[0] // 3, hw[0] // 2), "cols": (0, hw[1] // 4), "fill": 17}
    views[1][1]["sobel"] = False  # and a mix within the batch
    views[0][2]["sigma"] = None
    for nhwc in (True, False):
        check_against_restatement(aug, images, views, launch(aug, images, params, views, nhwc, call=7), call=7)


def test_noise_is_deterministic_per_seed_and_call_and_has_the_table_distribution():
    from peclr_amd.augment import IMAGENET_MEAN, IMAGENET_STD, TwoViewAugmenter, noise_cdf_table

    b = 32  # 64 images
    g = np.random.default_rng(4)
    images = np.stack([synth_image(i, (160, 160)) for i in range(b)])
    joints = torch.from_numpy(np.concatenate([g.normal((80, 80), 18, (b, 21, 2)), g.normal(0, 1, (b, 21, 1))], 2)).float()
    aug = TwoViewAugmenter({"resize": True, "crop": True, "gaussian_noise": True}, rng=random.Random(5),
                           np_rng=np.random.RandomState(5), extended=True, noise_seed=1234)
    params, views = aug.sample_batch(joints, (160, 160))
    for vs in views:
        for w in vs:
            w["noise"] = True
    a = launch(aug, images, params, views, True, call=0)[0]
    assert torch.equal(a, launch(aug, images, params, views, True, call=0)[0])
    assert not torch.equal(a, launch(aug, images, params, views, True, call=1)[0])
    aug.noise_seed = 1235
    assert not torch.equal(a, launch(aug, images, params, views, True, call=0)[0])
    aug.noise_seed = 1234
    for vs in views:
        for w in vs:
            w["noise"] = False
    clean = launch(aug, images, params, views, True, call=0)[0]

    def to_u8(t):
        mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float64, device=t.device)[None, :, None, None]
        std = torch.tensor(IMAGENET_STD, dtype=torch.float64, device=t.device)[None, :, None, None]
        return torch.round((t.double() * std + mean) * 255).long()

    assert torch.equal(to_u8(clean), to_u8(clean).clamp(0, 255))
    n = ((to_u8(a) - to_u8(clean)) % 256).flatten().cpu().numpy()
    hist = np.bincount(n, minlength=256) / n.size
    t = [0] + noise_cdf_table(25.0) + [2 ** 32]
    p = np.zeros(256)
    p[:len(t) - 1] = np.diff(np.array(t, dtype=np.float64)) / 2 ** 32
    assert np.abs(hist - p).max() < 0.005, np.abs(hist - p).max()


def test_recipe_path_unchanged_when_no_extended_flag_is_on():
    from peclr_amd import TwoViewAugmenter, _capi

    b = 6
    g = np.random.default_rng(8)
    images = torch.from_numpy(np.stack([synth_image(i, (224, 224)) for i in range(b)])).to(DEV)
    joints = torch.from_numpy(np.concatenate([g.normal((112, 108), 25, (b, 21, 2)), g.normal(0, 1, (b, 21, 1))], 2)).float()
    outs, logs = [], []
    for extended in (False, True):
        aug = TwoViewAugmenter(rng=random.Random(3), extended=extended)
        _capi.EVENT_LOG = {}
        try:
            outs.append(aug(images, joints))
            torch.cuda.synchronize()
            logs.append({k: len(v) for k, v in _capi.EVENT_LOG.items()})
        finally:
            _capi.EVENT_LOG = None
    assert set(outs[0]) == set(outs[1])
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert logs[0] == logs[1] == {"augment_warp_crop": 1, "augment_resize_color_norm": 1}


def test_all_ten_flags_batch_drives_a_training_step():
    import warnings

    from peclr_amd import Hybrid2Model, Trainer, TwoViewAugmenter, hybrid2_config
    from peclr_amd.augment import RECIPE_FLAGS, noise_cdf_table
    from peclr_amd.bn2d import enable_hip_batchnorm

    warnings.simplefilter("ignore")
    b = 8
    g = np.random.default_rng(2)
    images_np = np.stack([synth_image(i, (224, 224)) for i in range(b)])
    joints = torch.from_numpy(np.concatenate([g.normal((112, 108), 25, (b, 21, 2)), g.normal(0, 1, (b, 21, 1))], axis=2)).float()
    flags = dict(RECIPE_FLAGS, **{k: True for k in NEW})
    aug = TwoViewAugmenter(flags, {"resize_shape": [64, 64]}, rng=random.Random(3), np_rng=np.random.RandomState(3),
                           extended=True, noise_seed=77)
    batch = aug(torch.from_numpy(images_np).to(DEV), joints)
    assert batch["transformed_image1"].shape == (b, 3, 64, 64) and batch["blur_flag_1"].dtype == torch.bool
    assert bool(batch["blur_flag_1"].any() or batch["blur_flag_2"].any())
    # the same draws through the restatement give the same tensors (the call index was 0)
    aug2 = TwoViewAugmenter(flags, {"resize_shape": [64, 64]}, rng=random.Random(3), np_rng=np.random.RandomState(3),
                            extended=True, noise_seed=77)
    _, views = aug2.sample_batch(joints, (224, 224))
    for v in (0, 1):
        assert batch[f"blur_flag_{v + 1}"].cpu().tolist() == [w["sigma"] is not None for w in views[v]]
    table = noise_cdf_table(25.0)
    for v in (0, 1):
        for i in range(b):
            ref = R.render_view_ext(images_np[i], views[v][i], (64, 64),
                                    {"table": table, "seed": 77, "call": 0, "view": v, "sample": i})
            assert np.array_equal(batch[f"transformed_image{v + 1}"][i].cpu().numpy(), ref), (v, i)
    assert aug.noise_call == 1
    torch.manual_seed(0)
    cfg = hybrid2_config(resnet_size="18", projection_head_input_dim=512, augmentation=["crop", "rotate"], batch_size=b,
                         num_samples=64, pretrained=False)
    model = Hybrid2Model(cfg).to(DEV).train()
    model.encoder = model.encoder.to(memory_format=torch.channels_last)
    enable_hip_batchnorm(model.encoder)
    trainer = Trainer(max_epochs=1).attach(model)
    out = trainer.training_micro_step(batch, 0)
    assert torch.isfinite(out["loss"]).item() and len(out) == 17
