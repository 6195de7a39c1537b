"""Mixed-size batches through csrc/augment.hip: every view of every sample of a ragged batch equals, bit for bit and
stage by stage, the NumPy restatement (oracle/augment_oracle.py, tests/augment_ext_ref.py) rendered from that sample's
image alone; every cv::resize path and the unaligned packed layout through hand-made records; the ragged and the
uniform path on the same images; and a mixed batch driving a training step."""
import random

import numpy as np
import pytest
import torch

from oracle import augment_oracle as A
from tests import augment_ext_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEW = ("sobel_filter", "cut_out", "gaussian_blur", "gaussian_noise", "color_drop")
# 37 x 53 is narrower than one 64-wide block and has an odd byte size (everything after it is misaligned); 480 x 640
# sets the grid for everyone else; 224 x 224 comes twice, at different batch positions
SIZES = [(224, 224), (37, 53), (240, 320), (129, 67), (480, 640), (224, 224)]


def synth_image(seed, hw):
    """Smooth structure + texture, so filtering and interpolation errors would show (as in test_augment_gpu.py)."""
    g = np.random.default_rng(seed)
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 120 * np.sin(xx / 17.0 + seed), 127 + 120 * np.cos(yy / 11.0), 60 + (xx + yy) % 190], axis=2)
    return np.clip(base + g.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def joints_for(sizes, seed=0):
    """Joints around each image's centre with a spread of a tenth of its shorter side: no sample draws an empty crop."""
    g = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([np.concatenate([g.normal((w / 2, h / 2), min(h, w) / 10, (21, 2)),
                                                      g.normal(0, 1, (21, 1))], axis=1) for h, w in sizes])).float()


_IMAGES = {}


def images_for(sizes):
    key = tuple(sizes)
    if key not in _IMAGES:
        _IMAGES[key] = [synth_image(20 + i, hw) for i, hw in enumerate(sizes)]
    return _IMAGES[key]


def warp_with_inverse(image, minv, region):
    """oracle warp driven by the already-inverted matrix (what the product hands to the kernel)."""
    orig = A.invert_affine
    try:
        A.invert_affine = lambda m: np.asarray(minv, dtype=np.float64)
        return A.warp_affine_u8(image, np.eye(2, 3), region=region)
    finally:
        A.invert_affine = orig


def test_recipe_flags_mixed_batch_bit_exact_stage_by_stage():
    from peclr_amd import RaggedImages, _capi
    from peclr_amd.augment import IMAGENET_MEAN, IMAGENET_STD, TwoViewAugmenter

    images, joints = images_for(SIZES), joints_for(SIZES, 1)
    aug = TwoViewAugmenter(rng=random.Random(11))
    params, views = aug.sample_batch(joints, SIZES)
    ragged = RaggedImages.from_list(images, DEV)
    assert ragged.data.is_cuda and ragged.data.numel() == sum(h * w * 3 for h, w in SIZES)
    geom, wins = aug.ragged_tables(SIZES, ragged.offsets, views)
    rw, rh = aug.params["resize_shape"]
    b = len(SIZES)
    for nhwc in (True, False):
        out, crops, tab = _capi.augment_views_ragged(ragged.data, geom, wins, params.to(DEV), (rh, rw), IMAGENET_MEAN,
                                                     IMAGENET_STD, channels_last=nhwc)
        assert out.shape == (2 * b, 3, rh, rw)
        assert out.is_contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format)
        assert crops.numel() == sum(w["crop"][2] * w["crop"][3] * 3 for vs in views for w in vs)  # the packed sum
        for v in (0, 1):
            for i in range(b):
                w = views[v][i]
                x0, y0, cw, ch = w["crop"]
                win = _capi.ragged_window(crops, tab, v, i).cpu().numpy()
                assert win.shape == (ch, cw, 3)
                ref_win = warp_with_inverse(images[i], np.array(w["minv"]).reshape(2, 3), (x0, y0, cw, ch))
                assert np.array_equal(win, ref_win), f"window, view {v} sample {i}"
                img = A.color_jitter_u8(A.resize_area_u8(ref_win, (rw, rh)), w["h"], w["s"], w["a"], w["b"])
                got = out[v * b + i].cpu().numpy()
                assert np.array_equal(got, A.to_tensor_normalize(img)), f"view {v} sample {i}"


def test_all_ten_flags_mixed_batch_bit_exact_stage_by_stage():
    from peclr_amd import RaggedImages, _capi
    from peclr_amd.augment import (EXT_BLUR, EXT_COLOR_DROP, EXT_CUT_OUT, EXT_NOISE, EXT_SOBEL, IMAGENET_MEAN, IMAGENET_STD,
                                   RECIPE_FLAGS, TwoViewAugmenter, blur_ksize, noise_cdf_table)

    images, joints = images_for(SIZES), joints_for(SIZES, 2)
    flags = dict(RECIPE_FLAGS, **{k: True for k in NEW})
    aug = TwoViewAugmenter(flags, {"resize_shape": [96, 96]}, rng=random.Random(5), np_rng=np.random.RandomState(5),
                           extended=True, noise_seed=4242)
    params, views = aug.sample_batch(joints, SIZES)
    # not vacuous: every one of the five is drawn somewhere, blur for samples of different kernel lengths
    drawn = [[aug.ext_flags(w) for w in vs] for vs in views]
    for bit in (EXT_SOBEL, EXT_CUT_OUT, EXT_BLUR, EXT_NOISE, EXT_COLOR_DROP):
        assert any(f & bit for fs in drawn for f in fs), bit
    blurred = {blur_ksize(SIZES[i]) for v in (0, 1) for i in range(len(SIZES)) if drawn[v][i] & EXT_BLUR}
    assert len(blurred) >= 2, blurred
    for v in (0, 1):
        for i, w in enumerate(views[v]):
            assert w["ksize"] is None or w["ksize"] == blur_ksize(SIZES[i])
    ragged = RaggedImages.from_list(images, DEV)
    geom, wins = aug.ragged_tables(SIZES, ragged.offsets, views)
    ext, coefs = aug.pack_ext(views)
    table_t, n_table = aug.noise_table()
    ops = int(np.bitwise_or.reduce(ext[..., 0].flatten().numpy()))
    table, b, call = noise_cdf_table(float(aug.params["noise_std"])), len(SIZES), 3
    refs = {(v, i): R.render_view_ext(images[i], views[v][i], (96, 96),
                                      {"table": table, "seed": aug.noise_seed, "call": call, "view": v, "sample": i}, stages=True)
            for v in (0, 1) for i in range(b)}
    for nhwc in (True, False):
        out, srcs, crops, tab = _capi.augment_views_ragged_ext(
            ragged.data, geom, wins, params.to(DEV), ext.to(DEV), coefs.to(DEV), table_t.to(DEV), n_table, aug.noise_seed,
            call, ops, (96, 96), IMAGENET_MEAN, IMAGENET_STD, channels_last=nhwc)
        assert srcs.shape == (2, ragged.data.numel())
        for (v, i), ref in refs.items():
            got_src = _capi.ragged_image(srcs[v], geom, i).cpu().numpy()
            assert np.array_equal(got_src, ref["source"]), f"stage 0, view {v} sample {i}"
            assert np.array_equal(_capi.ragged_window(crops, tab, v, i).cpu().numpy(), ref["window"]), f"window, view {v} sample {i}"
            got = out[v * b + i].cpu().numpy()
            assert np.array_equal(got, ref["tensor"]), f"view {v} sample {i}: max |d| = {np.abs(got - ref['tensor']).max()}"


def test_hand_made_records_cover_every_resize_path_and_an_identity_blur():
    """One batch, one 64 x 64 output, sources of different sizes, no rotation: windows that take cv::resize's copy,
    integer-box (2x, 3x), general-area and linear paths, and a 9 x 11 image whose blur lengths are (1, 1)."""
    from peclr_amd import RaggedImages, _capi
    from peclr_amd.augment import (EXT_BLUR, EXT_INTS, IMAGENET_MEAN, IMAGENET_STD, TwoViewAugmenter, blur_ksize,
                                   gaussian_kernel_q8)

    # source (H, W), window (x0, y0, cw, ch)
    cases = [((80, 70), (3, 5, 64, 64)), ((140, 150), (7, 2, 128, 128)), ((200, 230), (11, 6, 192, 192)),
             ((95, 107), (4, 2, 100, 90)), ((53, 41), (1, 3, 40, 50)), ((224, 224), (50, 60, 90, 40)),
             ((9, 11), (0, 0, 11, 9))]
    sizes = [c[0] for c in cases]
    assert {A.resize_mode(c[1][2], c[1][3], 64, 64) for c in cases} == {"copy", "area_fast", "area", "linear"}
    assert blur_ksize((9, 11)) == (1, 1) and gaussian_kernel_q8(1, 0.7) == [256]
    images = [synth_image(40 + i, hw) for i, hw in enumerate(sizes)]
    jit = (0.73, 0.44, 0.9, 13.0)
    recs = [[1.0, 0, 0, 0, 1.0, 0, 0.0, *map(float, win), 1.0, *jit] for _, win in cases]
    params = torch.tensor([recs], dtype=torch.float64)
    views = [[{"crop": win} for _, win in cases]]
    ragged = RaggedImages.from_list(images, DEV)
    geom, wins = TwoViewAugmenter.ragged_tables(sizes, ragged.offsets, views)
    out, crops, tab = _capi.augment_views_ragged(ragged.data, geom, wins, params.to(DEV), (64, 64), IMAGENET_MEAN,
                                                 IMAGENET_STD, channels_last=False)
    # the same batch through stage 0 with the blur bit on the 9 x 11 image alone: taps [256] twice leave it unchanged
    ext = torch.zeros((1, len(cases), EXT_INTS), dtype=torch.int32)
    ext[0, :, 6] = -1
    ext[0, 6, 0], ext[0, 6, 6] = EXT_BLUR, 0
    coefs = torch.tensor([256, 256], dtype=torch.int32)
    table = torch.zeros(1, dtype=torch.int32)
    out2, srcs, crops2, _ = _capi.augment_views_ragged_ext(ragged.data, geom, wins, params.to(DEV), ext.to(DEV), coefs.to(DEV),
                                                           table.to(DEV), 0, 1, 0, EXT_BLUR, (64, 64), IMAGENET_MEAN,
                                                           IMAGENET_STD, channels_last=False)
    for i, (hw, (x0, y0, cw, ch)) in enumerate(cases):
        win = images[i][y0:y0 + ch, x0:x0 + cw]
        assert np.array_equal(_capi.ragged_window(crops, tab, 0, i).cpu().numpy(), win), i
        ref = A.to_tensor_normalize(A.color_jitter_u8(A.resize_area_u8(win, (64, 64)), *jit))
        assert np.array_equal(out[i].cpu().numpy(), ref), (i, A.resize_mode(cw, ch, 64, 64))
        assert np.array_equal(_capi.ragged_image(srcs[0], geom, i).cpu().numpy(), images[i]), i
        assert np.array_equal(out2[i].cpu().numpy(), ref), i
    assert torch.equal(crops, crops2)


@pytest.mark.parametrize("all_ten", [False, True], ids=["recipe", "all_ten"])
def test_same_sizes_ragged_and_uniform_paths_agree(all_ten):
    from peclr_amd import TwoViewAugmenter
    from peclr_amd.augment import RECIPE_FLAGS

    b = 8
    images = images_for([(224, 224)] * b)
    g = np.random.default_rng(2)
    joints = torch.from_numpy(np.concatenate([g.normal((112, 108), 25, (b, 21, 2)), g.normal(0, 1, (b, 21, 1))], axis=2)).float()
    flags = dict(RECIPE_FLAGS, **{k: True for k in NEW}) if all_ten else None

    def make():
        return TwoViewAugmenter(flags, {"resize_shape": [64, 64]}, rng=random.Random(3), np_rng=np.random.RandomState(3),
                                extended=all_ten, noise_seed=77)

    one = make()(torch.from_numpy(np.stack(images)).to(DEV), joints)
    two = make()(list(images), joints)
    if all_ten:
        assert bool(one["blur_flag_1"].any() or one["blur_flag_2"].any())
    assert set(one) == set(two)
    for k in one:
        assert one[k].dtype == two[k].dtype and one[k].device == two[k].device and one[k].shape == two[k].shape, k
        assert torch.equal(one[k], two[k]), k
    assert one["transformed_images"].is_contiguous(memory_format=torch.channels_last)
    assert two["transformed_images"].is_contiguous(memory_format=torch.channels_last)
    assert two["transformed_image1"].data_ptr() == two["transformed_images"].data_ptr()  # both views: one buffer


def test_mixed_batch_keeps_the_recipes_two_launches_and_drives_a_training_step():
    import warnings

    from peclr_amd import Hybrid2Model, RaggedImages, Trainer, TwoViewAugmenter, _capi, hybrid2_config
    from peclr_amd.bn2d import enable_hip_batchnorm

    warnings.simplefilter("ignore")
    sizes = SIZES + [(240, 320), (129, 67)]
    b = len(sizes)
    images, joints = images_for(sizes), joints_for(sizes, 1)
    aug = TwoViewAugmenter(params={"resize_shape": [64, 64]}, rng=random.Random(3), extended=True)
    _capi.EVENT_LOG = {}
    try:
        batch = aug(RaggedImages.from_list(images, DEV), joints)
        torch.cuda.synchronize()
        launches = {k: len(v) for k, v in _capi.EVENT_LOG.items()}
    finally:
        _capi.EVENT_LOG = None
    assert launches == {"augment_warp_crop": 1, "augment_resize_color_norm": 1}
    assert batch["transformed_image1"].shape == (b, 3, 64, 64) and batch["transformed_image1"].dtype == torch.float32
    assert batch["transformed_images"].shape == (2 * b, 3, 64, 64)
    assert batch["angle_1"].dtype == torch.float64 and batch["jitter_x_2"].dtype == torch.int64
    assert batch["blur_flag_1"].dtype == torch.bool and batch["h_1"].dtype == torch.float64
    assert batch["crop_margin_scale_2"].dtype == torch.float64
    assert all(t.is_cuda for t in batch.values())
    # the same draws through the oracle, each sample from its own image alone
    rng = random.Random(3)
    for i in range(b):
        ref = A.prepare_hybrid2_sample(images[i], joints[i].numpy(), aug.flags, aug.params, rng)
        assert np.array_equal(batch["transformed_image1"][i].cpu().numpy(), ref["transformed_image1"]), i
        assert np.array_equal(batch["transformed_image2"][i].cpu().numpy(), ref["transformed_image2"]), i
        assert float(batch["angle_2"][i]) == ref["angle_2"] and int(batch["jitter_y_1"][i]) == ref["jitter_y_1"]
    torch.manual_seed(0)
    cfg = hybrid2_config(resnet_size="18", projection_head_input_dim=512, augmentation=["crop", "rotate"], batch_size=b,
                         num_samples=64, pretrained=False)
    model = Hybrid2Model(cfg).to(DEV).train()
    model.encoder = model.encoder.to(memory_format=torch.channels_last)
    enable_hip_batchnorm(model.encoder)
    trainer = Trainer(max_epochs=1).attach(model)
    out = trainer.training_micro_step(batch, 0)
    assert torch.isfinite(out["loss"]).item() and len(out) == 17
