"""Left hands through csrc/augment.hip and csrc/labels.hip: a sample flagged `is_left` comes out, bit for bit and stage by stage,
as the NumPy restatement (oracle/augment_oracle.py, tests/augment_ext_ref.py) renders `img[:, ::-1]` -- the reference loader's
cv2.flip(img, 1) -- while its right-handed neighbours in the same launch come out from `img`; the labels are those of
(float32(F K M), X negated); nothing changes for a batch without left hands; and such a batch drives training.

Every draw is host-side, so the seeds below were picked on the CPU; each test asserts what it was picked for."""
import random

import numpy as np
import pytest
import torch

from oracle import augment_oracle as A
from tests import augment_ext_ref as R
from tests.test_augment_ragged_gpu import joints_for, synth_image
from tests.test_supervised_gpu import hands

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEW = ("sobel_filter", "cut_out", "gaussian_blur", "gaussian_noise", "color_drop")
# 37 x 53: narrower than one 64-wide block, odd width, odd byte size; 129 x 67 and 96 x 130: two and three blocks in x, so blur
# halos cross block edges on mirrored columns.  The set comes twice, each size once left and once right.
SIZES = [(37, 53), (64, 64), (129, 67), (96, 130)] * 2
LEFT = [True, False, True, False, False, True, False, True]
_IMAGES = {}


def images_for(sizes):
    key = tuple(sizes)
    if key not in _IMAGES:
        _IMAGES[key] = [synth_image(70 + i, hw) for i, hw in enumerate(sizes)]
    return _IMAGES[key]


def flip(img):
    return np.ascontiguousarray(img[:, ::-1])


def seen(images, left):
    """What the augmenter is to see of each stored image: the mirror image of a left hand."""
    return [flip(im) if l else im for im, l in zip(images, left)]


def mirror_of(left, sizes):
    from peclr_amd.augment import mirror_table

    return mirror_table(list(left), sizes).to(DEV)


def flipped_joints(joints, sizes, left):
    out = joints.clone()
    for i, (l, (_, w)) in enumerate(zip(left, sizes)):
        if l:
            out[i, :, 0] = w - out[i, :, 0]          # float32, the loader's rule
    return out


def launches(fn):
    """fn() with the event log on -> (its result, [(tag, kernel field)] per logged launch, sorted)."""
    from peclr_amd import _capi

    _capi.EVENT_LOG = {}
    try:
        out = fn()
        torch.cuda.synchronize()
        log = sorted(((tag, e[4]) for tag, es in _capi.EVENT_LOG.items() for e in es), key=lambda t: (t[0], t[1] or ""))
    finally:
        _capi.EVENT_LOG = None
    return out, log


def same_dict(a, b, skip=("is_left",)):
    ka, kb = set(a) - set(skip), set(b) - set(skip)
    assert ka == kb, ka ^ kb
    for k in sorted(ka):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].device == b[k].device, k
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------ 1. the recipe, stage by stage
def test_recipe_flags_ragged_batch_left_and_right_bit_exact_stage_by_stage():
    """View 1 is drawn with the rotation and view 2 without it, so every left sample takes both read paths of warp_crop_kernel
    (the bilinear taps and the plain copy) in the one launch."""
    from peclr_amd import RaggedImages, _capi
    from peclr_amd.augment import IMAGENET_MEAN, IMAGENET_STD, RECIPE_FLAGS, TwoViewAugmenter

    images, joints = images_for(SIZES), joints_for(SIZES, 1)
    b = len(SIZES)
    assert any(LEFT) and not all(LEFT)
    par = {"resize_shape": [32, 32]}
    rot = TwoViewAugmenter(RECIPE_FLAGS, par, rng=random.Random(13))
    flat = TwoViewAugmenter(dict(RECIPE_FLAGS, rotate=False), par, rng=random.Random(12))
    _, rot_views = rot.sample_batch(joints, SIZES, LEFT)
    _, flat_views = flat.sample_batch(joints, SIZES, LEFT)
    views = [rot_views[0], flat_views[1]]
    assert all(w["minv"] is not None and w["angle"] != 0 for w in views[0]) and all(w["minv"] is None for w in views[1])
    params = torch.tensor([[rot.pack(w) for w in vs] for vs in views], dtype=torch.float64)
    ragged = RaggedImages.from_list(images, DEV)
    geom, wins = rot.ragged_tables(SIZES, ragged.offsets, views)
    src = seen(images, LEFT)
    for nhwc in (True, False):
        (out, crops, tab), log = launches(lambda: _capi.augment_views_ragged(
            ragged.data, geom, wins, params.to(DEV), (32, 32), IMAGENET_MEAN, IMAGENET_STD, channels_last=nhwc,
            mirror=mirror_of(LEFT, SIZES)))
        assert [t for t, _ in log] == ["augment_resize_color_norm", "augment_warp_crop"]
        assert out.is_contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format)
        differs = 0
        for v in (0, 1):
            for i in range(b):
                w = views[v][i]
                win = _capi.ragged_window(crops, tab, v, i).cpu().numpy()
                ref_win = R.crop_window(src[i], w)
                assert np.array_equal(win, ref_win), f"window, view {v} sample {i} left {LEFT[i]}"
                differs += LEFT[i] and not np.array_equal(ref_win, R.crop_window(images[i], w))
                img = A.color_jitter_u8(A.resize_area_u8(ref_win, (32, 32)), w["h"], w["s"], w["a"], w["b"])
                assert np.array_equal(out[v * b + i].cpu().numpy(), A.to_tensor_normalize(img)), f"view {v} sample {i}"
        assert differs == 2 * sum(LEFT), "vacuous: a left window that the unmirrored read would have produced as well"


# ------------------------------------------------------------------ 2. hand-made records
def test_hand_made_records_taps_across_both_borders_and_the_identity_window():
    from peclr_amd import RaggedImages, _capi
    from peclr_amd.augment import IMAGENET_MEAN, IMAGENET_STD, TwoViewAugmenter

    sizes = [(37, 53), (64, 64), (37, 53), (64, 64), (129, 67), (96, 130)]
    left = [True, True, False, False, True, True]
    images = images_for(sizes)
    recs, views = [[], []], [[], []]
    for h, w in sizes:
        # view 1: the whole window of the image rotated by 10 degrees and shrunk to 0.8 about its centre -- the inverse map
        # scales by 1.25, so the window's corners read from beyond every border
        a, s = 1.25 * np.cos(np.deg2rad(10.0)), 1.25 * np.sin(np.deg2rad(10.0))
        cx, cy = (w - 1) / 2, (h - 1) / 2
        minv = [a, s, cx - a * cx - s * cy, -s, a, cy + s * cx - a * cy]
        xx, yy = np.meshgrid(np.arange(w), np.arange(h))
        sx = np.floor(minv[0] * xx + minv[1] * yy + minv[2])
        assert (sx == -1).any() and (sx == w - 1).any() and (sx < -1).any() and (sx > w).any(), "taps straddle both borders"
        recs[0].append([*minv, 1.0, 0.0, 0.0, float(w), float(h), 0.0, 1.0, 1.0, 1.0, 0.0])
        views[0].append({"crop": (0, 0, w, h), "minv": minv})
        # view 2: no rotation, the whole image
        recs[1].append([1.0, 0, 0, 0, 1.0, 0, 0.0, 0.0, 0.0, float(w), float(h), 0.0, 1.0, 1.0, 1.0, 0.0])
        views[1].append({"crop": (0, 0, w, h), "minv": None})
    assert {w % 2 for (_, w), l in zip(sizes, left) if l} == {0, 1}, "an odd and an even width, left"
    params = torch.tensor(recs, dtype=torch.float64)
    ragged = RaggedImages.from_list(images, DEV)
    geom, wins = TwoViewAugmenter.ragged_tables(sizes, ragged.offsets, views)
    out, crops, tab = _capi.augment_views_ragged(ragged.data, geom, wins, params.to(DEV), (64, 64), IMAGENET_MEAN, IMAGENET_STD,
                                                 channels_last=False, mirror=mirror_of(left, sizes))
    src = seen(images, left)
    b = len(sizes)
    for i in range(b):
        got = _capi.ragged_window(crops, tab, 0, i).cpu().numpy()
        assert np.array_equal(got, R.crop_window(src[i], views[0][i])), f"rotated, sample {i} left {left[i]}"
        whole = _capi.ragged_window(crops, tab, 1, i).cpu().numpy()
        assert np.array_equal(whole, src[i]), f"identity window, sample {i} left {left[i]}"      # img[:, ::-1] itself
        assert np.array_equal(out[b + i].cpu().numpy(), A.to_tensor_normalize(A.resize_area_u8(src[i], (64, 64)))), i
    # the dense path on the two 64 x 64 images, one left and one right: the same kernel over the uniform geometry
    dense = torch.from_numpy(np.stack([images[1], images[3]])).to(DEV)
    p2 = params[:, [1, 3]].contiguous().to(DEV)
    out2, crops2 = _capi.augment_views(dense, p2, (64, 64), IMAGENET_MEAN, IMAGENET_STD, channels_last=False,
                                       mirror=torch.tensor([64, 0], dtype=torch.int32, device=DEV))
    for v in (0, 1):
        for k, i in enumerate((1, 3)):
            assert np.array_equal(crops2[v, k].cpu().numpy(), _capi.ragged_window(crops, tab, v, i).cpu().numpy()), (v, i)
            assert torch.equal(out2[v * 2 + k], out[v * b + i])


# ------------------------------------------------------------------ 3. all ten flags: the mirror is applied once
EXT_SEED = 1


def ext_augmenter(seed=EXT_SEED):
    from peclr_amd.augment import RECIPE_FLAGS, TwoViewAugmenter

    flags = dict(RECIPE_FLAGS, **{k: True for k in NEW})
    return TwoViewAugmenter(flags, {"resize_shape": [32, 32]}, rng=random.Random(seed), np_rng=np.random.RandomState(seed),
                            extended=True, noise_seed=4242)


def drawn_on_left(aug, views):
    """-> (OR of the stage-0 bits drawn on left samples, the blur lengths drawn on left samples)."""
    from peclr_amd.augment import EXT_BLUR, blur_ksize

    bits, lengths = 0, set()
    for vs in views:
        for i, w in enumerate(vs):
            if LEFT[i]:
                bits |= aug.ext_flags(w)
                if aug.ext_flags(w) & EXT_BLUR:
                    lengths.add(blur_ksize(SIZES[i]))
    return bits, lengths


def test_all_ten_flags_left_samples_bit_exact_stage_by_stage():
    from peclr_amd import RaggedImages, _capi
    from peclr_amd.augment import EXT_BLUR, EXT_CUT_OUT, EXT_SOBEL, IMAGENET_MEAN, IMAGENET_STD, noise_cdf_table

    images, joints = images_for(SIZES), joints_for(SIZES, 2)
    aug = ext_augmenter()
    params, views = aug.sample_batch(joints, SIZES, LEFT)
    bits, lengths = drawn_on_left(aug, views)
    assert bits & EXT_SOBEL and bits & EXT_CUT_OUT and bits & EXT_BLUR, bits
    assert len(lengths) >= 2, lengths
    # a cut-out box on a left sample that is not its own mirror image: a box in the wrong frame would show
    assert any(LEFT[i] and w["cut_out"] is not None and w["cut_out"]["cols"][1] > w["cut_out"]["cols"][0]
               and w["cut_out"]["rows"][1] > w["cut_out"]["rows"][0]
               and w["cut_out"]["cols"] != (SIZES[i][1] - w["cut_out"]["cols"][1], SIZES[i][1] - w["cut_out"]["cols"][0])
               for vs in views for i, w in enumerate(vs))
    ragged = RaggedImages.from_list(images, DEV)
    geom, wins = aug.ragged_tables(SIZES, ragged.offsets, views)
    ext, coefs = aug.pack_ext(views)
    table_t, n_table = aug.noise_table()
    ops = int(np.bitwise_or.reduce(ext[..., 0].flatten().numpy()))
    table, b, call = noise_cdf_table(float(aug.params["noise_std"])), len(SIZES), 3
    src = seen(images, LEFT)
    refs = {(v, i): R.render_view_ext(src[i], views[v][i], (32, 32),
                                      {"table": table, "seed": aug.noise_seed, "call": call, "view": v, "sample": i}, stages=True)
            for v in (0, 1) for i in range(b)}
    for nhwc in (True, False):
        (out, srcs, crops, tab), log = launches(lambda: _capi.augment_views_ragged_ext(
            ragged.data, geom, wins, params.to(DEV), ext.to(DEV), coefs.to(DEV), table_t.to(DEV), n_table, aug.noise_seed,
            call, ops, (32, 32), IMAGENET_MEAN, IMAGENET_STD, channels_last=nhwc, mirror=mirror_of(LEFT, SIZES)))
        # stage 0 took the flags, the two per-view warps are the plain ones: the mirror is applied once
        assert log == [("augment_pre", "pre_rows_kernel<Mirrored>"), ("augment_resize_color_norm_ext", None),
                       ("augment_warp_crop", None), ("augment_warp_crop", None)], log
        for (v, i), ref in refs.items():
            got_src = _capi.ragged_image(srcs[v], geom, i).cpu().numpy()
            assert np.array_equal(got_src, ref["source"]), f"stage 0, view {v} sample {i} left {LEFT[i]}"
            assert np.array_equal(_capi.ragged_window(crops, tab, v, i).cpu().numpy(), ref["window"]), f"window, view {v} sample {i}"
            assert np.array_equal(out[v * b + i].cpu().numpy(), ref["tensor"]), f"view {v} sample {i} left {LEFT[i]}"


# ------------------------------------------------------------------ 4. the same batch three ways
@pytest.mark.parametrize("all_ten", [False, True], ids=["recipe", "all_ten"])
def test_dense_list_and_host_flipped_batches_agree(all_ten):
    from peclr_amd import TwoViewAugmenter

    sizes, left = [(96, 130)] * 4, [True, False, True, False]
    images = images_for(tuple(sizes))
    joints = joints_for(sizes, 3)

    def make():
        if all_ten:
            return ext_augmenter(9)
        return TwoViewAugmenter(params={"resize_shape": [32, 32]}, rng=random.Random(3))

    one = make()(torch.from_numpy(np.stack(images)).to(DEV), joints, is_left=left)
    two = make()(list(images), joints, is_left=torch.tensor(left))
    three = make()(torch.from_numpy(np.stack(seen(images, left))).to(DEV), flipped_joints(joints, sizes, left))
    assert one["is_left"].dtype == torch.bool and one["is_left"].is_cuda and one["is_left"].tolist() == left
    assert torch.equal(one["is_left"], two["is_left"]) and "is_left" not in three
    same_dict(one, two)
    same_dict(one, three)
    if all_ten:
        assert bool(one["blur_flag_1"][[0, 2]].any() or one["blur_flag_2"][[0, 2]].any()), "blur drawn on a left sample"
        return
    # the draws and the pixels are the reference's on the flipped inputs, sample by sample
    rng, aug = random.Random(3), make()
    flipped = flipped_joints(joints, sizes, left)
    for i in range(4):
        ref = A.prepare_hybrid2_sample(seen(images, left)[i], flipped[i].numpy(), aug.flags, aug.params, rng)
        assert np.array_equal(one["transformed_image1"][i].cpu().numpy(), ref["transformed_image1"]), i
        assert np.array_equal(one["transformed_image2"][i].cpu().numpy(), ref["transformed_image2"]), i
        for key in ("angle_1", "angle_2", "jitter_x_1", "jitter_y_2", "crop_margin_scale_1", "h_2"):
            assert one[key][i].item() == ref[key], (key, i)


# ------------------------------------------------------------------ 5. nothing changes without left hands
@pytest.mark.parametrize("all_ten", [False, True], ids=["recipe", "all_ten"])
def test_no_left_hand_is_the_call_of_before_and_a_left_hand_adds_no_launch(all_ten):
    from peclr_amd import TwoViewAugmenter

    images, joints = images_for(SIZES), joints_for(SIZES, 1)
    b = len(SIZES)

    def make():
        if all_ten:
            return ext_augmenter(9)
        return TwoViewAugmenter(params={"resize_shape": [32, 32]}, rng=random.Random(3))

    plain, log_plain = launches(lambda: make()(list(images), joints))
    none, log_none = launches(lambda: make()(list(images), joints, is_left=None))
    false, log_false = launches(lambda: make()(list(images), joints, is_left=[False] * b))
    with_left, log_left = launches(lambda: make()(list(images), joints, is_left=LEFT))
    assert "is_left" not in plain and "is_left" not in none and not false["is_left"].any()
    same_dict(plain, none, skip=())
    same_dict(plain, false)
    assert log_plain == log_none == log_false and all(kernel is None for _, kernel in log_plain)
    # one batch of left and right hands: the same launches, no launch per sample -- and one of them mirrors
    assert [t for t, _ in log_left] == [t for t, _ in log_plain]
    assert len(log_left) == (4 if all_ten else 2), log_left
    assert [k for _, k in log_left if k is not None] == (["pre_rows_kernel<Mirrored>"] if all_ten else ["warp_crop_kernel<Mirrored>"])
    assert not torch.equal(with_left["transformed_images"], plain["transformed_images"])
    # (dense batches: the same through the uniform entry points)
    dense = torch.from_numpy(np.stack(images_for(((64, 64),) * 4))).to(DEV)
    j4 = joints_for([(64, 64)] * 4, 1)
    d_plain, dl_plain = launches(lambda: make()(dense, j4))
    d_false, dl_false = launches(lambda: make()(dense, j4, is_left=np.zeros(4, dtype=np.int64)))
    d_left, dl_left = launches(lambda: make()(dense, j4, is_left=[0, 1, 1, 0]))
    same_dict(d_plain, d_false)
    assert dl_plain == dl_false and [t for t, _ in dl_left] == [t for t, _ in dl_plain]
    assert sum(k is not None for _, k in dl_left) == 1


# ------------------------------------------------------------------ 6. SupervisedAugmenter: the definition
def supervised_batch(sizes, seed):
    images = images_for(tuple(sizes))
    ks, js = [], []
    for i, hw in enumerate(sizes):
        k, j = hands(1, seed + i, hw, focal=200.0)
        ks.append(k[0]), js.append(j[0])
    K, J = torch.from_numpy(np.array(ks)), torch.from_numpy(np.array(js))
    raw = J + 0.01 * torch.from_numpy(np.random.default_rng(seed).standard_normal(J.shape)).float()
    return images, K, J, raw


def mirrored_labels(K, J, raw, sizes, left):
    from peclr_amd.supervised import mirror_camera

    Kf, Jf, rawf = K.clone(), J.clone(), raw.clone()
    for i, (l, (_, w)) in enumerate(zip(left, sizes)):
        if l:
            Kf[i], Jf[i] = mirror_camera(K[i], J[i], w)
            rawf[i] = mirror_camera(K[i], raw[i], w)[1]
    return Kf, Jf, rawf


@pytest.mark.parametrize("with_raw", [False, True], ids=["no_raw", "joints_raw"])
@pytest.mark.parametrize("use_palm", [False, True], ids=["plain", "use_palm"])
def test_supervised_left_sample_is_the_flipped_sample_by_definition(use_palm, with_raw):
    from peclr_amd import SupervisedAugmenter

    images, K, J, raw = supervised_batch(SIZES, 50)
    Kf, Jf, rawf = mirrored_labels(K, J, raw, SIZES, LEFT)

    def make():
        return SupervisedAugmenter(params={"resize_shape": [32, 32]}, use_palm=use_palm, rng=random.Random(9))

    a, b = make(), make()
    got, log = launches(lambda: a(list(images), K, J, joints_raw=raw if with_raw else None, is_left=LEFT))
    want = b(seen(images, LEFT), Kf, Jf, joints_raw=rawf if with_raw else None)
    assert got["is_left"].tolist() == LEFT and "is_left" not in want
    same_dict(got, want)
    assert torch.equal(a.last_params, b.last_params) and torch.equal(a.last_T, b.last_T)
    assert log == [("augment_resize_color_norm", None), ("augment_warp_crop", "warp_crop_kernel<Mirrored>"),
                   ("supervised_labels", "supervised_labels_kernel<mirror>")], log
    # not vacuous: the flag changed the left samples and only them
    plain = make()(list(images), K, J, joints_raw=raw if with_raw else None)
    li = [i for i, l in enumerate(LEFT) if l]
    ri = [i for i, l in enumerate(LEFT) if not l]
    assert all(not torch.equal(got["K"][i], plain["K"][i]) and not torch.equal(got["image"][i], plain["image"][i]) for i in li)
    for key in ("K", "joints3D", "joints_raw", "scale"):
        assert torch.equal(got[key][ri], plain[key][ri]), key
    # ... and the dense path, through the uniform entry points
    s4, l4 = [(96, 130)] * 4, [False, True, True, False]
    im4, K4, J4, raw4 = supervised_batch(s4, 60)
    Kf4, Jf4, rawf4 = mirrored_labels(K4, J4, raw4, s4, l4)
    got4 = make()(torch.from_numpy(np.stack(im4)).to(DEV), K4, J4, joints_raw=raw4 if with_raw else None, is_left=l4)
    want4 = make()(torch.from_numpy(np.stack(seen(im4, l4))).to(DEV), Kf4, Jf4, joints_raw=rawf4 if with_raw else None)
    same_dict(got4, want4)


def test_supervised_all_ten_flags_left_sample_is_the_flipped_sample():
    """Stage 0 in the supervised path: the mirror moves to it, and the result is still the flipped sample's."""
    from peclr_amd import SupervisedAugmenter
    from peclr_amd.augment import EXT_PRE, RECIPE_FLAGS

    images, K, J, raw = supervised_batch(SIZES, 50)
    Kf, Jf, rawf = mirrored_labels(K, J, raw, SIZES, LEFT)

    def make():
        return SupervisedAugmenter(dict(RECIPE_FLAGS, **{k: True for k in NEW}), {"resize_shape": [32, 32]}, rng=random.Random(4),
                                   np_rng=np.random.RandomState(4), extended=True, noise_seed=7)

    a = make()
    got = a(list(images), K, J, joints_raw=raw, is_left=LEFT)
    assert any(LEFT[i] and a.views.ext_flags(w) & EXT_PRE for i, w in enumerate(a.last_views)), "a stage-0 op on a left sample"
    same_dict(got, make()(seen(images, LEFT), Kf, Jf, joints_raw=rawf))


# ------------------------------------------------------------------ 7. SupervisedAugmenter: an independent statement
def test_supervised_left_labels_are_the_mirror_image_in_stored_pixels():
    """Resize only.  In pixels of the stored image a joint at column u appears, in the left call, at (W - 1) - u; undoing the
    resize (T is diagonal) the two calls' `joints` must agree within 2 float32 ulps of the image width -- the only error is
    the float32 rounding of coordinates no larger than W.  X of joints3D is negated exactly, and the re-created 3D joints are
    the 3D joints within the label tests' round-trip tolerance (twice the reference's own, tests/golden/g13_supervised.json)."""
    from peclr_amd import SupervisedAugmenter
    from tests import supervised_ref

    rel = 2 * supervised_ref.load_fixture()["round_trip_rel"]
    sizes = SIZES[:4]
    images, K, J, _ = supervised_batch(sizes, 80)

    def make():
        return SupervisedAugmenter({"resize": True}, {"resize_shape": [32, 32]}, rng=random.Random(1))

    plain = make()(list(images), K, J)
    left = make()(list(images), K, J, is_left=[True] * 4)
    assert torch.equal(left["joints3D"][..., 0], -plain["joints3D"][..., 0])
    assert torch.equal(left["joints3D"][..., 1:], plain["joints3D"][..., 1:])
    assert torch.equal(left["scale"], plain["scale"]) and torch.equal(left["T"], plain["T"])
    assert torch.equal(left["joints"][..., 2], plain["joints"][..., 2])
    for i, (h, w) in enumerate(sizes):
        t = plain["T"][i].double().cpu().numpy()
        assert t[0, 1] == 0 and t[0, 2] == 0 and t[1, 0] == 0 and t[1, 2] == 0
        u = plain["joints"][i, :, 0].double().cpu().numpy() / t[0, 0]
        u_left = left["joints"][i, :, 0].double().cpu().numpy() / t[0, 0]
        err = np.abs(u_left - ((w - 1) - u)).max()
        tol = 2 * float(np.spacing(np.float32(w)))
        print(f"{h}x{w}: worst |u_left - ((W - 1) - u)| = {err:.3e} pixels, bound {tol:.3e}")
        assert err <= tol, (i, err, tol)
        v_err = np.abs(left["joints"][i, :, 1].double().cpu().numpy() - plain["joints"][i, :, 1].double().cpu().numpy()).max()
        assert v_err <= 2 * float(np.spacing(np.float32(h))), (i, v_err)
        for out in (plain, left):
            j3, rec = out["joints3D"][i].double().cpu().numpy(), out["joints3D_recreated"][i].double().cpu().numpy()
            worst = np.abs(rec - j3).max() / np.abs(j3).max()
            print(f"{h}x{w}: re-created 3D joints off by {worst:.3e} of the largest coordinate, bound {rel:.3e}")
            assert worst <= rel, (i, worst)


# ------------------------------------------------------------------ 8. a left-hand batch drives training
def test_left_hand_batches_drive_a_pretraining_and_a_fine_tuning_step():
    import warnings

    from peclr_amd import Hybrid2Model, SupervisedAugmenter, Trainer, TwoViewAugmenter, bn2d, hybrid2_config
    from peclr_amd.bn2d import enable_hip_batchnorm
    from tests.test_finetune_gpu import B, new_module

    warnings.simplefilter("ignore")
    images, joints = images_for(SIZES), joints_for(SIZES, 1)
    b = len(SIZES)
    aug = TwoViewAugmenter(params={"resize_shape": [64, 64]}, rng=random.Random(3))
    batch = aug(list(images), joints, is_left=LEFT)
    torch.manual_seed(0)
    cfg = hybrid2_config(resnet_size="18", projection_head_input_dim=512, augmentation=["crop", "rotate"], batch_size=b,
                         num_samples=64, pretrained=False)
    model = Hybrid2Model(cfg).to(DEV).train()
    model.encoder = model.encoder.to(memory_format=torch.channels_last)
    enable_hip_batchnorm(model.encoder)
    trainer = Trainer(max_epochs=1).attach(model)
    out = trainer.training_micro_step(batch, 0)
    assert torch.isfinite(out["loss"]).item() and len(out) == 17

    assert B == b
    im, K, J, _ = supervised_batch(SIZES, 50)
    sup = SupervisedAugmenter({"crop": True, "resize": True}, {"resize_shape": [64, 64]}, rng=random.Random(5))
    sbatch = sup(list(im), K, J, is_left=LEFT)
    assert sbatch["is_left"].tolist() == LEFT
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with bn2d.routing(force=True), torch.cuda.stream(side):
        m = new_module(num_samples=64)
        step = m.training_step(sbatch, 0)
        assert torch.isfinite(step["loss"]).item()
        assert all(torch.isfinite(v).all().item() for v in step.values())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    bn2d.end_backward()
