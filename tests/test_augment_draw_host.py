"""Device draws of the two-view augmenter, the part that needs no GPU: the Philox4x32-10 restatement the GPU tests compare
against, the refusals (before any device call), the untouched default path, the C ABI of the new entry point, and the fragile
pairs of the inputs the GPU tests commit to."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import augment_draw_ref as R
from tests.conftest import GOLDEN as GOLDEN_DIR
from tests.conftest import ROOT

ALL_FLAGS = ("color_drop", "color_jitter", "crop", "cut_out", "gaussian_blur", "random_crop", "resize", "rotate",
             "gaussian_noise", "sobel_filter")


# ------------------------------------------------------------------ Philox4x32-10: the published known-answer vectors
@pytest.mark.parametrize("counter, key, expect", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, expect):
    assert R.philox4x32_10(counter, key) == expect


def test_uniforms_are_pythons_construction():
    """53 bits of two words, in [0, 1); the counter layout of include/peclr_hip.h; nothing but (seed, call, v, i) enters."""
    assert R.unit(0, 0) == 0.0 and R.unit(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53
    assert R.unit(1 << 5, 0) == 2.0 ** -27 and R.unit(0, 1 << 6) == 2.0 ** -53
    seed, call = (7 << 32) | 5, (3 << 32) | 9
    u = R.uniforms(seed, call, 1, 11)
    x, y, z, w = R.philox4x32_10((11, 4 * 1 + 2, 9, 3), (5, 7))
    assert u[4] == R.unit(x, y) and u[5] == R.unit(z, w) and len(u) == 8
    assert len({tuple(R.uniforms(s, c, v, i)) for s in (1, 2) for c in (0, 1) for v in (0, 1) for i in (0, 1)}) == 16


def test_replay_drives_sample_view_in_slot_order():
    """A slot whose flag is off is skipped, not shifted: the colour factors come from slots 4..7 whatever else is on."""
    from peclr_amd.augment import TwoViewAugmenter

    u = np.linspace(0.05, 0.75, 8)
    _, j = R.make_inputs([(224, 224)], 0, with_images=False)
    full = TwoViewAugmenter(R.RECIPE, rng=R.Replay(u, R.RECIPE)).sample_view(j[0], (224, 224))
    flags = dict(R.RECIPE, rotate=False, random_crop=False)
    part = TwoViewAugmenter(flags, rng=R.Replay(u, flags)).sample_view(j[0], (224, 224))
    assert full["angle"] == (45 + (-45 - 45) * u[0]) // 1 and part["angle"] is None
    assert full["crop_margin_scale"] == 0.9 + (1.5 - 0.9) * u[1] and part["crop_margin_scale"] == 1.25
    assert [full[k] for k in "hsab"] == [part[k] for k in "hsab"]
    assert full["h"] == 0.01 + (1.0 - 0.01) * u[4] and full["b"] == 5 + (20 - 5) * u[7]


# ------------------------------------------------------------------ refusals, before any device call
def test_device_draws_refuse_before_any_device_call(monkeypatch):
    from peclr_amd import _capi
    from peclr_amd.augment import TwoViewAugmenter

    def no_launch(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_capi, "_launch", no_launch)
    monkeypatch.setattr(_capi, "lib", no_launch)
    for flag in ("sobel_filter", "cut_out", "gaussian_blur", "gaussian_noise", "color_drop"):
        for extended in (False, True):
            with pytest.raises(NotImplementedError, match=rf"{flag}.*device draws cover the recipe flags"):
                TwoViewAugmenter(dict(R.RECIPE, **{flag: True}), extended=extended, device_draws=True)
    with pytest.raises(ValueError, match="rng"):
        TwoViewAugmenter(rng=random.Random(0), device_draws=True)
    with pytest.raises(ValueError, match="np_rng"):
        TwoViewAugmenter(np_rng=np.random.RandomState(0), device_draws=True)
    with pytest.raises(NotImplementedError, match="resize"):
        TwoViewAugmenter({"crop": True}, device_draws=True)
    with pytest.raises(ValueError, match="device_draws=True"):
        TwoViewAugmenter(draw_seed=3)
    aug = TwoViewAugmenter(device_draws=True, draw_seed=3)
    images, joints = R.make_inputs([(32, 32)] * 2, 0)
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        aug(torch.stack(images), joints)
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        aug(torch.stack(images), joints, is_left=[True, False], return_uniforms=True)
    with pytest.raises(ValueError, match="device_draws=True"):
        TwoViewAugmenter()(torch.stack(images), joints, return_uniforms=True)
    with pytest.raises(ValueError, match="is_left"):
        TwoViewAugmenter(device_draws=True)._call_device([images[0].numpy(), images[1].numpy()], joints, [True], False)
    assert aug.bad_windows() == 0  # no state yet: nothing to read, no device call
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="before capturing"):     # the state's two fills must not land in a graph
        aug.draw_state("cuda:0")


def test_draw_seed_defaults_to_torchs_and_is_64_bits():
    from peclr_amd.augment import TwoViewAugmenter

    assert TwoViewAugmenter(device_draws=True).draw_seed == torch.initial_seed() & (2 ** 64 - 1)
    assert TwoViewAugmenter(device_draws=True, draw_seed=-1).draw_seed == 2 ** 64 - 1
    aug = TwoViewAugmenter(dict(R.RECIPE, rotate=False), device_draws=True, draw_seed=1)
    assert aug.draw_flags() == 2 | 4 | 8 | 16
    assert aug.draw_ranges() == [45.0, -45.0, 0.9, 1.5, 1.25, 15.0, 0.01, 1.0, 0.01, 1.0, 0.5, 1.0, 5.0, 20.0]


# ------------------------------------------------------------------ the default path is the parent's
def _g9():
    with open(os.path.join(GOLDEN_DIR, "g9_augment_params.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", _g9(), ids=[c["name"] for c in _g9()])
def test_default_path_still_draws_the_references_parameters(case):
    """device_draws=False (the default, also spelled out) with a seeded rng: the emitted values and the crop windows of
    tests/golden/g9_augment_params.json, through the public functions."""
    from peclr_amd.augment import TwoViewAugmenter, convert_to_2_5d

    flags = {k: k in case["flags_on"] for k in ALL_FLAGS}
    j25, _ = convert_to_2_5d(torch.tensor(case["K"], dtype=torch.float32), torch.tensor(case["joints3D"], dtype=torch.float32))
    got = []
    for kwargs in ({}, {"device_draws": False}):
        aug = TwoViewAugmenter(flags, case["params"], rng=random.Random(case["seed"]), **kwargs)
        assert aug.device_draws is False
        params, views = aug.sample_batch(j25[None], tuple(case["image_hw"]))
        emitted = aug.collate(views)
        assert set(emitted) == set(case["emitted"])
        for key, ref in case["emitted"].items():
            assert float(emitted[key][0]) == ref["value"], key
        h_img, w_img = case["image_hw"]
        for i, gv in enumerate(case["views"]):
            box = gv["boxes"][-1]
            x0, y0 = min(box[0], w_img), min(box[1], h_img)
            window = (x0, y0, min(box[0] + box[2], w_img) - x0, min(box[1] + box[2], h_img) - y0)
            assert views[i][0]["crop"] == window
            assert params[i, 0, 7:11].tolist() == [float(t) for t in window]
        got.append(params)
    assert torch.equal(got[0], got[1])


# ------------------------------------------------------------------ the C ABI
def test_symbol_is_in_the_header_the_library_and_the_table():
    from peclr_amd import _capi

    name = "peclr_augment_draw_views"
    header = open(os.path.join(ROOT, "include", "peclr_hip.h")).read()
    assert re.search(rf"\bint {name}\s*\(", header)
    assert "stays on the host" not in header
    assert hasattr(ctypes.CDLL(_capi.library_path()), name)
    _P, _I = ctypes.c_void_p, ctypes.c_int
    assert _capi.SIGNATURES[name] == (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _I, _P, ctypes.c_uint64] + [_P] * 7)
    for macro, value in (("ROTATE", 1), ("CROP", 2), ("RANDOM_CROP", 4), ("RESIZE", 8), ("COLOR_JITTER", 16), ("RANGES", 14),
                         ("SCALARS", 6), ("UNIFORMS", 8)):
        assert re.search(rf"#define PECLR_AUG_DRAW_{macro} {value}\b", header), macro
        assert getattr(_capi, f"AUG_DRAW_{macro}") == value
    makefile = open(os.path.join(ROOT, "peclr_amd", "csrc", "Makefile")).read()
    assert "augment_draw.hip" in makefile and os.path.exists(os.path.join(ROOT, "peclr_amd", "csrc", "augment_draw.hip"))


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    """Argument validation happens before the launch (and before the host `ranges` are read), so it is checkable on the CPU."""
    from peclr_amd import _capi

    f = _capi.lib().peclr_augment_draw_views
    one = 1  # any non-null address: refused before it is read
    recipe, f32 = 31, _capi.DTYPE_F32

    def call(joints=one, dtype=f32, b=4, v=2, h=224, w=224, geom=None, mirror=None, flags=recipe, ranges=one, seed=0, cnt=one,
             counters=one, params=one, scalars=one, jitter=one, uniforms=None):
        return f(joints, dtype, b, v, h, w, geom, mirror, flags, ranges, seed, cnt, counters, params, scalars, jitter, uniforms, None)

    for missing in ("joints", "ranges", "cnt", "counters", "params", "scalars", "jitter"):
        assert call(**{missing: None}) == -1, missing
    for b in (0, -3, 32768):
        assert call(b=b) == -2
    for v in (0, 3, -1):
        assert call(v=v) == -2
    assert call(h=0) == -2 and call(w=0) == -2
    assert call(flags=recipe & ~8) == -5       # resize off
    assert call(flags=recipe | 32) == -5       # not a recipe flag
    assert call(dtype=_capi.DTYPE_BF16) == -5


# ------------------------------------------------------------------ the inputs the GPU tests commit to
@pytest.mark.parametrize("name", ["dense64", "ragged8", "one", "b300", "dense64_left", "ragged8_left"])
def test_committed_inputs_keep_the_fragile_cap(name):
    """tests/test_augment_draw_gpu.py asserts that at most 5 % of a case's pairs are fragile; the same count from the Python
    Philox alone, for the seeds committed there, calls 0 and 3."""
    from tests.test_augment_draw_gpu import CASES, DRAW_SEED, INPUT_SEED, half_left

    sizes = CASES[name.replace("_left", "")]
    left = half_left(len(sizes)) if name.endswith("_left") else None
    _, joints = R.make_inputs(sizes, INPUT_SEED, with_images=False)
    for call in (0, 3):
        views = R.host_views(joints, sizes, R.uniforms_table(DRAW_SEED, call, len(sizes)), left=left)
        fragile = sum(w["fragile"] for vs in views for w in vs)
        assert fragile <= 0.05 * 2 * len(sizes), (call, fragile)


def test_committed_special_cases_have_no_fragile_pair():
    """The other draws of tests/test_augment_draw_gpu.py: flags off on the mixed-size batch, and the key with a high word."""
    from tests.test_augment_draw_gpu import CASES, DRAW_SEED, INPUT_SEED

    sizes = CASES["ragged8"]
    _, joints = R.make_inputs(sizes, INPUT_SEED, with_images=False)
    for off in (("rotate", "random_crop"), ("color_jitter", "crop")):
        flags = dict(R.RECIPE, **{k: False for k in off})
        views = R.host_views(joints, sizes, R.uniforms_table(DRAW_SEED, 0, len(sizes)), flags)
        assert not any(w["fragile"] for vs in views for w in vs), off
    _, joints = R.make_inputs(CASES["one"], INPUT_SEED, with_images=False)
    views = R.host_views(joints, CASES["one"], R.uniforms_table(2 ** 63 + 5, 0, 1))
    assert not any(w["fragile"] for vs in views for w in vs)
