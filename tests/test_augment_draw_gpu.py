"""TwoViewAugmenter(device_draws=True) on the GPU against the host path driven by the same uniforms (tests/augment_draw_ref.py):
uniforms bit for bit against the Python Philox, continuous fields bit for bit, matrices within a derived bound, integer fields
exact away from fragile pairs, left hands, pixels, the empty window, no synchronisation, one hipGraph."""
import numpy as np
import pytest
import torch

from tests import augment_draw_ref as R

pytestmark = pytest.mark.gpu

INPUT_SEED, DRAW_SEED = 1, 1235          # fragile pairs re-checked on the CPU: tests/test_augment_draw_host.py
CASES = {
    "dense64": [(224, 224)] * 64,
    "ragged8": [(224, 224), (240, 320), (480, 640), (97, 131)] * 2,   # 97 x 131: odd, non-square
    "one": [(224, 224)],
    "b300": [(224, 224)] * 300,          # five workgroups: the ticket decides who advances the counter
}
RAGGED = ("ragged8",)
SCALARS = ("angle", "crop_margin_scale", "h", "s", "a", "b")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def half_left(b):
    return [i % 2 == 1 for i in range(b)]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()]) if t.dtype != torch.bool else t


_INPUTS = {}


def inputs(name):
    """(images for the call -- a [B,H,W,3] device tensor or a RaggedImages --, the list of device images, joints on the device,
    joints on the host), built once per case."""
    from peclr_amd.augment import RaggedImages

    if name not in _INPUTS:
        images, joints = R.make_inputs(CASES[name], INPUT_SEED)
        on_dev = [im.to(dev()) for im in images]
        batch = RaggedImages.from_list(on_dev, dev()) if name in RAGGED else torch.stack(on_dev)
        _INPUTS[name] = (batch, on_dev, joints.to(dev()), joints)
    return _INPUTS[name]


def augmenter(seed=DRAW_SEED, flags=None):
    from peclr_amd.augment import TwoViewAugmenter

    return TwoViewAugmenter(flags, device_draws=True, draw_seed=seed)


def run(name, aug, is_left=None, calls=1):
    """`calls` calls; the last one's dict, on the host except for the images."""
    batch, _, joints, _ = inputs(name)
    for _ in range(calls):
        out = aug(batch, joints, is_left, return_uniforms=True)
    torch.cuda.synchronize()
    return out


def check_against_host(name, out, call, left=None, flags=R.RECIPE, seed=DRAW_SEED):
    """Conditions 1 - 4 of one call's outputs."""
    sizes = CASES[name]
    b = len(sizes)
    joints = inputs(name)[3]
    u = out["uniforms"].cpu().numpy()
    # 1. uniforms: the Python Philox's, bit for bit
    assert u.shape == (2, b, 8) and np.array_equal(u, R.uniforms_table(seed, call, b))
    views = R.host_views(joints, sizes, u, flags, left=left)
    params = out["params"].cpu()
    assert params.shape == (2, b, 16) and params.dtype == torch.float64
    n_fragile = 0
    for v in (0, 1):
        got = {k: out[f"{k}_{v + 1}"].cpu() for k in SCALARS + ("jitter_x", "jitter_y", "blur_flag") if f"{k}_{v + 1}" in out}
        # the dict is collate's: same keys, dtypes, shapes
        assert set(got) == {k for k in SCALARS + ("jitter_x", "jitter_y", "blur_flag") if views[v][0][k] is not None}
        for k, t in got.items():
            assert t.shape == (b,) and t.dtype == (torch.bool if k == "blur_flag" else torch.int64 if k.startswith("jitter")
                                                   else torch.float64), k
        assert not got["blur_flag"].any()
        for i, w in enumerate(views[v]):
            hgt, wid = sizes[i]
            rec, ref = params[v, i], torch.tensor(w["packed"], dtype=torch.float64)
            # 2. continuous fields: exact
            for k in SCALARS:
                if k in got:
                    assert float(got[k][i]) == w[k], (k, v, i)
            assert torch.equal(bits(rec[11:16]), bits(ref[11:16])), (v, i)
            # 3. matrices: cos / sin may differ from libm's by an ulp, carried through at most six float64 operations on
            # magnitudes <= H + W
            assert float((rec[:6] - ref[:6]).abs().max()) <= 1e-12 * max(1, hgt, wid), (v, i)
            assert float(rec[6]) == float(ref[6])
            # 4. integer fields: exact unless fragile, then within one
            ints = [int(x) for x in rec[7:11]] + [int(got["jitter_x"][i]), int(got["jitter_y"][i])]
            assert [float(x) for x in ints[:4]] == rec[7:11].tolist()
            want = [*w["crop"], w["jitter_x"], w["jitter_y"]]
            x0, y0, cw, ch = ints[:4]
            assert 0 <= x0 and 0 <= y0 and cw >= 1 and ch >= 1 and x0 + cw <= wid and y0 + ch <= hgt, (v, i)
            if w["fragile"]:
                n_fragile += 1
                assert max(abs(a - e) for a, e in zip(ints, want)) <= 1, (v, i, ints, want)
            else:
                assert ints == want, (v, i, ints, want)
    assert n_fragile <= 0.05 * 2 * b, n_fragile
    return views


def same_outputs(a, b, rows=None):
    """Every entry of two dicts bit-equal (for the samples `rows`)."""
    assert set(a) == set(b)
    for k in a:
        x, y = a[k], b[k]
        if k in ("params", "uniforms"):
            x, y = x.transpose(0, 1), y.transpose(0, 1)          # sample first
        elif k == "transformed_images":
            x, y = x.view(2, -1, *x.shape[1:]).transpose(0, 1), y.view(2, -1, *y.shape[1:]).transpose(0, 1)
        if rows is not None:
            x, y = x[rows], y[rows]
        assert torch.equal(bits(x), bits(y)), k


# ------------------------------------------------------------------ 1 - 4: every case, at call 0 and at call 3
_CALLS = {}


def calls_0_and_3(name):
    if name not in _CALLS:
        aug = augmenter()
        first = run(name, aug)
        _CALLS[name] = (first, run(name, aug, calls=3), aug)
    return _CALLS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_draws_equal_the_host_replay(name):
    first, fourth, aug = calls_0_and_3(name)
    check_against_host(name, first, 0)
    check_against_host(name, fourth, 3)
    call, counters = aug.draw_state(dev())
    assert int(call[0]) == 4 and counters.tolist() == [0, 0] and aug.bad_windows() == 0


def test_same_seed_agrees_and_another_seed_differs():
    first = calls_0_and_3("dense64")[0]
    same_outputs(first, run("dense64", augmenter()))
    other = run("dense64", augmenter(DRAW_SEED + 1))
    assert not np.array_equal(other["uniforms"].cpu().numpy(), first["uniforms"].cpu().numpy())
    check_against_host("one", run("one", augmenter(2 ** 63 + 5)), 0, seed=2 ** 63 + 5)     # the key's high word


def test_flags_off_drop_their_entries_and_use_no_slot():
    flags = dict(R.RECIPE, rotate=False, random_crop=False)
    out = run("ragged8", augmenter(flags=flags))
    assert "angle_1" not in out and "crop_margin_scale_2" in out and "h_1" in out
    views = check_against_host("ragged8", out, 0, flags=flags)
    assert all(w["crop_margin_scale"] == 1.25 and w["minv"] is None for vs in views for w in vs)
    flags = dict(R.RECIPE, color_jitter=False, crop=False)
    out = run("ragged8", augmenter(flags=flags))
    assert "h_1" not in out and "b_2" not in out and "angle_2" in out
    check_against_host("ragged8", out, 0, flags=flags)


def test_float64_joints_are_rounded_to_float32_first():
    batch, _, joints, _ = inputs("dense64")
    wide = joints.double() * (1 + 2.0 ** -30)               # far inside half an ulp: rounds back to the float32 value
    assert torch.equal(wide.float(), joints)
    out = augmenter()(batch, wide, return_uniforms=True)
    same_outputs(out, calls_0_and_3("dense64")[0])
    out = augmenter()(batch, inputs("dense64")[3], return_uniforms=True)   # CPU joints are uploaded
    same_outputs(out, calls_0_and_3("dense64")[0])


# ------------------------------------------------------------------ 5: left hands
@pytest.mark.parametrize("name", ["dense64", "ragged8"])
def test_left_hands_follow_the_host_rule(name):
    b = len(CASES[name])
    left = half_left(b)
    as_list = run(name, augmenter(), left)
    check_against_host(name, as_list, 0, left=left)
    as_tensor = run(name, augmenter(), torch.tensor(left, device=dev()))
    same_outputs(as_list, as_tensor)
    as_ints = run(name, augmenter(), torch.tensor(left, device=dev()).to(torch.int32))
    same_outputs(as_list, as_ints)
    assert as_tensor["is_left"].dtype == torch.bool and as_tensor["is_left"].tolist() == left
    unflagged = [i for i in range(b) if not left[i]]
    same_outputs({k: t for k, t in as_list.items() if k != "is_left"}, calls_0_and_3(name)[0], rows=unflagged)
    flagged = [i for i in range(b) if left[i]]
    assert not torch.equal(as_list["params"][:, flagged].cpu(), calls_0_and_3(name)[0]["params"][:, flagged].cpu())


# ------------------------------------------------------------------ 6: pixels
@pytest.mark.parametrize("with_left", [False, True], ids=["right", "left"])
def test_dense_pixels_are_the_pixel_stages_on_the_drawn_params(with_left):
    from peclr_amd import _capi

    batch = inputs("dense64")[0]
    left = half_left(64) if with_left else None
    out = run("dense64", augmenter(), None if left is None else torch.tensor(left, device=dev()))
    mirror = {} if left is None else {"mirror": torch.tensor(left, device=dev()).to(torch.int32)}
    ref, _ = _capi.augment_views(batch, out["params"], (128, 128), MEAN, STD, True, **mirror)
    assert out["transformed_images"].shape == (128, 3, 128, 128)
    assert out["transformed_images"].is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(bits(out["transformed_images"]), bits(ref))
    assert torch.equal(out["transformed_image1"], out["transformed_images"][:64])
    assert torch.equal(out["transformed_image2"], out["transformed_images"][64:])


@pytest.mark.parametrize("with_left", [False, True], ids=["right", "left"])
def test_ragged_pixels_equal_each_sample_alone(with_left):
    from peclr_amd import _capi
    from peclr_amd.augment import TwoViewAugmenter

    batch, on_dev, _, _ = inputs("ragged8")
    sizes = CASES["ragged8"]
    left = half_left(8) if with_left else None
    out = run("ragged8", augmenter(), left)
    params = out["params"]
    mirror = None if left is None else torch.tensor([w if l else 0 for l, (_, w) in zip(left, sizes)], dtype=torch.int32, device=dev())
    geom, wins = TwoViewAugmenter.ragged_slot_tables(sizes, batch.offsets, batch.data.numel())
    assert int(wins[1, 0, 0]) == batch.data.numel() and wins[0, 2].tolist() == [int(batch.offsets[2]), 640, 640, 480]
    ref = _capi.augment_views_ragged(batch.data, geom, wins, params, (128, 128), MEAN, STD, True,
                                     **({} if mirror is None else {"mirror": mirror}))[0]
    assert torch.equal(bits(out["transformed_images"]), bits(ref))
    for i, image in enumerate(on_dev):                    # ... and each sample alone, as a dense batch of one, through `params`
        alone, _ = _capi.augment_views(image[None], params[:, i:i + 1].contiguous(), (128, 128), MEAN, STD, True,
                                       **({} if mirror is None else {"mirror": mirror[i:i + 1]}))
        assert torch.equal(bits(out["transformed_images"][[i, 8 + i]]), bits(alone)), i


# ------------------------------------------------------------------ 7: the empty window
def test_empty_window_is_clamped_and_counted():
    batch, _, joints, _ = inputs("dense64")
    off = joints.clone()
    off[5, :, 0] = 2 * 224 + 20 * torch.rand(21, device=dev())     # every joint right of the image, in both views
    aug = augmenter()
    out = aug(batch, off, return_uniforms=True)
    torch.cuda.synchronize()
    assert aug.bad_windows() == 1
    same_outputs(out, calls_0_and_3("dense64")[0], rows=[i for i in range(64) if i != 5])
    for v in (0, 1):
        x0, y0, cw, ch = (int(t) for t in out["params"][v, 5, 7:11])
        assert (cw, ch) == (1, 1) and x0 == 223 and 0 <= y0 <= 223
    assert torch.isfinite(out["transformed_images"]).all()
    aug(batch, off)
    assert aug.bad_windows() == 2                          # cumulative
    with pytest.raises(ValueError, match="empty crop window"):      # what the host path does with this sample
        R.host_views(off[5:6].cpu(), [(224, 224)], out["uniforms"][:, 5:6].cpu().numpy())


# ------------------------------------------------------------------ 8: no synchronisation; one graph
def test_dense_call_does_not_synchronise_with_the_host():
    batch, _, joints, _ = inputs("dense64")
    left = torch.tensor(half_left(64), device=dev())
    aug = augmenter()
    aug(batch, joints, left)                               # (first use: the draw state, the allocator)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        aug(batch, joints)
        out = aug(batch, joints, left, return_uniforms=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert np.array_equal(out["uniforms"].cpu().numpy(), R.uniforms_table(DRAW_SEED, 2, 64))


def test_one_launch_under_its_log_name():
    from peclr_amd import _capi

    batch, _, joints, _ = inputs("dense64")
    aug = augmenter()
    out = aug(batch, joints)
    assert "params" not in out and "uniforms" not in out   # only with return_uniforms=True
    _capi.EVENT_LOG = {}
    try:
        aug(batch, joints)
        torch.cuda.synchronize()
        log = {k: len(v) for k, v in _capi.EVENT_LOG.items()}
    finally:
        _capi.EVENT_LOG = None
    assert log == {"augment_draw": 1, "augment_warp_crop": 1, "augment_resize_color_norm": 1}


def test_captured_call_draws_afresh_on_every_replay():
    batch, _, joints, _ = inputs("dense64")
    left = torch.tensor(half_left(64), device=dev())
    eager_aug, aug = augmenter(), augmenter()
    eager = []
    for _ in range(5):                                     # eager calls number 0 .. 4
        out = eager_aug(batch, joints, left, return_uniforms=True)
        eager.append({k: t.clone() for k, t in out.items()})
    for _ in range(2):                                     # c = 2 eager calls before the capture
        aug(batch, joints, left, return_uniforms=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = aug(batch, joints, left, return_uniforms=True)
    torch.cuda.synchronize()
    call = aug.draw_state(dev())[0]
    assert int(call[0]) == 2                               # the capture itself drew nothing
    for n in (2, 3, 4):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(captured["uniforms"].cpu().numpy(), R.uniforms_table(DRAW_SEED, n, 64))
        same_outputs(captured, eager[n])
    assert int(call[0]) == 5 and aug.draw_state(dev())[1].tolist() == [0, 0]
