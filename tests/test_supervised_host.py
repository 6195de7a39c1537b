"""The supervised sample's host side (peclr_amd/supervised.py) and the float64 restatement the GPU tests measure against
(tests/supervised_ref.py), on the reference's own results (tests/golden/g13_supervised.json).  No GPU."""
import random

import numpy as np
import pytest
import torch

from tests import supervised_ref as ref

FIX = ref.load_fixture()
CASES = FIX["cases"]
IDS = [c["name"] for c in CASES]
REL = 1e-12  # both sides are float64 and differ only in evaluation order; c ~ -1, so -b + sqrt(d) does not cancel


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    worst = np.max(err / np.where(want == 0, 1.0, np.abs(want)))
    print(f"{what}: worst relative error {worst:.3e}")
    assert np.all(err <= REL * np.abs(want)), (what, worst)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_agrees_with_the_reference_in_float64(case):
    g32 = {k: ref.dec(v) for k, v in case["gold32"].items()}
    g64 = {k: ref.dec(v) for k, v in case["gold64"].items()}
    k, j = ref.dec(case["K"]), ref.dec(case["joints3D"])
    raw = ref.dec(case["joints_raw"]) if "joints_raw" in case else None
    T = np.array(case["T"], np.float64)
    # convert_to_2_5D on the inputs
    j25, s = ref.to_25d(k, j)
    close(j25, g64["raw25"], "raw25")
    close(s, g64["raw_scale"][0], "raw_scale")
    # K' = fl32(T) @ K
    close(ref.f32(T) @ k.astype(np.float64), g64["K"], "K")
    # joints and scale: each stage on the float32 tensors the reference's stage read
    if case["use_palm"]:
        joints, scale = ref.to_25d(g32["K"], g32["joints3D"])
        close(ref.move_wrist_to_palm(j), g64["joints3D"], "joints3D")
        close(ref.move_wrist_to_palm(j if raw is None else raw), g64["joints_raw"], "joints_raw")
    else:
        hom = j25.copy()
        hom[:, 2] = 1.0
        joints, scale = j25.copy(), s
        joints[:, :2] = (hom @ T.T)[:, :2]
    close(joints, g64["joints"], "joints")
    close(scale, g64["scale"][0], "scale")
    # convert_2_5D_to_3D / get_root_depth on the reference's float32 joints, scale, K'
    rec, zr = ref.to_3d(g32["joints"], g32["scale"][0], g32["K"])
    close(rec, g64["joints3D_recreated"], "joints3D_recreated")
    close(zr, g64["z_root"][0], "z_root")
    if case["clamp"]:
        assert zr == 0.5 * np.sqrt(1e-6) / 1e-6  # a = 0 and b = 0 exactly: both clamps decide


def test_restatement_agrees_with_the_batched_reference():
    blk = FIX["batched"]
    k, j25, sc, zc = (ref.dec(blk[n]) for n in ("K", "joints25D", "scale", "z_root_calc"))
    g64 = {n: ref.dec(v) for n, v in blk["gold64"].items()}
    for i in range(len(k)):
        out, zr = ref.to_3d(j25[i], sc[i], k[i])
        close(out, g64["joints3D"][i], f"joints3D[{i}]")
        close(zr, g64["z_root"][i], f"z_root[{i}]")
        close(ref.to_3d(j25[i], sc[i], k[i], zc[i])[0], g64["joints3D_calc"][i], f"joints3D_calc[{i}]")


def test_label_chain_rounds_each_emitted_tensor_once():
    """The chain the device is held to.  Its outputs are float32 values, and where a stage reads the sample's inputs alone
    (K'; joints and scale without use_palm) the output is ONE rounding of the reference's float64 result: within 2^-23
    relative, with the GPU tests' absolute floor of 2^-40 x the sample's largest magnitude."""
    for case in CASES:
        raw = ref.dec(case["joints_raw"]) if "joints_raw" in case else None
        out = ref.label_chain(ref.dec(case["K"]), ref.dec(case["joints3D"]), case["T"], case["use_palm"], raw)
        for key, v in out.items():
            assert np.array_equal(v, ref.f32(v)), key
        for key in ("K",) if case["use_palm"] else ("K", "joints", "scale"):
            g64 = ref.dec(case["gold64"][key]).reshape(np.shape(out[key]))
            bound = np.maximum(2.0 ** -23 * np.abs(g64), 2.0 ** -40 * np.max(np.abs(g64)))
            assert np.all(np.abs(out[key] - g64) <= bound), (case["name"], key)


# ------------------------------------------------------------------ the parameter side
def _augmenter(case, **kw):
    from peclr_amd import SupervisedAugmenter

    flags = {k: True for k in case["flags_on"]}
    return SupervisedAugmenter(flags, case["params"], use_palm=case["use_palm"], rng=random.Random(case["seed"]), **kw)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parameter_side_equals_the_reference(case):
    aug = _augmenter(case)
    k, j = torch.from_numpy(ref.dec(case["K"]))[None], torch.from_numpy(ref.dec(case["joints3D"]))[None]
    h, w = case["image_hw"]
    params, views, T = aug.sample_batch(k, j, [(h, w)])
    view, d = views[0], case["draws"]
    assert np.array_equal(T[0].numpy(), np.array(case["T"], np.float64)), "T must match to the last bit"
    assert T.dtype == torch.float64 and tuple(params.shape) == (1, 1, 16)
    crop_on, rotate_on = "crop" in case["flags_on"], "rotate" in case["flags_on"]
    assert view["angle"] == (d["angle"] if rotate_on else None)
    if crop_on:
        ox, oy, side = case["boxes"][-1]
        assert view["origin"] == (ox, oy)
        x0, y0 = min(ox, w), min(oy, h)
        assert view["crop"] == (x0, y0, min(ox + side, w) - x0, min(oy + side, h) - y0)
        assert (view["jitter_x"], view["jitter_y"]) == (d["jitter_x"], d["jitter_y"])
        assert view["crop_margin_scale"] == d["crop_margin_scale"]
    else:  # no jitter and no margin draw; the window is the whole image
        assert view["origin"] is None and view["crop"] == (0, 0, w, h)
        assert len(case["boxes"]) == (1 if rotate_on else 0)
    if "color_jitter" in case["flags_on"]:
        assert (view["h"], view["s"], view["a"], view["b"]) == (d["h"], d["s"], d["a"], d["b"])
    assert aug.views.rng.random() == d["next_random"], "a different number of draws than the reference's"
    rw, rh = case["params"]["resize_shape"]
    assert case["out_shape"] == [rh, rw, 3]


def test_always_crop_default_keeps_the_two_view_draws():
    """`sample_view`'s new switch defaults to the hybrid2 behaviour: the window is cropped with the crop flag off."""
    from peclr_amd import TwoViewAugmenter

    case = next(c for c in CASES if c["name"] == "nocrop")
    j25 = torch.from_numpy(ref.dec(case["gold32"]["raw25"]))
    flags = {k: True for k in case["flags_on"]}
    a, b = (TwoViewAugmenter(flags, case["params"], rng=random.Random(3)) for _ in range(2))
    hw = tuple(case["image_hw"])
    cropped, whole = a.sample_view(j25, hw), b.sample_view(j25, hw, always_crop=False)
    assert cropped["crop"] != (0, 0, hw[1], hw[0]) and cropped["origin"] is not None
    assert whole["crop"] == (0, 0, hw[1], hw[0]) and whole["origin"] is None


# ------------------------------------------------------------------ the emitted dict, with the native calls replaced
def test_emitted_dict_keys_shapes_dtypes(monkeypatch):
    from peclr_amd import RaggedImages, SupervisedAugmenter, _capi

    calls = []

    def labels(K, joints3d, T, use_palm=False, joints_raw=None):
        calls.append("labels")
        b = joints3d.shape[0]
        assert K.dtype == torch.float32 and joints3d.dtype == torch.float32 and T.dtype == torch.float64
        assert tuple(T.shape) == (b, 3, 3)
        z = lambda *s: torch.zeros(s, dtype=torch.float32)  # noqa: E731
        return {"joints": z(b, 21, 3), "K": z(b, 3, 3), "scale": z(b), "joints3D": z(b, 21, 3), "joints3D_recreated": z(b, 21, 3),
                "joints_raw": z(b, 21, 3), "T": z(b, 3, 3)}

    def pixels(packed, geom, wins, params, out_hw, mean, std, channels_last=True):
        calls.append("pixels")
        assert tuple(params.shape) == (1, geom.shape[0], 16) and tuple(wins.shape) == (1, geom.shape[0], 4)
        return torch.zeros((geom.shape[0], 3) + tuple(out_hw)), None, wins

    def host_pack(cls, images, device):
        sizes = cls.check(images)
        return cls(torch.cat([torch.from_numpy(im).reshape(-1) for im in images]), sizes)

    monkeypatch.setattr(_capi, "supervised_labels", labels)
    monkeypatch.setattr(_capi, "augment_views_ragged", pixels)
    monkeypatch.setattr(RaggedImages, "from_list", classmethod(host_pack))
    sizes = [(96, 96), (72, 120), (96, 96)]
    images = [np.zeros((h, w, 3), np.uint8) for h, w in sizes]
    K = torch.tensor([[[200.0, 0, w / 2], [0, 200.0, h / 2], [0, 0, 1]] for h, w in sizes])
    g = np.random.default_rng(0)
    J = []
    for h, w in sizes:
        z = 0.6 + 0.05 * g.standard_normal(21)
        u, v = w / 2 + 8 * g.standard_normal(21), h / 2 + 8 * g.standard_normal(21)
        J.append(np.stack([(u - w / 2) * z / 200, (v - h / 2) * z / 200, z], 1))
    J = torch.tensor(np.array(J), dtype=torch.float32)
    aug = SupervisedAugmenter(params={"resize_shape": [32, 32]}, rng=random.Random(5))
    out = aug(images, K, J)
    assert calls == ["labels", "pixels"]
    want = {"image": (torch.float32, (3, 3, 32, 32)), "joints": (torch.float32, (3, 21, 3)), "joints3D": (torch.float32, (3, 21, 3)),
            "K": (torch.float32, (3, 3, 3)), "scale": (torch.float32, (3,)), "joints3D_recreated": (torch.float32, (3, 21, 3)),
            "joints_valid": (torch.float32, (3, 21, 1)), "joints_raw": (torch.float32, (3, 21, 3)), "T": (torch.float32, (3, 3, 3))}
    assert list(out) == list(want)
    for key, (dtype, shape) in want.items():
        assert out[key].dtype == dtype and tuple(out[key].shape) == shape, key
    assert torch.equal(out["joints_valid"], torch.ones(3, 21, 1))
    assert len(aug.last_views) == 3 and tuple(aug.last_params.shape) == (1, 3, 16) and tuple(aug.last_T.shape) == (3, 3, 3)
    valid = torch.zeros(3, 21, 1, dtype=torch.int64)
    given = aug(images, K, J, joints_valid=valid)["joints_valid"]
    assert given.dtype == torch.int64 and torch.equal(given, valid)          # as given


def test_refusals_come_before_any_device_call(monkeypatch):
    from peclr_amd import RaggedImages, SupervisedAugmenter, _capi

    def no_device(*a, **k):
        raise AssertionError("device call")

    for name in ("supervised_labels", "augment_views", "augment_views_ragged", "augment_views_ext", "augment_views_ragged_ext"):
        monkeypatch.setattr(_capi, name, no_device)
    monkeypatch.setattr(RaggedImages, "from_list", classmethod(no_device))
    case = CASES[0]
    k, j = torch.from_numpy(ref.dec(case["K"]))[None], torch.from_numpy(ref.dec(case["joints3D"]))[None]
    aug = _augmenter(case)
    img = np.zeros((224, 224, 3), np.uint8)
    with pytest.raises(ValueError, match="for 2 images"):
        aug([img, img], k, j)                                     # a length mismatch
    with pytest.raises(ValueError, match="joints_raw"):
        aug([img], k, j, joints_raw=j[:, :20])
    with pytest.raises(ValueError, match="empty crop window"):
        aug([np.zeros((30, 30, 3), np.uint8)], k, j + torch.tensor([0.5, 0.5, 0.0]))   # the hand lies outside the image
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        aug(torch.zeros((1, 224, 224, 3), dtype=torch.uint8), k, j)


def test_cpu_tensors_are_refused():
    from peclr_amd import PoseEvaluator, _capi, joints3d_to_25d, joints25d_to_3d, root_depth

    k, j, s = torch.eye(3)[None], torch.ones(1, 21, 3), torch.ones(1)
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        joints3d_to_25d(k, j)
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        joints25d_to_3d(j, s, k)
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        root_depth(j, k)
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        _capi.supervised_labels(k, j, torch.eye(3, dtype=torch.float64)[None])
    assert hasattr(PoseEvaluator, "update_25d")


def test_entry_points_are_declared_bound_and_refuse_null():
    from peclr_amd import _capi
    from tests.test_capi_abi import declared_signatures

    declared = declared_signatures()
    for name in ("peclr_joints3d_to_25d", "peclr_joints25d_to_3d", "peclr_supervised_labels"):
        assert declared[name] == (_capi.SIGNATURES[name][0], list(_capi.SIGNATURES[name][1]))
    L = _capi.lib()
    assert L.peclr_joints3d_to_25d(None, None, 4, None, None, None) == -1
    assert L.peclr_joints25d_to_3d(None, None, None, None, 4, None, None, None) == -1
    assert L.peclr_supervised_labels(None, None, None, None, 0, 0, None, None, None, None, None, None, None, None) == -1
