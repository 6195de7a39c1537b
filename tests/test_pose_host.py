"""The fine-tuned 2.5D hand-pose model and the FreiHAND helpers on the host, against g11 (tests/golden/make_golden_pose.py:
the reference's own RN_25D_wMLPref, fh_utils and pred())."""
import json
import os
import zipfile

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def g11():
    with open(os.path.join(GOLDEN, "g11_pose.json")) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(GOLDEN, "g11_pose.npz")))


def golden_model(npz, backend="rn50"):
    """RN25DwMLPref with g11's fc and MLP weights (the backbone keeps its random init), eval mode."""
    from peclr_amd.pose import RN25DwMLPref

    m = RN25DwMLPref(backend)
    sd = m.state_dict()
    for k in sd:
        if "w/" + k in npz:
            sd[k] = torch.from_numpy(npz["w/" + k].astype(np.float32) if "fc." in k else npz["w/" + k])
    m.load_state_dict(sd)
    return m.eval()


def _nan_none(a):
    return np.array([[np.nan if v is None else v for v in r] for r in a], dtype=np.float32)


def test_state_dict_keys_follow_the_reference(g11):
    from peclr_amd import resnet
    from peclr_amd.pose import RN25DwMLPref

    meta, _ = g11
    for name, tv in (("rn50", resnet.resnet50), ("rn152", resnet.resnet152)):
        keys = list(RN25DwMLPref(name).state_dict())
        backend = ["backend_model." + k for k in tv().state_dict()]   # torchvision's layout (test_resnet_state_dict_layout)
        assert keys[:len(backend)] == backend
        assert [k for k in keys if k.startswith("backend_model.fc.") or k.startswith("zroot_ref.")] == meta["head_keys"]
        assert keys == backend + meta["head_keys"][2:]
        sd = RN25DwMLPref(name).state_dict()
        assert tuple(sd["backend_model.fc.weight"].shape) == (64, 2048)
    m = RN25DwMLPref()
    assert "K_default" not in m.state_dict() and "zroot_ref.eps" not in m.state_dict()
    np.testing.assert_array_equal(m.K_default.numpy(), np.array(meta["K_default"], dtype=np.float32))
    assert float(m.zroot_ref.eps) == np.float32(1e-8)
    with pytest.raises(ValueError):
        RN25DwMLPref("rn18")


def test_reference_checkpoint_layout_loads_unchanged(tmp_path, g11):
    """A {"state_dict": ...} file with the reference's keys loads with strict=True into a fresh model."""
    from peclr_amd.pose import RN25DwMLPref

    _, npz = g11
    src = golden_model(npz)
    p = tmp_path / "rn50_peclr_yt3d-fh_pt_fh_ft.pth"
    torch.save({"state_dict": src.state_dict()}, p)
    dst = RN25DwMLPref("rn50")
    dst.load_state_dict(torch.load(p)["state_dict"])
    for (k, a), (k2, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert k == k2 and torch.equal(a, b)


@pytest.mark.parametrize("b", [1, 7, 64])
@pytest.mark.parametrize("kname", ["default", "per_sample"])
def test_stock_head_matches_the_reference(g11, b, kname):
    _, npz = g11
    m = golden_model(npz)
    feat = torch.from_numpy(npz[f"feat_{b}"].astype(np.float32))
    K = None if kname == "default" else torch.from_numpy(npz[f"K_{b}"])
    with torch.no_grad():
        out = m.head(feat, K)
    name = f"fwd_{b}_{kname}"
    for key in ("kp3d", "zrel", "kp2d", "kp25d"):
        ref = npz[f"{name}/{key}"]
        got = out[key].numpy()
        assert got.shape == ref.shape, key
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=key)
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-6, err_msg=key)
    # zrel[:, 0] = 0 is written in place: visible in kp25d, also in the NaN row
    assert (out["kp25d"][:, 0, 2] == 0).all() and (out["zrel"][:, 0] == 0).all()
    if b == 7:
        assert np.isnan(out["kp3d"][4].numpy()).all()


def test_stock_forward_runs_the_backbone_and_the_head():
    from peclr_amd.pose import RN25DwMLPref

    torch.manual_seed(0)
    m = RN25DwMLPref("rn50").eval()
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        out = m(x)
        ref = m.head(m.features(x))
        logits = m.backend_model(x)
    assert tuple(out["kp3d"].shape) == (2, 21, 3) and tuple(out["kp25d"].shape) == (2, 21, 3)
    torch.testing.assert_close(out["kp3d"], ref["kp3d"], equal_nan=True)
    assert tuple(logits.shape) == (2, 64)


def test_fh_utils_restatements_match_the_reference_bit_for_bit(g11):
    from peclr_amd import pose

    meta, _ = g11
    for c in meta["modify_bbox"]:
        got = pose.modify_bbox(np.array(c["box"], dtype=c["dtype"]), c["scale"])
        np.testing.assert_array_equal(got.astype(np.float64), np.array(c["out"]))
    for c in meta["affine_from_bbox"]:
        got = pose.create_affine_transform_from_bbox(np.array(c["box"], dtype=c["dtype"]), c["size"])
        np.testing.assert_array_equal(got, np.array(c["T"]))
    for c in meta["bbox_from_pose"]:
        got = pose.get_bbox_from_pose(_nan_none(c["pose"]))
        assert got.tolist() == c["box"]
    with pytest.raises(ValueError):
        pose.get_bbox_from_pose(np.full((21, 2), np.nan, dtype=np.float32))
    np.testing.assert_array_equal(pose.initial_transform(), np.array(meta["T1"]))
    for c in meta["pred"]:
        T2 = pose.recrop_transform(_nan_none(c["kp2d_1"]), np.array(meta["T1"]))
        np.testing.assert_array_equal(T2[:2], np.array(c["T_pass2"]))
        np.testing.assert_array_equal(np.array(meta["T1"])[:2], np.array(c["T_pass1"]))
        xyz = pose.to_freihand(np.array(c["kp3d_2"], dtype=np.float32), c["scale"])
        np.testing.assert_array_equal(xyz, np.array(c["xyz"]))
        assert c["verts_shape"] == [778, 3]


def test_normalisation_table_and_k_prime_match_preprocess(g11):
    from peclr_amd import pose

    meta, npz = g11
    np.testing.assert_array_equal(pose.normalisation_table(), npz["norm_table"])
    Kp = (pose.initial_transform() @ np.array(meta["preprocess_K_in"])).astype(np.float32)
    np.testing.assert_array_equal(Kp, npz["preprocess_K"])
    for c in meta["pred"]:
        for t, k in (("T_pass1", "K_pass1"),):
            T = np.concatenate([np.array(c[t]), [[0, 0, 1]]])
            np.testing.assert_array_equal((T @ np.array(c["K"])).astype(np.float32), np.array(c[k], dtype=np.float32))


def test_submission_round_trips(tmp_path):
    from peclr_amd.pose import write_freihand_submission

    kp = np.random.default_rng(0).standard_normal((3, 21, 3))
    path = write_freihand_submission(str(tmp_path / "out" / "pred_rn50"), torch.from_numpy(kp))
    assert path.endswith("pred_rn50.json")
    with open(path) as f:
        xyz, verts = json.load(f)
    assert np.array(xyz).shape == (3, 21, 3) and np.array(verts).shape == (3, 778, 3)
    np.testing.assert_array_equal(np.array(xyz), kp)
    assert not np.array(verts).any()
    with zipfile.ZipFile(str(tmp_path / "out" / "pred_rn50.zip")) as z:
        assert z.namelist() == ["pred_rn50.json"]
        assert json.loads(z.read("pred_rn50.json")) == [xyz, verts]


def test_pose_entry_points_reject_bad_arguments_before_launch():
    from peclr_amd import _capi

    L = _capi.lib()
    assert L.peclr_pose_crop_u8(None, 1, 4, 4, None, None, None, 224, None, None, None) == -1
    assert L.peclr_pose_head_f32(None, 1, 2048, None, None, None, 1e-5, 1e-5, None, 1, 1e-8, None, None, None, None, 224,
                                 None, None, None, None) == -1
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        _capi.pose_crop(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 3, 3, dtype=torch.float64), None,
                        torch.zeros(3, 256), 224)
