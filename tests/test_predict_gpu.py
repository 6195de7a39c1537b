"""`HandPosePredictor` on the device (peclr_amd/predict.py, csrc/predict.hip): the packed crop against the dense one, the
mirrored read, and the whole two-pass call against the existing predictor, against zero-padded dense batches, against
host-flipped left hands, as a hipGraph, and from the command line.

Every comparison is `np.array_equal` / `torch.equal`: the two sides feed bit-identical inputs through the same launches at the
same batch size, so no tolerance is involved (each test prints the largest difference before it asserts).

Which routing the end-to-end comparisons run in: two eval forwards of the fp32 backbone on the same input do not give the same
bits under the default routing (tests/test_pose_gpu.py says so of the existing predictor).  At these batch sizes the default
routing leaves most fp32 convolutions to MIOpen, whose kernels "do not give the same bits on every run" (peclr_amd/bn2d.py); the
first output that differs between two runs is that of layer1.1.conv1, a 1x1 convolution for which no in-tree launch is logged,
on bit-identical input.  Four calls of `FreiHANDPredictor` on the batch of test 3 differed from one another by up to 4.49e-07
(100 to 137 of 189 values), and `HandPosePredictor` from it by up to 5.98e-07, with T1, K1 and T2 equal bit for bit.  The
in-tree kernels are fixed-order, fp32 (`bn2d.routing(force=True)`: every shape they accept goes to them) and 16-bit.  A
bit-for-bit comparison of two whole predictions therefore says something about the new code only on those: the fp32 case of
test 3 runs under `routing(force=True)`, tests 4, 5 and 7 in bf16 with folding."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

CROP_SIZES = [(224, 224), (97, 131), (180, 320), (1, 1), (2, 3)]     # (97, 131): the next image starts at an odd byte


def _prediction_model(seed=7, backend="rn50"):
    """A random backbone with an fc scaled so that the 2D keypoints spread over the crop (~112 +- 40 px) and zrel ~ 0.1
    (the recipe of tests/test_pose_gpu.py): the pass-1 boxes are valid."""
    from peclr_amd import pose

    torch.manual_seed(seed)
    m = pose.RN25DwMLPref(backend).eval()
    with torch.no_grad():
        feats = m.features(torch.randn(4, 3, 224, 224))
        sd = float(feats.std()) * np.sqrt(2048)
        w = torch.randn(64, 2048) / sd
        w[0::3] *= 40
        w[1::3] *= 40
        w[2::3] *= 0.1
        m.backend_model.fc.weight.copy_(w)
        m.backend_model.fc.bias.copy_(torch.tensor([112.0, 112.0, 0.0] * 21 + [0.0]))
        for mod in m.zroot_ref.zroot_ref:
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.uniform_(-0.1, 0.1)
                mod.running_var.uniform_(0.5, 1.5)
    return m


def _images(sizes, seed=0):
    """Smooth random images (a few blobs) of the given sizes, so that the crop samples structure rather than noise."""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in sizes:
        yy, xx = np.mgrid[:h, :w]
        im = np.zeros((h, w, 3))
        for _ in range(6):
            cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0.07, 0.27) * max(h, w)
            im += np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * r * r))[..., None] * rng.uniform(30, 120, 3)
        im += rng.uniform(0, 25, im.shape)
        out.append(np.clip(im, 0, 255).astype(np.uint8))
    return out


def _k_and_scale(sizes, seed=0):
    rng = np.random.default_rng(seed + 100)
    K = np.stack([np.array([[rng.uniform(350, 450), 0, w / 2 + rng.uniform(-12, 12)], [0, rng.uniform(350, 450), h / 2 + rng.uniform(-12, 12)],
                            [0, 0, 1]]) for h, w in sizes])
    return K, rng.uniform(0.02, 0.04, len(sizes))


def _centre_boxes(sizes, seed=0):
    rng = np.random.default_rng(seed + 200)
    return np.array([[w * rng.uniform(0.1, 0.3), h * rng.uniform(0.1, 0.3), w * rng.uniform(0.7, 0.9), h * rng.uniform(0.7, 0.9)]
                     for h, w in sizes])


def _same(got, want, what):
    got, want = (np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a) for a in (got, want))
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{what}: max |difference| {np.nanmax(diff) if diff.size else 0.0:.3e}, {int((got != want).sum())} of {got.size} differ")
    assert np.array_equal(got, want), what


@pytest.fixture(scope="module")
def model():
    return _prediction_model().to(DEV).enable_hip()


@pytest.fixture(scope="module")
def hand(model):
    """bf16 with folding (see the module docstring)."""
    from peclr_amd.predict import HandPosePredictor

    return HandPosePredictor(model, precision="bf16")


# ------------------------------------------------------------------ 1, 2. the crop kernel
def _affines(sizes, size, rng):
    """A general affine per sample whose window overlaps its image: scale, a little rotation and shear, the image centre near
    the crop centre."""
    out = []
    for h, w in sizes:
        s, th = rng.uniform(0.3, 3.0) * size / max(h, w, 8), rng.uniform(-0.5, 0.5)
        A = s * np.array([[np.cos(th), -np.sin(th) + rng.uniform(-0.1, 0.1)], [np.sin(th), np.cos(th)]])
        t = np.array([size / 2, size / 2]) - A @ np.array([w / 2, h / 2]) + rng.uniform(-0.2, 0.2, 2) * size
        out.append(np.array([[A[0, 0], A[0, 1], t[0]], [A[1, 0], A[1, 1], t[1]], [0, 0, 1.0]]))
    return np.stack(out)


def _general_K(b, rng):
    return np.stack([np.array([[rng.uniform(300, 500), rng.uniform(-2, 2), rng.uniform(50, 200)],
                               [rng.uniform(-2, 2), rng.uniform(300, 500), rng.uniform(50, 200)],
                               [rng.uniform(-1e-3, 1e-3), rng.uniform(-1e-3, 1e-3), 1.0]]) for _ in range(b)])


def _ragged_crop(imgs, flips, T, K, table, size):
    from peclr_amd import _capi
    from peclr_amd.augment import RaggedImages

    packed = RaggedImages.from_list(imgs, DEV)
    geom = torch.tensor([[o, h, w, f] for o, (h, w), f in zip(packed.offsets.tolist(), packed.sizes, flips)], dtype=torch.int64)
    return _capi.pose_crop_ragged(packed.data, geom.to(DEV), torch.from_numpy(T).to(DEV), torch.from_numpy(K).to(DEV), table, size)


def _matmul_in_order(T, K):
    """float32(T @ K), each entry t0 k0 + t1 k1 + t2 k2 left to right in float64, no fused multiply-add."""
    return (T[:, :, 0:1] * K[:, 0:1, :] + T[:, :, 1:2] * K[:, 1:2, :] + T[:, :, 2:3] * K[:, 2:3, :]).astype(np.float32)


@pytest.mark.parametrize("size", [96, 224])
def test_ragged_crop_equals_the_dense_crop_of_each_image_alone(size):
    from peclr_amd import _capi, pose

    rng = np.random.default_rng(size)
    imgs = _images(CROP_SIZES, seed=size)
    table = torch.from_numpy(pose.normalisation_table()).to(DEV)
    K = _general_K(len(imgs), rng)
    T_in = _affines(CROP_SIZES, size, rng)
    T_out = T_in.copy()
    T_out[2] = np.array([[1.0, 0, 5000.0], [0, 1.0, -7000.0], [0, 0, 1]])        # this window lies wholly outside its image
    for T in (T_in, T_out):
        out, kp = _ragged_crop(imgs, [0] * len(imgs), T, K, table, size)
        assert out.shape == (len(imgs), 3, size, size) and out.stride() == (3 * size * size, 1, 3 * size, 3)
        for i, im in enumerate(imgs):
            one, k_one = _capi.pose_crop(torch.from_numpy(im[None]).to(DEV), torch.from_numpy(T[i:i + 1]).to(DEV),
                                         torch.from_numpy(K[i:i + 1]).to(DEV), table, size)
            _same(out[i], one[0], f"S={size} crop of sample {i}")
            _same(kp[i], k_one[0], f"S={size} K' of sample {i}")
    border = table[:, 0]
    assert torch.equal(out[2].permute(1, 2, 0), border.expand(size, size, 3))         # outside: the table's value of 0 everywhere
    assert not torch.equal(out[1].permute(1, 2, 0), border.expand(size, size, 3))


@pytest.mark.parametrize("size", [96, 224])
def test_mirrored_read_is_the_crop_of_the_flipped_image(size):
    from peclr_amd import _capi, pose, predict

    rng = np.random.default_rng(size + 1)
    sizes = CROP_SIZES + [(7, 1)]                                                 # W = 1: the mirror is the image itself
    imgs = _images(sizes, seed=size + 1)
    table = torch.from_numpy(pose.normalisation_table()).to(DEV)
    K = _general_K(len(imgs), rng)
    T = _affines(sizes, size, rng)
    s = 0.5 * size / 131                                                          # (97, 131) at half the crop's width, centred:
    T[1] = np.array([[s, 0, size / 2 - s * 65.0], [0, s, size / 2 - s * 48.0], [0, 0, 1]])   # the window crosses its left and right borders
    flips = [1, 1, 1, 1, 1, 1]
    out, kp = _ragged_crop(imgs, flips, T, K, table, size)
    Kf = np.stack([predict.flip_camera(K[i], sizes[i][1]) for i in range(len(imgs))])
    _same(kp, _matmul_in_order(T, Kf), f"S={size} K' = float32(T @ Kf)")
    for i, im in enumerate(imgs):
        flipped = im[:, ::-1].copy()
        one, k_one = _capi.pose_crop(torch.from_numpy(flipped[None]).to(DEV), torch.from_numpy(T[i:i + 1]).to(DEV),
                                     torch.from_numpy(Kf[i:i + 1]).to(DEV), table, size)
        _same(out[i], one[0], f"S={size} mirrored crop of sample {i}")
        _same(kp[i], k_one[0], f"S={size} K' of sample {i}")
    # flags are per sample: a mixed batch gives the mirrored sample where the flag is set and the plain one elsewhere
    mixed, kp_mixed = _ragged_crop(imgs, [1, 0, 1, 0, 0, 1], T, K, table, size)
    plain, kp_plain = _ragged_crop(imgs, [0] * 6, T, K, table, size)
    for i, f in enumerate([1, 0, 1, 0, 0, 1]):
        _same(mixed[i], (out if f else plain)[i], f"S={size} mixed batch, sample {i}")
        _same(kp_mixed[i], (kp if f else kp_plain)[i], f"S={size} mixed batch K', sample {i}")
    assert not torch.equal(out[2], plain[2])


# ------------------------------------------------------------------ 3. same size: the existing predictor
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_same_size_batch_equals_the_freihand_predictor(model, precision):
    """fp32 with every convolution on the in-tree fixed-order kernels (module docstring), and bf16 with folding."""
    from peclr_amd import bn2d
    from peclr_amd.pose import FreiHANDPredictor
    from peclr_amd.predict import HandPosePredictor

    sizes = [(224, 224)] * 3
    imgs = torch.from_numpy(np.stack(_images(sizes, seed=3))).to(DEV)
    K, scale = (torch.from_numpy(a).to(DEV) for a in _k_and_scale(sizes, seed=3))
    old = FreiHANDPredictor(model, precision=precision)
    new = HandPosePredictor(model, precision=precision)
    assert new.fold_bn == old.fold_bn == (precision == "bf16")
    with (bn2d.routing(force=True) if precision == "fp32" else contextlib.nullcontext()):
        want = old.predict(imgs, K, scale)
        old_last = old.last
        again = old.predict(imgs, K, scale)
        got = new.predict(imgs, K, scale)
    _same(again, want, f"{precision} FreiHANDPredictor against itself")
    old.last = old_last
    _same(new.last["T1"], old.last["T1"], f"{precision} T1")
    _same(new.last["K1"], old.last["K1"], f"{precision} K1")
    _same(new.last["T2"], old.last["T2"], f"{precision} T2")
    _same(got["xyz"], want, f"{precision} xyz")
    assert got["kp3d"].dtype == torch.float32 and got["kp2d"].shape == (3, 21, 2)


# ------------------------------------------------------------------ 4. mixed sizes end to end
MIXED = [(150, 200), (224, 224), (97, 131)]


def test_mixed_sizes_equal_the_zero_padded_dense_batch(hand):
    imgs = _images(MIXED, seed=4)
    K, scale = _k_and_scale(MIXED, seed=4)
    boxes = _centre_boxes(MIXED, seed=4)
    got = {k: v.clone() for k, v in hand.predict(imgs, K, scale, boxes).items()}
    assert hand.last["geom"].cpu().tolist() == [[0, 150, 200, 0], [90000, 224, 224, 0], [90000 + 150528, 97, 131, 0]]
    hmax, wmax = max(h for h, _ in MIXED), max(w for _, w in MIXED)
    padded = np.zeros((3, hmax, wmax, 3), dtype=np.uint8)                  # taps outside an image contribute 0: so do these pixels
    for i, im in enumerate(imgs):
        padded[i, :im.shape[0], :im.shape[1]] = im
    want = hand.predict(torch.from_numpy(padded), K, scale, boxes)
    for k in ("xyz", "kp3d", "kp2d"):
        _same(got[k], want[k], f"mixed sizes against the padded batch: {k}")
    assert got["xyz"].dtype == torch.float64 and got["xyz"].shape == (3, 21, 3)
    assert torch.isfinite(got["xyz"]).all() and torch.isfinite(got["kp2d"]).all()


# ------------------------------------------------------------------ 5, 6. left hands, kp2d
def _cv_invert(m):
    """cv::invertAffineTransform on Python floats (float64, nothing fused), [a11 a12 b1 a21 a22 b2] in and out."""
    d = m[0] * m[4] - m[1] * m[3]
    d = 1.0 / d if d != 0.0 else 0.0
    a11, a22, a12, a21 = m[4] * d, m[0] * d, m[1] * -d, m[3] * -d
    return [a11, a12, -a11 * m[2] - a12 * m[5], a21, a22, -a21 * m[2] - a22 * m[5]]


def test_left_hands_equal_host_flipped_right_hands_and_kp2d_follows_its_formula(hand):
    from peclr_amd import predict

    imgs = _images(MIXED, seed=5)
    K, scale = _k_and_scale(MIXED, seed=5)
    boxes = _centre_boxes(MIXED, seed=5)
    left = np.array([True, False, True])
    got = {k: v.cpu().numpy() for k, v in hand.predict(imgs, K, scale, boxes, is_left=left).items()}
    last = hand.last
    assert last["geom"][:, 3].cpu().tolist() == [1, 0, 1]

    # 6. kp2d: the pass-2 keypoints through inv(T2), un-mirrored; kp3d / xyz: the pass-2 values with X negated
    T2, kp2d_crop = last["T2"].cpu().numpy(), last["pass2"]["kp2d"].cpu().numpy()
    want2d = np.empty((3, 21, 2))
    for b in range(3):
        mi = _cv_invert([float(v) for v in T2[b].reshape(-1)[:6]])
        for j in range(21):
            x, y = float(kp2d_crop[b, j, 0]), float(kp2d_crop[b, j, 1])
            u, v = mi[0] * x + mi[1] * y + mi[2], mi[3] * x + mi[4] * y + mi[5]
            want2d[b, j] = ((MIXED[b][1] - 1) - u if left[b] else u), v
    _same(got["kp2d"], want2d, "kp2d against the float64 restatement")
    sign = np.where(left[:, None, None] & (np.arange(3) == 0), -1.0, 1.0)
    _same(got["kp3d"], last["pass2"]["kp3d"].cpu().numpy() * sign.astype(np.float32), "kp3d against pass 2")
    # the boxes were in source pixels: the keypoints come back near them (within the crop's field of view)
    assert np.isfinite(got["kp2d"]).all()

    # 5. the same hands flipped on the host, the camera and the boxes mirrored there, no flag
    imgs_f = [im[:, ::-1].copy() if f else im for im, f in zip(imgs, left)]
    K_f = np.stack([predict.flip_camera(K[i], MIXED[i][1]) if left[i] else K[i] for i in range(3)])
    boxes_f = np.stack([predict.mirror_box(boxes[i], MIXED[i][1]) if left[i] else boxes[i] for i in range(3)])
    want = {k: v.cpu().numpy() for k, v in hand.predict(imgs_f, K_f, scale, boxes_f).items()}
    for b in np.flatnonzero(left):
        want["xyz"][b, :, 0] = -want["xyz"][b, :, 0]
        want["kp3d"][b, :, 0] = -want["kp3d"][b, :, 0]
        want["kp2d"][b, :, 0] = (MIXED[b][1] - 1) - want["kp2d"][b, :, 0]
    for k in ("xyz", "kp3d", "kp2d"):
        _same(got[k], want[k], f"left hands against host-flipped inputs: {k}")       # as numbers: -0.0 == 0.0


# ------------------------------------------------------------------ 7. one hipGraph
def test_graph_replays_ragged_batches_without_a_host_sync(model):
    from peclr_amd.predict import HandPosePredictor

    pred = HandPosePredictor(model, precision="bf16")
    big, small = [(150, 200), (224, 224), (97, 131)], [(64, 80), (33, 47), (120, 90)]
    max_bytes = 3 * sum(h * w for h, w in big) + 1000                     # the tail is never read
    calls = []
    for sizes, seed, left in ((big, 7, None), (small, 8, np.array([False, True, False]))):
        K, scale = _k_and_scale(sizes, seed=seed)
        calls.append((_images(sizes, seed=seed), K, scale, _centre_boxes(sizes, seed=seed), left))
    eager = [{k: v.clone() for k, v in pred.predict(*c).items()} for c in calls]
    pred.capture(3, max_bytes)
    for c, want in zip(calls, eager):                                      # the second batch has fewer bytes than the first
        got = pred.replay(*c)
        for k in ("xyz", "kp3d", "kp2d"):
            _same(got[k], want[k], f"replay against eager: {k}")
    assert pred.last["T2"].shape == (3, 3, 3) and pred.last["geom"][:, 3].cpu().tolist() == [0, 1, 0]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                               # after that warm-up: nothing but the status read
    try:
        again = pred.replay(*calls[0])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    for k in ("xyz", "kp3d", "kp2d"):
        _same(again[k], eager[0][k], f"third replay against eager: {k}")
    with pytest.raises(ValueError, match="captured for 3 images, got 2"):
        pred.replay(calls[0][0][:2])
    with pytest.raises(ValueError, match="at most"):
        pred.replay(_images([(300, 300)] * 3))


# ------------------------------------------------------------------ 8. the tool
def test_pred_images_tool_predicts_and_scores_2d(tmp_path):
    from PIL import Image

    sizes = [(120, 160), (224, 224), (90, 70)]
    imgs = _images(sizes, seed=9)
    (tmp_path / "frames").mkdir()
    meta = []
    rng = np.random.default_rng(9)
    for i, (im, box) in enumerate(zip(imgs, _centre_boxes(sizes, seed=9))):
        Image.fromarray(im).save(str(tmp_path / "frames" / f"f{i}.png"))
        meta.append({"file": f"f{i}.png", "box": box.tolist(), "is_left": i == 1,
                     "uv": (rng.uniform(0.2, 0.8, (21, 2)) * [sizes[i][1], sizes[i][0]]).tolist()})
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    ckpt = tmp_path / "rn50_peclr_yt3d-fh_pt_fh_ft.pth"
    torch.save({"state_dict": _prediction_model().state_dict()}, ckpt)
    out = tmp_path / "res" / "pred.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pred_images.py"), "--model_path", str(ckpt), "--images",
                        str(tmp_path / "frames"), "--meta", str(tmp_path / "meta.json"), "--batch", "2", "--eval", "--out", str(out)],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out) as f:
        res = json.load(f)
    assert sorted(res) == ["f0.png", "f1.png", "f2.png"]
    for rec in res.values():
        assert np.array(rec["xyz"]).shape == (21, 3) and np.array(rec["kp2d"]).shape == (21, 2)
        assert np.isfinite(np.array(rec["xyz"])).all() and np.isfinite(np.array(rec["kp2d"])).all()
    with open(tmp_path / "res" / "pred_eval.json") as f:
        metrics = json.load(f)
    assert np.isfinite(metrics["Mean_EPE_2D"]) and np.isfinite(metrics["Median_EPE_2D"]) and "Mean_EPE_3D" not in metrics
    # the 2D error is the distance between the written keypoints and the given ones
    d = np.concatenate([np.linalg.norm(np.array(res[m["file"]]["kp2d"]) - np.array(m["uv"]), axis=1) for m in meta])
    np.testing.assert_allclose(metrics["Mean_EPE_2D"], d.mean(), rtol=1e-9)
    assert "Mean_EPE_2D" in r.stdout
