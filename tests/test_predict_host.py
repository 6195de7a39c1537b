"""peclr_amd/predict.py on the host: the crop geometry of `HandPosePredictor` (boxes -> T1, the left-hand mirror, the mirrored
camera), every refusal before the binding is touched, the replay refusals, and tools/pred_images.py's meta validation.
No GPU, no device call."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import _capi_double
from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = [(224, 224), (97, 131), (180, 320)]


def _list_images(sizes=SIZES, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _boxes(sizes=SIZES, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for h, w in sizes:
        x1, y1 = rng.uniform(-10, w / 2), rng.uniform(-10, h / 2)
        out.append([x1, y1, x1 + rng.uniform(5, w), y1 + rng.uniform(5, h)])
    return np.array(out, dtype=np.float64)


# ------------------------------------------------------------------ geometry
@pytest.mark.parametrize("box_scale,crop", [(1.0, 224), (1.25, 96)])
def test_T1_from_boxes_is_the_per_sample_composition_of_pose_py(box_scale, crop):
    from peclr_amd import pose, predict

    boxes = _boxes()
    p = predict.plan(_list_images(), boxes=boxes, crop_size=crop, box_scale=box_scale)
    assert p.T1.dtype == np.float64 and p.T1.shape == (3, 3, 3)
    for i in range(3):
        want = pose.create_affine_transform_from_bbox(pose.modify_bbox(boxes[i].copy(), box_scale), crop)
        assert np.array_equal(p.T1[i], want), i
    # the packed layout: byte offsets are the running sums of 3 H W, no flags
    assert p.geom.dtype == np.int64
    assert p.geom.tolist() == [[0, 224, 224, 0], [224 * 224 * 3, 97, 131, 0], [224 * 224 * 3 + 97 * 131 * 3, 180, 320, 0]]
    assert p.total_bytes == 3 * (224 * 224 + 97 * 131 + 180 * 320)


def test_T1_without_boxes_on_224_images_is_the_initial_transform():
    from peclr_amd import pose, predict

    dense = torch.zeros((2, 224, 224, 3), dtype=torch.uint8)
    p = predict.plan(dense)
    assert np.array_equal(p.T1[0], pose.initial_transform()) and np.array_equal(p.T1[1], pose.initial_transform())
    assert p.geom.tolist() == [[0, 224, 224, 0], [224 * 224 * 3, 224, 224, 0]]
    # ... and on another size it is the same rule on the image's own extent, box in float32
    p = predict.plan(_list_images([(97, 131)]))
    box = pose.modify_bbox(np.array([0, 0, 131, 97], dtype=np.float32), pose.BBOX_SCALE)
    assert np.array_equal(p.T1[0], pose.create_affine_transform_from_bbox(box, 224))


def test_left_hand_boxes_are_mirrored_before_T1():
    from peclr_amd import pose, predict

    assert predict.mirror_box([10.0, 20.0, 50.5, 90.0], 131).tolist() == [130 - 50.5, 20.0, 120.0, 90.0]
    boxes = _boxes()
    left = np.array([True, False, True])
    p = predict.plan(_list_images(), boxes=boxes, is_left=left)
    assert p.geom[:, 3].tolist() == [1, 0, 1]
    for i, (h, w) in enumerate(SIZES):
        x1, y1, x2, y2 = boxes[i]
        box = np.array([(w - 1) - x2, y1, (w - 1) - x1, y2]) if left[i] else boxes[i].copy()
        assert np.array_equal(p.T1[i], pose.create_affine_transform_from_bbox(pose.modify_bbox(box, 1.0), 224)), i
    # a torch.bool tensor and a list of bools are the same flags
    for flags in (torch.tensor([True, False, True]), [True, False, True]):
        assert np.array_equal(predict.plan(_list_images(), boxes=boxes, is_left=flags).T1, p.T1)


def test_mirrored_camera_follows_the_rule():
    from peclr_amd import predict

    rng = np.random.default_rng(3)
    for w in (1, 131, 320):
        K = [[rng.uniform(300, 500), rng.uniform(-1, 1), rng.uniform(50, 200)], [rng.uniform(-1, 1), rng.uniform(300, 500), rng.uniform(50, 200)],
             [rng.uniform(-1e-3, 1e-3), rng.uniform(-1e-3, 1e-3), 1.0]]
        r = [float(w - 1) * K[2][c] - K[0][c] for c in range(3)]           # Python floats: float64, one product, one difference
        want = [[-r[0], r[1], r[2]], [-K[1][0], K[1][1], K[1][2]], [-K[2][0], K[2][1], K[2][2]]]
        got = predict.flip_camera(np.array(K), w)
        assert got.dtype == np.float64 and got.tolist() == want
    # a point of the mirrored scene lands on the mirrored pixel
    K = np.array([[400.0, 0, 60.0], [0, 410.0, 50.0], [0, 0, 1.0]])
    X = np.array([0.03, -0.02, 0.6])
    u = K @ X
    uf = predict.flip_camera(K, 131) @ (X * [-1, 1, 1])
    np.testing.assert_allclose(uf[:2] / uf[2], [130 - u[0] / u[2], u[1] / u[2]], rtol=1e-12)


# ------------------------------------------------------------------ refusals
class _Tripwire:
    def __init__(self, what):
        self.what = what

    def __call__(self, *a, **k):
        raise AssertionError(f"{self.what} touched")

    def __getattr__(self, name):
        raise AssertionError(f"{self.what}.{name} touched")


@pytest.fixture
def host_predictor(monkeypatch):
    """A HandPosePredictor that never got a device (its constructor needs one): only the host half of a call can run.  The
    binding is the test double plus tripwires on the library and on everything the predictor launches."""
    from peclr_amd import _capi, predict

    _capi_double.install(monkeypatch)
    for name in ("lib", "_launch", "_call", "pose_crop", "pose_crop_ragged", "pose_head", "pose_unmap"):
        monkeypatch.setattr(_capi, name, _Tripwire(f"_capi.{name}"))
    monkeypatch.setattr(torch, "cuda", _Tripwire("torch.cuda"))
    monkeypatch.setattr(predict.HandPosePredictor, "_data", _Tripwire("HandPosePredictor._data"))     # the first device-side step
    p = object.__new__(predict.HandPosePredictor)
    p.size, p.bbox_scale, p.box_scale = 224, 0.33, 1.0
    p.model = p.device = p._table = _Tripwire("the device side of the predictor")
    p._graph = None
    return p


def _ok_args():
    K = np.stack([np.array([[400.0, 0, 112], [0, 400.0, 112], [0, 0, 1]])] * 3)
    return dict(images=_list_images(), K=K, scale=np.array([0.03, 0.03, 0.03]), boxes=_boxes(), is_left=np.array([False, True, False]))


def _bad_ragged():
    from peclr_amd.augment import RaggedImages

    r = RaggedImages(torch.zeros(3 * (4 * 5 + 2 * 3), dtype=torch.uint8), [(4, 5), (2, 3)])
    r.sizes[1] = (2, 4)                      # the second image now ends 6 bytes past the buffer
    return r


REFUSALS = [
    ("images", lambda a: [im.astype(np.float32) for im in a["images"]], TypeError, "image 0"),
    ("images", lambda a: a["images"][:2] + [np.zeros((5, 5), np.uint8)], ValueError, "image 2"),
    ("images", lambda a: torch.zeros((3, 8, 8, 4), dtype=torch.uint8), ValueError, "images"),
    ("images", lambda a: torch.zeros((3, 8, 8, 3), dtype=torch.float32), TypeError, "uint8"),
    ("images", lambda a: [], ValueError, "empty"),
    ("images", lambda a: "frames/", TypeError, "images"),
    ("K", lambda a: a["K"][:2], ValueError, "K"),
    ("K", lambda a: a["K"].reshape(3, 9), ValueError, "K"),
    ("K", lambda a: a["K"].astype(np.int64), TypeError, "K"),
    ("scale", lambda a: a["scale"][:2], ValueError, "scale"),
    ("scale", lambda a: torch.tensor([1, 1, 1]), TypeError, "scale"),
    ("is_left", lambda a: np.array([0, 1, 0]), TypeError, "is_left"),
    ("is_left", lambda a: np.array([False, True]), ValueError, "is_left"),
    ("boxes", lambda a: a["boxes"][:2], ValueError, "boxes"),
    ("boxes", lambda a: a["boxes"][:, :3], ValueError, "boxes"),
    ("boxes", lambda a: a["boxes"].astype(bool), TypeError, "boxes"),
    ("boxes", lambda a: np.where(np.arange(12).reshape(3, 4) == 6, np.nan, a["boxes"]), ValueError, "sample 1"),
    ("boxes", lambda a: np.where(np.arange(12).reshape(3, 4) == 11, np.inf, a["boxes"]), ValueError, "sample 2"),
    ("boxes", lambda a: np.array([[0, 0, 10, 10], [5, 0, 5, 10], [0, 0, 10, 10.0]]), ValueError, "sample 1"),
    ("boxes", lambda a: np.array([[0, 0, 10, 10], [0, 0, 10, 10], [0, 7, 10, 3.0]]), ValueError, "sample 2"),
]


@pytest.mark.parametrize("key,spoil,error,names", REFUSALS, ids=[f"{r[0]}{i}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_before_the_binding_is_touched(host_predictor, key, spoil, error, names):
    args = _ok_args()
    args[key] = spoil(args)
    with pytest.raises(error, match=names):
        host_predictor.predict(**args)


def test_an_image_past_the_end_of_the_packed_buffer_is_refused(host_predictor):
    with pytest.raises(ValueError, match="sample 1.*ends past the packed buffer"):
        host_predictor.predict(_bad_ragged())


def test_good_arguments_get_past_the_host_checks(host_predictor):
    """The fixture itself: with nothing to refuse the call goes on to the device side, and that is what trips."""
    with pytest.raises(AssertionError, match="touched"):
        host_predictor.predict(**_ok_args())


def test_replay_refuses_another_length_and_more_bytes_before_any_device_call(host_predictor):
    p = host_predictor
    with pytest.raises(RuntimeError, match="capture"):
        p.replay(_list_images())
    total = 3 * (224 * 224 + 97 * 131 + 180 * 320)
    p._graph, p._batch, p._max_bytes = object(), 3, total - 1
    with pytest.raises(ValueError, match=f"at most {total - 1} bytes.*need {total}"):
        p.replay(**_ok_args())
    p._max_bytes = total
    with pytest.raises(ValueError, match="captured for 3 images, got 2"):
        p.replay(_list_images(SIZES[:2]))
    with pytest.raises(ValueError, match="sample 0"):           # the argument checks come first here too
        p.replay(_list_images(), boxes=np.zeros((3, 4)))
    with pytest.raises(AssertionError, match="touched"):        # ... and a batch that fits goes on to the device
        p.replay(**_ok_args())


def test_constructor_is_the_freihand_predictors(monkeypatch):
    """Precision and fold_bn are parsed by the shared constructor; a CPU model is refused under this class's name."""
    from peclr_amd import _capi, pose, predict

    assert issubclass(predict.HandPosePredictor, pose.FreiHANDPredictor)
    assert predict.HandPosePredictor._passes is pose.FreiHANDPredictor._passes
    assert predict.HandPosePredictor._raise_on_status is pose.FreiHANDPredictor._raise_on_status
    m = pose.RN25DwMLPref("rn50")
    with pytest.raises(ValueError, match="HandPosePredictor: precision"):
        predict.HandPosePredictor(m, precision="fp8")
    with pytest.raises(_capi.PeclrHipError, match="HandPosePredictor: the model must be on a HIP device"):
        predict.HandPosePredictor(m)


def test_new_entry_points_refuse_null_arguments_before_any_launch():
    from peclr_amd import _capi

    L = _capi.lib()
    assert L.peclr_pose_crop_ragged_u8(None, 100, 1, None, None, None, None, 224, None, None, None) == -1
    assert L.peclr_pose_unmap(None, None, None, None, None, 1, None, None, None, None) == -1


# ------------------------------------------------------------------ tools/pred_images.py
def test_pred_images_meta_validation():
    import pred_images

    K = [[400.0, 0, 112], [0, 400.0, 112], [0, 0, 1]]
    good = [{"file": "a.png", "K": K, "scale": 0.03, "box": [1, 2, 30, 40], "is_left": True, "uv": np.zeros((21, 2)).tolist()},
            {"file": "b.png", "K": K, "scale": 0.03, "box": [1, 2, 30, 40], "xyz": np.zeros((21, 3)).tolist()}]
    assert pred_images.check_meta(good, want_eval=True) is good
    assert pred_images.check_meta([{"file": "a.png"}]) == [{"file": "a.png"}]

    def bad(meta, match, **kw):
        with pytest.raises(ValueError, match=match):
            pred_images.check_meta(meta, **kw)

    bad({}, "non-empty JSON list")
    bad([], "non-empty JSON list")
    bad([{"K": K}], "record 0")
    bad([{"file": "a.png"}, {"file": "a.png"}], "record 1.*twice")
    bad([{"file": "a.png", "bbox": [0, 0, 1, 1]}], "record 0.*unknown key")
    bad([{"file": "a.png", "is_left": 1}], "record 0.*is_left")
    bad([{"file": "a.png", "K": [1, 2, 3]}], "record 0.*K must be numbers of shape \\[3, 3\\]")
    bad([{"file": "a.png", "box": [0, 0, 1]}], "record 0.*box")
    bad([{"file": "a.png", "box": [0, 0, 1, "x"]}], "record 0.*box")
    bad([{"file": "a.png", "scale": [0.03]}], "record 0.*scale")
    bad([{"file": "a.png", "scale": float("nan")}], "record 0.*scale is not finite")
    bad([{"file": "a.png", "uv": np.zeros((21, 3)).tolist()}], "record 0.*uv")
    bad([{"file": "a.png", "xyz": np.zeros((20, 3)).tolist()}], "record 0.*xyz")
    bad([{"file": "a.png", "box": [0, 0, 1, 1]}, {"file": "b.png"}], "record 1 \\(b.png\\): no box")
    bad([{"file": "a.png"}], "--eval needs ground truth", want_eval=True)
