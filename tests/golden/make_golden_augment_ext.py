"""Golden vectors for the PARAMETER side of the reference's other five augmentations (sobel_filter, cut_out,
gaussian_blur, gaussian_noise, color_drop), as TwoViewAugmenter(extended=True) draws them.

Needs a checkout of the reference (REFERENCE_ROOT in _ref_import.py); not run by the tests:

    python tests/golden/make_golden_augment_ext.py

Same pattern as make_golden_augment.py: the reference's own `SampleAugmenter.transform_sample`
(sample_augmenter.py:47-129) and `Data_Set.prepare_hybrid2_sample` (data_set.py:357-384) run under
stubs for what they delegate to OpenCV.  The new stubs record their arguments and keep shapes:
`cvtColor(BGR2GRAY)` returns a 2-D zero image, `Sobel` a float64 zero image, `GaussianBlur` its input,
`randn` its (zero) destination.  Both global generators are seeded (`random.seed`, `np.random.seed`).

Recorded per view: the five decisions, cut-out's joint, box and fill, blur's ksize and sigma; per case:
the emitted dict and the next `random.random()` / `np.random.randint(2**31)` after the sample, which
pin the NUMBER of draws.  Fixture: g10_augment_ext_params.json.
"""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_augment as base  # noqa: E402  (installs the stubs and imports the reference)

cv2 = sys.modules["cv2"]
CALLS = base.CALLS
cv2.COLOR_BGR2GRAY, cv2.CV_64F = 6, 6
_cvt = cv2.cvtColor


def _cvt_color(img, code):
    if code == cv2.COLOR_BGR2GRAY:
        return np.zeros(img.shape[:2], dtype=img.dtype)
    return _cvt(img, code)


def _sobel(img, depth, dx, dy, ksize=3):
    CALLS.append(("Sobel", dx, dy, ksize))
    return np.zeros(img.shape[:2], dtype=np.float64)


def _gaussian_blur(img, ksize, sigma):
    CALLS.append(("GaussianBlur", [int(k) for k in ksize], float(sigma)))
    return img


def _randn(dst, mean, std):
    CALLS.append(("randn",))
    return dst


cv2.cvtColor, cv2.Sobel, cv2.GaussianBlur, cv2.randn = _cvt_color, _sobel, _gaussian_blur, _randn

from src.data_loader.data_set import Data_Set  # noqa: E402
from src.data_loader.sample_augmenter import SampleAugmenter  # noqa: E402

RECIPE = ("color_jitter", "random_crop", "rotate", "crop", "resize")
NEW = ("sobel_filter", "cut_out", "gaussian_blur", "gaussian_noise", "color_drop")


def run_case(name, on, seed, hw, centre, spread, params=None):
    p = dict(base.PARAMS, **(params or {}))
    aug = SampleAugmenter(base.edict(base.flags(*on)), base.edict(p))
    views, cur = [], {}
    randint = np.random.randint

    def randint_spy(*a, **k):
        out = randint(*a, **k)
        cur.setdefault("np_draws", []).append([list(a), np.asarray(out).tolist()])
        return out

    orig_box = aug.get_random_cut_out_box

    def box_spy(d0, d1, c0, c1):
        out = orig_box(d0, d1, c0, c1)
        cur["cut_out_box"] = {"rows": [int(v) for v in out[0]], "cols": [int(v) for v in out[1]]}
        return out

    aug.get_random_cut_out_box = box_spy
    orig_transform = aug.transform_sample

    def transform_spy(image, joints, override_angle=None, override_jitter=None):
        CALLS.clear()
        cur.clear()
        np.random.randint = randint_spy
        try:
            out = orig_transform(image, joints, override_angle, override_jitter)
        finally:
            np.random.randint = randint
        rec = {"sobel": aug._sobel_filter, "cut_out": aug._cut_out, "blur": aug._gaussian_blur,
               "noise": aug._gaussian_noise, "color_drop": aug._color_drop}
        if aug._cut_out:
            (_, joint), (_, fill) = cur["np_draws"]
            rec.update(cut_out_joint=int(joint[0]), cut_out_fill=int(fill[0]), **cur["cut_out_box"])
        blur = [c for c in CALLS if c[0] == "GaussianBlur"]
        if blur:
            rec.update(blur_ksize=blur[0][1], blur_sigma=blur[0][2])
        views.append(rec)
        return out

    aug.transform_sample = transform_spy
    sample = base.make_sample(seed, hw, centre, spread)
    fake = type("Fake", (), {"transform": None})()
    fake.get_random_augment_param = lambda a: Data_Set.get_random_augment_param(fake, a)
    random.seed(seed)
    np.random.seed(seed)
    out = Data_Set.prepare_hybrid2_sample(fake, sample, aug)
    probes = {"random": random.random(), "np_randint": int(np.random.randint(2 ** 31))}
    emitted = {}
    for k, v in out.items():
        if k.startswith("transformed_image"):
            continue
        emitted[k] = {"type": type(v).__name__, "value": (bool(v) if isinstance(v, bool) else float(v))}
    return {"name": name, "flags_on": list(on), "params": p, "seed": seed, "image_hw": list(hw),
            "K": sample["K"].numpy().tolist(), "joints3D": sample["joints3D"].double().numpy().tolist(),
            "views": views, "emitted": emitted, "probes": probes}


def first_case(pred, name, on, seed, *a, **k):
    """The first seed from `seed` on whose case satisfies `pred` (so each case exercises what it is named for)."""
    for s in range(seed, seed + 200):
        c = run_case(name, on, s, *a, **k)
        if pred(c):
            return c
    raise RuntimeError(f"no seed for {name}")


def fired(key):
    return lambda c: any(v[key] for v in c["views"])


def main():
    import torch

    torch.set_num_threads(1)
    cases = []
    for i, flag in enumerate(NEW):
        for j in range(3):
            seed = 200 + 10 * i + j
            cases.append(run_case(f"{flag}_{j}", RECIPE + (flag,), seed, (224, 224), (112 + 5 * j, 108 - 4 * j), 24 + 2 * j))
    for j in range(4):
        cases.append(run_case(f"all_ten_{j}", RECIPE + NEW, 300 + j, (224, 224), (110 + 6 * j, 112 - 3 * j), 25))
    cases.append(first_case(fired("blur"), "all_ten_wide_240x320", RECIPE + NEW, 310, (240, 320), (170, 110), 35))
    cases.append(first_case(fired("blur"), "all_ten_480x640", RECIPE + NEW, 320, (480, 640), (330, 250), 60))

    def clipped(c):
        return any(v["cut_out"] and (v["rows"][0] == 0 or v["cols"][0] == 0) for v in c["views"])

    cases.append(first_case(clipped, "cut_out_border", RECIPE + ("cut_out",), 330, (224, 224), (16, 12), 10,
                            {"cut_out_fraction": [0.1, 0.16]}))
    cases.append(first_case(fired("cut_out"), "cut_out_top_fraction", RECIPE + ("cut_out",), 340, (224, 224), (112, 112), 25,
                            {"cut_out_fraction": [0.16, 0.16]}))
    cases.append(run_case("all_ten_448", RECIPE + NEW, 350, (224, 224), (100, 120), 26, {"resize_shape": [448, 448]}))
    cases.append(run_case("new_only", ("resize",) + NEW, 360, (224, 224), (112, 112), 25))
    path = os.path.join(HERE, "g10_augment_ext_params.json")
    with open(path, "w") as f:
        json.dump({"cases": cases}, f)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases")
    for c in cases:
        print(c["name"], c["seed"], [{k: v for k, v in w.items() if v} for w in c["views"]])


if __name__ == "__main__":
    main()
