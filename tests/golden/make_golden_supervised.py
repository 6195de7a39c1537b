"""Golden vectors for the supervised sample: one augmented view's labels (peclr_amd/supervised.py, csrc/labels.hip).

Run where the reference checkout is present (tests/golden/_ref_import.py names its place):

    python tests/golden/make_golden_supervised.py

Calls the reference's own `Data_Set.prepare_supervised_sample` (data_set.py:278-329) on a SimpleNamespace that carries
`config.use_palm`, under the cv2 pass-through stubs of make_golden_augment.py (same `make_sample` hands, same `random.seed`),
and the reference's `convert_to_2_5D` / `convert_2_5D_to_3D` (data_loader/utils.py).

Fixture: g13_supervised.json.  Arrays are base64 of little-endian float32 / float64 bytes ({"f32": ...} / {"f64": ...}, with
"shape"); T is a list of float64 numbers (JSON round-trips them exactly).  Per case:

  inputs   K, joints3D (and joints_raw when the sample brings its own), image size, flags, params, seed, use_palm
  draws    the crop boxes `get_crop_size` computed, the augmenter's angle / jitter / margin / colour factors afterwards, and
           the next `random.random()` (it pins how many draws were consumed)
  T        the reference's NumPy matrix, float64
  gold32   what the reference emitted (float32): joints, K, scale, joints3D, joints3D_recreated, joints_raw; and raw25 /
           raw_scale = convert_to_2_5D(K, joints3D) as the chain's first call returned them; z_root = get_root_depth on the
           emitted joints and K
  gold64   the same functions on .double() copies of the float32 tensors each stage read:
             raw25, raw_scale    convert_to_2_5D(K, joints3D)                                  [reads the inputs]
             joints, scale       use_palm off: transform_sample on raw25 (float64), raw_scale  [reads the inputs and T]
                                 use_palm on:  convert_to_2_5D(gold32 K, gold32 joints3D)
             K                   fl32(T) @ K
             joints3D, joints_raw  move_wrist_to_palm on the double copy (use_palm), else the input
             joints3D_recreated, z_root   convert_2_5D_to_3D / get_root_depth on gold32's joints, scale, K
The float64 replay of `transform_sample` must draw the same parameters and compute the same crop boxes and T (asserted).

`batched`: 8 hands through convert_2_5D_to_3D(..., is_batch=True), with and without Z_root_calc, gold32 and gold64.
`round_trip_rel`: the reference's own float32 round-trip error max |convert_2_5D_to_3D(*convert_to_2_5D(K, J), K) - J| /
max |J| over all hands of the file but the clamp case (whose wrist and index MCP share a pixel: the root depth is the
clamps' 500 and nothing is recovered).
"""
import base64
import json
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_augment as mga  # noqa: E402  (installs the stubs and the cv2 pass-throughs)

from src.data_loader.data_set import Data_Set  # noqa: E402
from src.data_loader.sample_augmenter import SampleAugmenter  # noqa: E402
from src.data_loader.utils import convert_2_5D_to_3D, convert_to_2_5D, get_root_depth  # noqa: E402

edict = mga.edict
RECIPE = ("color_jitter", "random_crop", "rotate", "crop", "resize")


def enc(t):
    a = t.detach().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = np.ascontiguousarray(a)
    kind = {np.dtype("float32"): "f32", np.dtype("float64"): "f64"}[a.dtype]
    return {kind: base64.b64encode(a.astype(a.dtype.newbyteorder("<")).tobytes()).decode(), "shape": list(a.shape)}


def discriminant(joints25d, k):
    """(a, b^2 - 4ac) of get_root_depth, to keep every case on one side of the clamps."""
    from src.data_loader.utils import get_zroot_constraint_terms
    x_n, y_n, z_n, x_m, y_m, z_m, c_ = get_zroot_constraint_terms(joints25d, torch.inverse(k), False)
    a = (x_n - x_m) ** 2 + (y_n - y_m) ** 2
    b = 2 * (z_n * (x_n ** 2 + y_n ** 2 - x_n * x_m - y_n * y_m) + z_m * (x_m ** 2 + y_m ** 2 - x_n * x_m - y_n * y_m))
    c = (x_n * z_n - x_m * z_m) ** 2 + (y_n * z_n - y_m * z_m) ** 2 + (z_n - z_m) ** 2 - c_
    return float(a), float(b ** 2 - 4 * a * c)


def fake_dataset(use_palm):
    fake = types.SimpleNamespace(transform=None, config=types.SimpleNamespace(use_palm=use_palm))
    fake.move_wrist_to_palm = lambda j: Data_Set.move_wrist_to_palm(fake, j)
    return fake


ROUND_TRIP = []


def run_case(name, on, seed, hw, centre, spread, params=None, use_palm=False, own_raw=False, clamp=False):
    p = dict(mga.PARAMS, **(params or {}))
    sample = mga.make_sample(seed, hw, centre, spread)
    if clamp:  # index MCP = 2 x wrist: both project to the same pixel, bit for bit, in either precision
        sample["joints3D"][2] = 2 * sample["joints3D"][0]
    k_in, j_in = sample["K"].clone(), sample["joints3D"].clone()
    raw_in = None
    if own_raw:
        g = np.random.default_rng(seed + 1000)
        raw_in = (j_in + torch.from_numpy((0.01 * g.standard_normal((21, 3))).astype(np.float32))).clone()

    def one_pass(joints_dtype):
        """The reference's augmenter on the seed: float32 = the chain itself, float64 = its replay on double joints."""
        aug = SampleAugmenter(edict(mga.flags(*on)), edict(p))
        boxes, seen = [], {}
        orig = aug.get_crop_size

        def spy(joints, jitter=None, crop_margin=None):
            out = orig(joints, jitter, crop_margin)
            boxes.append([int(v) for v in out])
            return out

        aug.get_crop_size = spy
        random.seed(seed)
        if joints_dtype == torch.float32:
            orig_transform = aug.transform_sample

            def transform_spy(image, joints, override_angle=None, override_jitter=None):
                seen["raw25"] = joints.clone()
                img, joints_out, t = orig_transform(image, joints, override_angle, override_jitter)
                seen["T"] = np.asarray(t, dtype=np.float64).copy()
                seen["out_shape"] = list(img.shape)
                return img, joints_out, t

            aug.transform_sample = transform_spy
            s = {"image": sample["image"], "K": k_in.clone(), "joints3D": j_in.clone(), "joints_valid": torch.ones(21, 1)}
            if raw_in is not None:
                s["joints_raw"] = raw_in.clone()
            out = Data_Set.prepare_supervised_sample(fake_dataset(use_palm), s, aug)
        else:
            raw25, _ = convert_to_2_5D(k_in.double(), j_in.double())
            _, joints_out, t = aug.transform_sample(sample["image"], raw25)
            seen["T"] = np.asarray(t, dtype=np.float64).copy()
            out = {"joints": joints_out}
        draws = {"angle": aug.angle, "jitter_x": aug.jitter_x, "jitter_y": aug.jitter_y, "crop_margin_scale": aug._crop_margin_scale,
                 "h": aug.h, "s": aug.s, "a": aug.a, "b": aug.b, "next_random": random.random()}
        return out, boxes, seen, draws

    out, boxes, seen, draws = one_pass(torch.float32)
    out64, boxes64, seen64, draws64 = one_pass(torch.float64)
    assert boxes64 == boxes and draws64 == draws and np.array_equal(seen64["T"], seen["T"]), name
    for key in ("joints", "K", "joints3D", "joints3D_recreated", "joints_raw", "T"):
        assert out[key].dtype == torch.float32, (key, out[key].dtype)
    T = seen["T"]
    assert torch.equal(out["T"], torch.tensor(T, dtype=torch.float32))

    raw25_32, raw_scale32 = convert_to_2_5D(k_in.clone(), j_in.clone())
    assert torch.equal(raw25_32, seen["raw25"])
    raw25_64, raw_scale64 = convert_to_2_5D(k_in.double(), j_in.double())
    fake = fake_dataset(use_palm)
    if use_palm:
        joints64, scale64 = convert_to_2_5D(out["K"].double(), out["joints3D"].double())
        j3d64 = fake.move_wrist_to_palm(j_in.double())
        rawj64 = fake.move_wrist_to_palm((j_in if raw_in is None else raw_in).double())
    else:
        joints64, scale64 = out64["joints"], raw_scale64
        j3d64, rawj64 = j_in.double(), (j_in if raw_in is None else raw_in).double()
    rec64 = convert_2_5D_to_3D(out["joints"].double(), out["scale"].double(), out["K"].double())
    z32, _ = get_root_depth(out["joints"], out["K"])
    z64, _ = get_root_depth(out["joints"].double(), out["K"].double())
    for t in (joints64, scale64, rec64, z64, raw25_64):
        assert t.dtype == torch.float64
    a, disc = discriminant(out["joints"].double(), out["K"].double())
    a32, disc32 = discriminant(out["joints"], out["K"])
    if clamp:
        assert a == 0.0 and a32 == 0.0 and disc == 0.0 and disc32 == 0.0, (a, a32, disc, disc32)
    else:  # at least 10 x above both clamps, in both precisions
        assert min(a, a32) > 1e-5 and min(disc, disc32) > 1e-5, (name, a, a32, disc, disc32)
        back = convert_2_5D_to_3D(raw25_32, raw_scale32, k_in)
        ROUND_TRIP.append(float((back - j_in).abs().max() / j_in.abs().max()))

    gold32 = {k: enc(out[k]) for k in ("joints", "K", "joints3D", "joints3D_recreated", "joints_raw")}
    gold32.update(scale=enc(out["scale"].reshape(1)), raw25=enc(raw25_32), raw_scale=enc(raw_scale32.reshape(1)),
                  z_root=enc(z32.reshape(1)))
    gold64 = {"joints": enc(joints64), "K": enc(torch.tensor(T, dtype=torch.float32).double() @ k_in.double()),
              "scale": enc(scale64.reshape(1)), "joints3D": enc(j3d64), "joints3D_recreated": enc(rec64),
              "joints_raw": enc(rawj64), "raw25": enc(raw25_64), "raw_scale": enc(raw_scale64.reshape(1)),
              "z_root": enc(z64.reshape(1))}
    if not use_palm and raw_in is None:  # the inputs again: not stored twice
        for g in (gold32, gold64):
            del g["joints3D"], g["joints_raw"]
    case = {"name": name, "flags_on": list(on), "params": p, "seed": seed, "image_hw": list(hw), "use_palm": use_palm,
            "clamp": clamp, "K": enc(k_in), "joints3D": enc(j_in), "boxes": boxes, "draws": draws, "out_shape": seen["out_shape"],
            "T": T.tolist(), "gold32": gold32, "gold64": gold64}
    if raw_in is not None:
        case["joints_raw"] = enc(raw_in)
    return case


def batched_block():
    ks, js, j25, sc = [], [], [], []
    for i in range(8):
        s = mga.make_sample(200 + i, (224, 224), (100 + 5 * i, 120 - 4 * i), 20 + 2 * i)
        a, b = convert_to_2_5D(s["K"], s["joints3D"])
        ks.append(s["K"]), js.append(s["joints3D"]), j25.append(a), sc.append(b)
        back = convert_2_5D_to_3D(a, b, s["K"])
        ROUND_TRIP.append(float((back - s["joints3D"]).abs().max() / s["joints3D"].abs().max()))
    k, j25, sc = torch.stack(ks), torch.stack(j25), torch.stack(sc)
    z_calc = torch.tensor([3.0 + 0.37 * i for i in range(8)], dtype=torch.float32)
    z32, _ = get_root_depth(j25, k, True)
    z64, _ = get_root_depth(j25.double(), k.double(), True)
    return {"K": enc(k), "joints3D": enc(torch.stack(js)), "joints25D": enc(j25), "scale": enc(sc), "z_root_calc": enc(z_calc),
            "gold32": {"joints3D": enc(convert_2_5D_to_3D(j25, sc, k, True)), "z_root": enc(z32),
                       "joints3D_calc": enc(convert_2_5D_to_3D(j25, sc, k, True, z_calc))},
            "gold64": {"joints3D": enc(convert_2_5D_to_3D(j25.double(), sc.double(), k.double(), True)), "z_root": enc(z64),
                       "joints3D_calc": enc(convert_2_5D_to_3D(j25.double(), sc.double(), k.double(), True, z_calc.double()))}}


def main():
    torch.set_num_threads(1)
    cases = []
    for seed in range(6):
        cases.append(run_case(f"recipe_{seed}", RECIPE, 100 + seed, (224, 224), (112 + 9 * seed, 108 - 7 * seed), 24 + 3 * seed))
    cases.append(run_case("nocrop", ("resize", "color_jitter"), 21, (240, 320), (170, 110), 35))
    cases.append(run_case("nocrop_rotate", ("rotate", "resize", "random_crop"), 22, (240, 320), (150, 120), 30))
    cases.append(run_case("border_topleft", RECIPE, 7, (224, 224), (20, 14), 30))          # crop origin clamped at 0
    cases.append(run_case("border_bottomright", RECIPE, 8, (224, 224), (205, 214), 28))    # window truncated by the slice
    cases.append(run_case("palm_0", RECIPE, 31, (224, 224), (110, 115), 25, use_palm=True))
    cases.append(run_case("palm_1", RECIPE, 32, (224, 224), (125, 100), 22, use_palm=True))
    cases.append(run_case("own_raw", RECIPE, 33, (224, 224), (105, 118), 24, own_raw=True))
    cases.append(run_case("palm_own_raw", RECIPE, 35, (224, 224), (115, 108), 24, use_palm=True, own_raw=True))
    cases.append(run_case("resize_448", RECIPE, 11, (224, 224), (100, 120), 26, {"resize_shape": [448, 448]}))
    cases.append(run_case("clamp", RECIPE, 34, (224, 224), (112, 112), 20, clamp=True))
    doc = {"cases": cases, "batched": batched_block(), "round_trip_rel": max(ROUND_TRIP)}
    path = os.path.join(HERE, "g13_supervised.json")
    with open(path, "w") as f:
        json.dump(doc, f)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases; round trip", doc["round_trip_rel"])
    for c in cases:
        print(c["name"], c["boxes"], c["out_shape"], c["draws"]["next_random"])


if __name__ == "__main__":
    main()
