"""The supervised sample on the device (csrc/labels.hip, peclr_amd/supervised.py) against the reference's own results
(tests/golden/g13_supervised.json) and the float64 restatement tests/supervised_ref.py (held to the reference at 1e-12 by
tests/test_supervised_host.py).

The bounds.  The kernels evaluate a stage in float64 and round once, so against the reference's float64 result ON THE SAME
INPUTS (gold64) every element satisfies |dev - gold64| <= 2^-23 |gold64|: half a float32 ulp for the rounding, the rest
slack for float64 evaluation order; the absolute floor 2^-40 x the sample's largest magnitude covers elements that cancel to
(almost) nothing.  Against the reference's float32 result the triangle inequality gives |dev - gold32| <= |gold32 - gold64|
+ the same.  Both are stated for equal inputs, so:
  * `joints3d_to_25d` and `joints25d_to_3d` are fed exactly the float32 tensors the reference's stage read;
  * of the label launch, T, K', and without use_palm `joints` and `scale` read the sample's inputs alone and are held to gold64
    / gold32 directly; `joints3D` / `joints_raw` are one exact-or-once-rounded mean;
  * the stages that read an EMITTED tensor (use_palm's joints and scale read K'; the re-creation reads joints, scale, K') see
    the device's own float32 values, which may differ from the reference's float32 ones in the last bit.  They are held bit
    for bit to the entry point of that stage run on the device's emitted tensors, and to the restatement on the same tensors.
"""
import random

import numpy as np
import pytest
import torch

from tests import supervised_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIX = ref.load_fixture()
CASES = FIX["cases"]
EPS, FLOOR = 2.0 ** -23, 2.0 ** -40


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def per_sample_max(a):
    a = np.abs(a)
    return a.reshape(a.shape[0], -1).max(axis=1).reshape((-1,) + (1,) * (a.ndim - 1))


def check(got, g64, g32=None, what=""):
    """got, g64, g32: [B, ...].  The two bounds of the module docstring, element by element; prints the worst ratio."""
    got, g64 = np.asarray(got, np.float64), np.asarray(g64, np.float64)
    assert got.shape == g64.shape, (what, got.shape, g64.shape)
    bound = np.maximum(EPS * np.abs(g64), FLOOR * per_sample_max(g64))
    err = np.abs(got - g64)
    print(f"{what}: worst |dev - gold64| / bound = {np.max(err / np.where(bound == 0, 1, bound)):.3f}")
    assert np.all(err <= bound), (what, float(np.max(err - bound)))
    if g32 is not None:
        g32 = np.asarray(g32, np.float64)
        err32, bound32 = np.abs(got - g32), np.abs(g32 - g64) + bound
        print(f"{what}: worst |dev - gold32| / bound = {np.max(err32 / np.where(bound32 == 0, 1, bound32)):.3f}")
        assert np.all(err32 <= bound32), (what, float(np.max(err32 - bound32)))


def gold(cases, key, which):
    """[B, ...] stack of one fixture entry; joints3D / joints_raw fall back to the inputs where the fixture does not repeat them."""
    out = []
    for c in cases:
        if key in c[which]:
            a = ref.dec(c[which][key])
        else:
            a = ref.dec(c["joints_raw"] if key == "joints_raw" and "joints_raw" in c else c["joints3D"])
        out.append(a.astype(np.float64))
    a = np.stack(out)
    return a.reshape(len(cases)) if a.shape[1:] == (1,) else a


def inputs(cases):
    return dev32(np.stack([ref.dec(c["K"]) for c in cases])), dev32(np.stack([ref.dec(c["joints3D"]) for c in cases]))


def hands(n, seed, hw=(224, 224), focal=480.0):
    """n synthetic hands of make_sample's kind -> (K [n,3,3], joints3D [n,21,3]) float32 NumPy arrays."""
    g = np.random.default_rng(seed)
    k = np.array([[focal, 0, hw[1] / 2], [0, focal, hw[0] / 2], [0, 0, 1]], dtype=np.float32)
    out = []
    for _ in range(n):
        z = 0.6 + 0.05 * g.standard_normal(21)
        u = g.uniform(0.35, 0.65) * hw[1] + min(hw) / 9 * g.standard_normal(21)
        v = g.uniform(0.35, 0.65) * hw[0] + min(hw) / 9 * g.standard_normal(21)
        out.append(np.stack([(u - k[0, 2]) * z / focal, (v - k[1, 2]) * z / focal, z], axis=1))
    return np.repeat(k[None], n, 0), np.array(out, dtype=np.float32)


# ------------------------------------------------------------------ 1. each entry point against the reference
def test_joints3d_to_25d_against_the_reference():
    from peclr_amd import joints3d_to_25d

    K, J = inputs(CASES)
    j25, scale = joints3d_to_25d(K, J)
    assert j25.dtype == torch.float32 and tuple(j25.shape) == (len(CASES), 21, 3) and tuple(scale.shape) == (len(CASES),)
    check(host(j25), gold(CASES, "raw25", "gold64"), gold(CASES, "raw25", "gold32"), "joints25D")
    check(host(scale), gold(CASES, "raw_scale", "gold64"), gold(CASES, "raw_scale", "gold32"), "scale")


def test_joints25d_to_3d_and_root_depth_against_the_reference():
    """On the float32 joints, scale and K' the reference's re-creation read -- the clamp case among them: its wrist and
    index MCP share a pixel, a = 0 and b = 0 exactly, and both clamps give the root depth 0.5 sqrt(1e-6) / 1e-6."""
    from peclr_amd import joints25d_to_3d, root_depth

    j25, s, k = (dev32(gold(CASES, key, "gold32")) for key in ("joints", "scale", "K"))
    out = joints25d_to_3d(j25, s, k)
    check(host(out), gold(CASES, "joints3D_recreated", "gold64"), gold(CASES, "joints3D_recreated", "gold32"), "joints3D")
    zr = root_depth(j25, k)
    check(host(zr), gold(CASES, "z_root", "gold64"), gold(CASES, "z_root", "gold32"), "z_root")
    i = next(i for i, c in enumerate(CASES) if c["clamp"])
    assert float(zr[i]) == float(np.float32(0.5 * np.sqrt(1e-6) / 1e-6))


def test_batched_block_with_and_without_z_root_calc():
    from peclr_amd import joints25d_to_3d, root_depth

    blk = FIX["batched"]
    k, j25, sc, zc = (dev32(ref.dec(blk[n])) for n in ("K", "joints25D", "scale", "z_root_calc"))
    g32 = {n: ref.dec(v).astype(np.float64) for n, v in blk["gold32"].items()}
    g64 = {n: ref.dec(v) for n, v in blk["gold64"].items()}
    check(host(joints25d_to_3d(j25, sc, k)), g64["joints3D"], g32["joints3D"], "joints3D")
    check(host(joints25d_to_3d(j25, sc, k, zc)), g64["joints3D_calc"], g32["joints3D_calc"], "joints3D with z_root_calc")
    check(host(root_depth(j25, k)), g64["z_root"], g32["z_root"], "z_root")


@pytest.mark.parametrize("use_palm", [False, True], ids=["plain", "use_palm"])
def test_supervised_labels_against_the_reference(use_palm):
    from peclr_amd import _capi, joints3d_to_25d, joints25d_to_3d

    cases = [c for c in CASES if c["use_palm"] == use_palm]
    assert len(cases) >= 2
    K, J = inputs(cases)
    T64 = torch.tensor([c["T"] for c in cases], dtype=torch.float64)
    # (a sample without joints_raw of its own gets a clone of its joints3D in the reference: the same tensor)
    raw = dev32(np.stack([ref.dec(c["joints_raw"] if "joints_raw" in c else c["joints3D"]) for c in cases]))
    out = _capi.supervised_labels(K, J, T64.to(DEV), use_palm, raw)
    assert torch.equal(out["T"].cpu(), T64.to(torch.float32)), "T is the float32 of the reference's matrix, exactly"
    without = _capi.supervised_labels(K, J, T64.to(DEV), use_palm, None)      # no joints_raw given: joints3D stands in
    rows = [i for i, c in enumerate(cases) if "joints_raw" not in c]
    assert rows and all(torch.equal(without[key][rows], out[key][rows]) for key in out)
    check(host(out["K"]), gold(cases, "K", "gold64"), gold(cases, "K", "gold32"), "K'")
    check(host(out["joints3D"]), gold(cases, "joints3D", "gold64"), gold(cases, "joints3D", "gold32"), "joints3D")
    check(host(out["joints_raw"]), gold(cases, "joints_raw", "gold64"), gold(cases, "joints_raw", "gold32"), "joints_raw")
    if use_palm:
        # joints and scale read the emitted K' and joints3D: the stage, on the device's own tensors
        j25, scale = joints3d_to_25d(out["K"], out["joints3D"])
        assert torch.equal(out["joints"], j25) and torch.equal(out["scale"], scale)
    else:
        check(host(out["joints"]), gold(cases, "joints", "gold64"), gold(cases, "joints", "gold32"), "joints")
        check(host(out["scale"]), gold(cases, "scale", "gold64"), gold(cases, "scale", "gold32"), "scale")
    assert torch.equal(out["joints3D_recreated"], joints25d_to_3d(out["joints"], out["scale"], out["K"]))
    # ... and each such stage is the restatement's on what the device emitted
    for i, c in enumerate(cases):
        if use_palm:
            j25, scale = ref.to_25d(host(out["K"][i]), host(out["joints3D"][i]))
            check(host(out["joints"][i])[None], j25[None], what=f"{c['name']} joints")
            check(host(out["scale"][i]).reshape(1, 1), np.reshape(scale, (1, 1)), what=f"{c['name']} scale")
        rec, _ = ref.to_3d(host(out["joints"][i]), host(out["scale"][i]), host(out["K"][i]))
        check(host(out["joints3D_recreated"][i])[None], rec[None], what=f"{c['name']} joints3D_recreated")


# ------------------------------------------------------------------ 2. batch sizes: 65 is one past a wave and past a 64-sample block
def test_batch_sizes_and_every_sample_as_it_would_be_alone():
    from peclr_amd import _capi, joints3d_to_25d, joints25d_to_3d

    n = 65
    k_np, j_np = hands(n, 7)
    g = np.random.default_rng(8)
    K, J = dev32(k_np), dev32(j_np)
    T = torch.from_numpy(np.array([[[c * 0.9, s, 7.0 * i], [-s, c * 1.1, 3.0 - i], [0, 0, 1]]
                                   for i, (c, s) in enumerate(zip(np.cos(g.uniform(-1, 1, n)), np.sin(g.uniform(-1, 1, n))))])).to(DEV)
    raw = dev32(j_np + 0.01 * g.standard_normal(j_np.shape))
    zc = dev32(g.uniform(2.0, 6.0, n))

    def run(sl):
        j25, scale = joints3d_to_25d(K[sl], J[sl])
        out = [j25, scale, *_capi.joints25d_to_3d(j25, scale, K[sl]), joints25d_to_3d(j25, scale, K[sl], zc[sl])]
        for palm in (False, True):
            d = _capi.supervised_labels(K[sl], J[sl], T[sl], palm, raw[sl])
            out += [d[key] for key in sorted(d)]
        return out

    whole = run(slice(0, n))
    # against the restatement, so that "the same everywhere" is also "right" (sample 64 sits alone in the last wave's block)
    for i in (0, 63, 64):
        j25, scale = ref.to_25d(k_np[i], j_np[i])
        check(host(whole[0][i])[None], j25[None], what=f"joints25D[{i}]")
        back, zr = ref.to_3d(host(whole[0][i]), host(whole[1][i]), k_np[i])
        check(host(whole[2][i])[None], back[None], what=f"joints3D[{i}]")
        check(host(whole[3][i]).reshape(1, 1), np.reshape(zr, (1, 1)), what=f"z_root[{i}]")
        check(host(whole[4][i])[None], ref.to_3d(host(whole[0][i]), host(whole[1][i]), k_np[i], host(zc[i]))[0][None],
              what=f"joints3D with z_root_calc [{i}]")
    for b in (1, 3):
        for full, part in zip(whole, run(slice(0, b))):
            assert torch.equal(full[:b], part), b
    for i in range(n):
        for full, alone in zip(whole, run(slice(i, i + 1))):
            assert torch.equal(full[i:i + 1], alone), i


# ------------------------------------------------------------------ 3. pixels: the existing launches with one view
def _pixel_batch(sizes, seed):
    from tests.test_augment_ragged_gpu import synth_image

    images = [synth_image(40 + i, hw) for i, hw in enumerate(sizes)]
    ks, js = [], []
    for i, hw in enumerate(sizes):
        k, j = hands(1, seed + i, hw, focal=200.0)
        ks.append(k[0]), js.append(j[0])
    return images, torch.from_numpy(np.array(ks)), torch.from_numpy(np.array(js))


@pytest.mark.parametrize("hw", [(96, 96), (72, 120)], ids=["96x96", "72x120"])
@pytest.mark.parametrize("crop", [True, False], ids=["crop", "whole_image"])
def test_image_is_the_existing_launches_with_one_view(hw, crop):
    from peclr_amd import SupervisedAugmenter, _capi
    from peclr_amd.augment import IMAGENET_MEAN, IMAGENET_STD, RECIPE_FLAGS

    sizes = [hw] * 3
    images, K, J = _pixel_batch(sizes, 50)
    aug = SupervisedAugmenter(dict(RECIPE_FLAGS, crop=crop), {"resize_shape": [32, 32]}, rng=random.Random(9))
    stacked = torch.from_numpy(np.stack(images)).to(DEV)
    out = aug(stacked, K, J)
    assert out["image"].dtype == torch.float32 and tuple(out["image"].shape) == (3, 3, 32, 32)
    assert tuple(aug.last_params.shape) == (1, 3, 16)
    if not crop:
        assert all(w["crop"] == (0, 0, hw[1], hw[0]) for w in aug.last_views)
    want, _ = _capi.augment_views(stacked, aug.last_params, (32, 32), IMAGENET_MEAN, IMAGENET_STD, True)
    assert torch.equal(out["image"], want)
    # the labels of the same call: the label launch on the same T
    lab = _capi.supervised_labels(K.to(DEV), J.to(DEV), aug.last_T.to(DEV))
    for key, t in lab.items():
        assert torch.equal(out[key], t), key
    assert torch.equal(out["joints_valid"], torch.ones(3, 21, 1, device=DEV))


def test_ragged_batch_is_the_existing_ragged_launches():
    from peclr_amd import RaggedImages, SupervisedAugmenter, _capi
    from peclr_amd.augment import IMAGENET_MEAN, IMAGENET_STD

    sizes = [(96, 96), (72, 120), (96, 96)]
    images, K, J = _pixel_batch(sizes, 60)
    aug = SupervisedAugmenter(params={"resize_shape": [32, 32]}, rng=random.Random(10))
    out = aug(images, K, J)
    ragged = RaggedImages.from_list(images, DEV)
    geom, wins = aug.views.ragged_tables(sizes, ragged.offsets, [aug.last_views])
    want = _capi.augment_views_ragged(ragged.data, geom, wins, aug.last_params, (32, 32), IMAGENET_MEAN, IMAGENET_STD, True)[0]
    assert tuple(out["image"].shape) == (3, 3, 32, 32) and torch.equal(out["image"], want)
    # every sample as it would be alone through the uniform path
    for i, im in enumerate(images):
        alone = _capi.augment_views(torch.from_numpy(im)[None].to(DEV), aug.last_params[:, i:i + 1].contiguous(), (32, 32),
                                    IMAGENET_MEAN, IMAGENET_STD, True)[0]
        assert torch.equal(out["image"][i:i + 1], alone), i


# ------------------------------------------------------------------ 4. round trip
def test_round_trip_within_the_reference_own_error():
    """joints25d_to_3d(*joints3d_to_25d(K, J), K) returns J within twice the reference's own float32 round-trip error on the
    same hands (the fixture's `round_trip_rel`, relative to the sample's largest coordinate; the clamp case recovers nothing
    in the reference either and is left out there and here).  2 x: the device rounds fewer times than the reference does."""
    from peclr_amd import joints3d_to_25d, joints25d_to_3d

    cases = [c for c in CASES if not c["clamp"]]
    k_np = np.concatenate([np.stack([ref.dec(c["K"]) for c in cases]), ref.dec(FIX["batched"]["K"])])
    j_np = np.concatenate([np.stack([ref.dec(c["joints3D"]) for c in cases]), ref.dec(FIX["batched"]["joints3D"])])
    K, J = dev32(k_np), dev32(j_np)
    back = host(joints25d_to_3d(*joints3d_to_25d(K, J), K))
    rel = np.abs(back - j_np).reshape(len(j_np), -1).max(1) / np.abs(j_np).reshape(len(j_np), -1).max(1)
    print(f"round trip: device worst {rel.max():.3e}, the reference's {FIX['round_trip_rel']:.3e}")
    assert np.all(rel <= 2 * FIX["round_trip_rel"])


# ------------------------------------------------------------------ 5. PoseEvaluator.update_25d
def test_update_25d_equals_update_on_the_lifted_joints_and_replays_from_a_graph():
    from peclr_amd import PoseEvaluator, joints3d_to_25d, joints25d_to_3d

    b = 5
    k_np, j_np = hands(b, 21)
    g = np.random.default_rng(22)
    K, gt = dev32(k_np), dev32(j_np)
    pred25, scale = joints3d_to_25d(K, dev32(j_np + 0.004 * g.standard_normal(j_np.shape)))

    def same(a, c):
        assert list(a) == list(c)
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(c[key]), equal_nan=True), key

    direct = PoseEvaluator(16, device=DEV)
    direct.update(joints25d_to_3d(pred25, scale, K), gt)
    eager = PoseEvaluator(16, device=DEV)
    eager.update_25d(pred25, scale, K, gt)
    same(eager.compute(), direct.compute())

    ev = PoseEvaluator(16, device=DEV)
    sp, ss, sk, sg = (torch.zeros_like(t) for t in (pred25, scale, K, gt))
    sk.copy_(K)                                                                # (a zero K has no inverse)
    ss.fill_(1.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.update_25d(sp, ss, sk, sg)
    for src, dst in ((pred25, sp), (scale, ss), (K, sk), (gt, sg)):
        dst.copy_(src)
    graph.replay()
    same(ev.compute(), direct.compute())
    with pytest.raises(ValueError, match="capacity"):
        PoseEvaluator(4, device=DEV).update_25d(pred25, scale, K, gt)
