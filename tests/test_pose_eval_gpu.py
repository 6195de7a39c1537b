"""Scoring pose predictions on the device: the `peclr_pose_eval` kernel, the reference-shaped functions and `PoseEvaluator`
against the recorded outputs of the reference (tests/golden/g12_pose_eval.*), and `tools/pred_freihand.py --eval`.

Bars (e_np64, e_ref32 and gap_min are the fixture's recorded figures, see tests/test_pose_eval_host.py):
  float64 Procrustes outputs   8 x e_np64 (floor 1e-13): aligned and translation relative to normX, rot_mat absolute, scale over
                               normX / normY
  float32 Procrustes outputs   distance to the float64 run <= e_ref32 of the case (the reference's own float32 error)
  raw distances                4 ulp of the dtype, relative, against the run of the same dtype; exact zeros stay exact
  PCK counts                   exact (no recorded distance lies within a relative 1e-5 of a threshold)
  AUC per joint                1e-7 absolute
  means (raw, 2D, aligned)     1e-6 relative to the reference's mean of the same dtype
  median, min, max of the raw distances: the distance bar
  aligned distances element by element, and their median: the issue sets no bar, and the raw distance bar cannot apply -- the
                               reference's own float32 run is off by 3.5e-5 on the x1000 row.  Held against the float64 run
                               instead: the points move by at most the Procrustes bar of the dtype, and a distance or an order
                               statistic moves no further than the points do (float32: e_ref32["aligned"] times sqrt(3) plus
                               one float32 rounding; float64: the float64 bar times normX times sqrt(3))
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import eval_ref
from tests.conftest import GOLDEN, ROOT, load_golden
from tests.test_pose_eval_host import CASES, f64_bar, fixture_gap, procrustes_errors

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = {"f32": torch.float32, "f64": torch.float64}
ULP = {"f32": 2.0 ** -23, "f64": 2.0 ** -52}
REF_KEYS = ("Mean_EPE_3D", "Median_EPE_3D", "AUC", "Mean_EPE_3D_procrustes", "Median_EPE_3D_procrustes", "auc_procrustes")


@pytest.fixture(scope="module")
def g12():
    with open(os.path.join(GOLDEN, "g12_pose_eval.json")) as f:
        meta = json.load(f)
    return load_golden("g12_pose_eval.npz"), meta


def _dev(a, name):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DTYPES[name]).to(DEV)


def _launch(pred, gt, name, thr=None, dim=3, procrustes=True):
    """One launch on NumPy clouds -> dict of NumPy outputs (+ counts [2,21,T] when thr is given)."""
    from peclr_amd import _capi

    p, g = _dev(pred, name), _dev(gt, name)
    counts = t = None
    if thr is not None:
        t = _dev(thr, name)
        counts = torch.zeros((2, 21, len(thr)), dtype=torch.int64, device=DEV)
    out = _capi.pose_eval(p, g, dim=dim, procrustes=procrustes, thr=t, counts=counts)
    out = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    if counts is not None:
        out["counts"] = counts.cpu().numpy()
    return out


def _assert_ulp(got, ref, name, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    rel = np.max(err / np.where(ref == 0, 1.0, np.abs(ref)))
    print(f"   {what}: {rel / ULP[name]:.2f} ulp")
    assert np.all(err <= 4 * ULP[name] * np.abs(ref)), what          # ref == 0 demands got == 0


def _aligned_bar(g, meta, b, name):
    """How far an aligned distance (or its mean / an order statistic) may lie from the float64 run."""
    if name == "f32":
        return meta["cases"][str(b)]["e_ref32"]["aligned"] * np.sqrt(3) + 2.0 ** -24 * float(g[f"f64/{b}/dist_aligned"].max())
    *_, normX, _ = eval_ref.procrustes_transform(g[f"in/{b}/gt"], g[f"in/{b}/pred"])
    return f64_bar(meta) * float(normX.max()) * np.sqrt(3)


# ------------------------------------------------------------------ 1. the kernel against the reference's recorded outputs
@pytest.mark.parametrize("name", ["f32", "f64"])
@pytest.mark.parametrize("b", CASES)
def test_kernel_matches_the_reference(g12, b, name):
    import peclr_amd
    from peclr_amd import pose_eval

    g, meta = g12
    assert fixture_gap(g) >= 1e-5                                   # the condition under which counts compare exactly
    gt, pred, thr = g[f"in/{b}/gt"], g[f"in/{b}/pred"], g["thresholds"]
    o = _launch(pred, gt, name, thr)
    p, case = f"{name}/{b}/", meta["cases"][str(b)]
    assert not o["status"].any()

    if name == "f64":
        e = procrustes_errors(g, b, o["aligned"], o["rot"], o["scale"], o["trans"])
        print(f"B={b} float64 against the reference: {e} (bar {f64_bar(meta):.2e})")
        assert max(e.values()) <= f64_bar(meta), e
    else:
        for key in ("aligned", "rot", "scale"):
            err = float(np.abs(o[key].astype(np.float64).reshape(-1) - g[f"f64/{b}/{key}"].reshape(-1)).max())
            print(f"B={b} float32 {key}: {err:.3e} from the float64 run (e_ref32 {case['e_ref32'][key]:.3e})")
            assert err <= case["e_ref32"][key], key

    _assert_ulp(o["dist"], g[p + "dist"], name, "raw distances")
    err = float(np.abs(o["dist_aligned"].astype(np.float64) - g[f"f64/{b}/dist_aligned"]).max())
    print(f"   aligned distances: {err:.3e} from the float64 run (bar {_aligned_bar(g, meta, b, name):.3e})")
    assert err <= _aligned_bar(g, meta, b, name)

    for s, ckey, akey in ((0, "pck", "auc"), (1, "pck_aligned", "auc_aligned")):
        want = np.rint(g[p + ckey].astype(np.float64) * b).astype(np.int64)
        assert np.array_equal(o["counts"][s], want), ckey
        auc = pose_eval.auc_from_counts(o["counts"][s], b, thr)
        assert np.abs(auc - g[p + akey]).max() <= 1e-7, akey
    dist_dev = _dev(o["dist"], name)
    curve, thr_out = peclr_amd.pck_curves(dist_dev, per_joint=True)
    assert np.array_equal(curve, g[p + "pck"]) and np.array_equal(thr_out, thr) and curve.dtype == np.float32
    overall, _ = peclr_amd.pck_curves(dist_dev)
    assert overall.dtype == np.float32 and np.array_equal(overall, g[p + "pck_overall"])      # get_pck_curves(per_joint=False)
    assert np.abs(peclr_amd.auc_joints(dist_dev) - g[p + "auc"]).max() <= 1e-7

    st = peclr_amd.epe_statistics(_dev(pred, name), _dev(gt, name), 3)
    assert st["eucledian_dist"].dtype == DTYPES[name] and np.array_equal(st["eucledian_dist"].cpu().numpy(), o["dist"])
    ref = case[name]["raw"]
    assert abs(float(st["mean"]) - ref["mean"]) <= 1e-6 * ref["mean"]
    for k in ("median", "min", "max"):
        _assert_ulp(float(st[k]), ref[k], name, k)

    yt, rot, scale, trans = peclr_amd.procrustes_transform(_dev(gt, name), _dev(pred, name))
    assert scale.shape == (b, 1, 1) and trans.shape == (b, 1, 3) and rot.shape == (b, 3, 3)
    for got, key in ((yt, "aligned"), (rot, "rot"), (scale, "scale"), (trans, "trans")):
        assert np.array_equal(got.cpu().numpy().reshape(-1), o[key].reshape(-1)), key

    ev = peclr_amd.PoseEvaluator(b, dtype=DTYPES[name], device=DEV)
    ev.update(_dev(pred, name), _dev(gt, name))
    m = ev.compute()
    assert list(m)[:6] == list(REF_KEYS) and set(m) == set(REF_KEYS) | {"pck", "pck_procrustes", "thresholds"}
    assert abs(float(m["Mean_EPE_3D"]) - ref["mean"]) <= 1e-6 * ref["mean"]
    _assert_ulp(float(m["Median_EPE_3D"]), ref["median"], name, "Median_EPE_3D")
    assert abs(m["AUC"] - np.mean(g[p + "auc"])) <= 1e-7 and abs(m["auc_procrustes"] - np.mean(g[p + "auc_aligned"])) <= 1e-7
    al = case[name]["aligned"]                                  # the issue's mean bar, against the run of the same dtype
    rel = abs(float(m["Mean_EPE_3D_procrustes"]) - al["mean"]) / al["mean"]
    print(f"   Mean_EPE_3D_procrustes: {rel:.2e} relative to the reference's {name} mean (bar 1e-6)")
    assert rel <= 1e-6
    al64, bar = meta["cases"][str(b)]["f64"]["aligned"], _aligned_bar(g, meta, b, name)
    assert abs(float(m["Median_EPE_3D_procrustes"]) - al64["median"]) <= bar
    assert np.array_equal(m["pck"], g[p + "pck"]) and np.array_equal(m["pck_procrustes"], g[p + "pck_aligned"])
    assert type(m["Mean_EPE_3D"]) is (np.float32 if name == "f32" else np.float64)


# ------------------------------------------------------------------ 2. the special rows, by name
@pytest.mark.parametrize("name", ["f32", "f64"])
def test_special_rows(g12, name):
    g, meta = g12
    rows = meta["special_rows"]
    gt, pred = g["in/7/gt"], g["in/7/pred"]
    o = _launch(pred, gt, name, g["thresholds"])
    tol = f64_bar(meta) if name == "f64" else None
    e32 = meta["cases"]["7"]["e_ref32"]
    det = np.linalg.det(o["rot"].astype(np.float64))
    ref_scale, ref_rot = g["f64/7/scale"].reshape(-1), g["f64/7/rot"]
    *_, normX, normY = eval_ref.procrustes_transform(gt, pred)

    def scale_ok(i):
        err = abs(float(o["scale"][i]) - ref_scale[i])
        return err <= (tol * normX[i] / normY[i] if tol else e32["scale"])

    def rot_ok(i):
        return np.abs(o["rot"][i].astype(np.float64) - ref_rot[i]).max() <= (tol or e32["rot"])

    i = rows["mirrored"]                     # det(V U^T) < 0 before the fix: a proper rotation comes out, the scale is the reference's
    assert abs(det[i] - 1.0) <= (1e-12 if name == "f64" else 1e-6) and scale_ok(i) and rot_ok(i)
    A = eval_ref.procrustes_transform(gt[i:i + 1], pred[i:i + 1])        # (the fixture row really takes the branch)
    Xc, Yc = gt[i] - gt[i].mean(0), pred[i] - pred[i].mean(0)
    U, _, Vt = np.linalg.svd(Xc.T @ Yc)
    assert np.linalg.det(Vt.T @ U.T) < 0 and np.linalg.det(A[1][0]) > 0

    i = rows["identity"]
    assert np.all(o["dist"][i] == 0)
    assert np.abs(o["rot"][i] - np.eye(3)).max() <= (tol or e32["rot"]) and scale_ok(i) and abs(float(o["scale"][i]) - 1) <= 1e-6
    assert o["dist_aligned"][i].max() <= (1e-15 if name == "f64" else 1e-7)
    assert not o["counts"][:, :, 0].any()    # nothing is strictly under threshold 0.0, the exact zeros included
    assert (o["counts"][0][:, 1] >= 1).all()  # ... and they are under the next one

    i = rows["planar"]                       # third singular value 0: the rotation is still unique once det = +1 is asked for
    assert abs(det[i] - 1.0) <= (1e-12 if name == "f64" else 1e-6) and rot_ok(i) and scale_ok(i)

    i = rows["scaled"]                       # millimetres against metres, far away
    assert 5e-4 < float(o["scale"][i]) < 2e-3 and scale_ok(i) and rot_ok(i)
    err = np.abs(o["aligned"][i].astype(np.float64) - g["f64/7/aligned"][i]).max()
    assert err <= (tol * normX[i] if tol else e32["aligned"])
    assert abs(det - 1.0).max() <= (1e-12 if name == "f64" else 1e-6)


# ------------------------------------------------------------------ 3. NaN and degenerate rows
def _with_bad_rows(g):
    """The batch of 7 with the NaN row at position 3 and the all-zero prediction at position 8 -> clouds and the kept rows."""
    gt, pred = g["in/7/gt"], g["in/7/pred"]
    gt9 = np.concatenate([gt[:3], g["in/nan_row/gt"], gt[3:], g["in/zero_row/gt"]])
    pred9 = np.concatenate([pred[:3], g["in/nan_row/pred"], pred[3:], g["in/zero_row/pred"]])
    return gt9, pred9, [0, 1, 2, 4, 5, 6, 7]


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_nan_and_degenerate_rows_touch_nothing_else(g12, name):
    import peclr_amd
    from peclr_amd import _capi

    g, _ = g12
    gt9, pred9, keep = _with_bad_rows(g)
    bad = _launch(pred9, gt9, name)
    clean = _launch(g["in/7/pred"], g["in/7/gt"], name)
    assert bad["status"][3] & _capi.POSE_STATUS_NAN and bad["status"][8] == _capi.POSE_EVAL_DEGENERATE
    assert not bad["status"][keep].any()
    for key in ("dist", "dist_aligned", "aligned", "rot", "scale", "trans"):
        assert np.array_equal(bad[key][keep], clean[key]), key                  # bit for bit
        assert np.isfinite(bad[key][keep]).all(), key
    for key in ("dist_aligned", "aligned", "rot", "scale", "trans"):             # the reference's 0 / 0
        assert np.isnan(bad[key][[3, 8]]).all(), key
    assert np.isnan(bad["dist"][3, 7]) and np.isfinite(np.delete(bad["dist"][3], 7)).all()
    assert np.isfinite(bad["dist"][8]).all()                                    # |gt| itself: the raw distance to an all-zero prediction

    # NaN distances are under no threshold: the nine rows count what the seven clean rows count, plus -- raw set only -- the 20
    # finite joints of the NaN row and the 21 of the all-zero prediction (their aligned distances are all NaN)
    thr = g["thresholds"]
    c9 = _launch(pred9, gt9, name, thr)["counts"]
    c7 = _launch(g["in/7/pred"], g["in/7/gt"], name, thr)["counts"]
    assert np.array_equal(c9[1], c7[1])
    extra = eval_ref.pck_counts(bad["dist"][[3, 8]], thr)                      # NumPy: NaN < t is False
    assert extra[7].max() <= 1 and extra[:, -1].sum() <= 20 + 21 and extra.sum() > 0      # joint 7 of the NaN row never counts
    assert np.array_equal(c9[0], c7[0] + extra)

    ev = peclr_amd.PoseEvaluator(16, dtype=DTYPES[name], device=DEV)
    ev.update(_dev(pred9, name), _dev(gt9, name))
    with pytest.raises(FloatingPointError, match=r"sample\(s\) \[3, 8\]"):
        ev.compute()
    m = ev.compute(allow_nan=True)
    assert np.isnan(m["Mean_EPE_3D"]) and np.isnan(m["Median_EPE_3D_procrustes"]) and np.isfinite(m["AUC"])
    # the all-zero early exit of the reference lives in procrustes_transform alone
    y = _dev(np.zeros((2, 21, 3)), name)
    assert peclr_amd.procrustes_transform(_dev(gt9[:2], name), y)[1:] == (None, None, None)


# ------------------------------------------------------------------ 4. a pure function of the sample
@pytest.mark.parametrize("name", ["f32", "f64"])
def test_sample_outputs_do_not_depend_on_the_batch(g12, name):
    g, meta = g12
    keys = ("dist", "dist_aligned", "aligned", "rot", "scale", "trans")
    for row in (meta["special_rows"]["noisy"], meta["special_rows"]["mirrored"]):
        gt1, pred1 = g["in/7/gt"][row:row + 1], g["in/7/pred"][row:row + 1]
        alone = _launch(pred1, gt1, name)
        in7 = _launch(g["in/7/pred"], g["in/7/gt"], name)
        gt130, pred130 = g["in/130/gt"].copy(), g["in/130/pred"].copy()
        for pos in (0, 64, 129):
            gt130[pos], pred130[pos] = gt1[0], pred1[0]
        in130 = _launch(pred130, gt130, name, g["thresholds"])
        again = _launch(pred130, gt130, name, g["thresholds"])
        for key in keys:
            assert np.array_equal(alone[key][0], in7[key][row]), key
            for pos in (0, 64, 129):
                assert np.array_equal(alone[key][0], in130[key][pos]), (key, pos)
            assert np.array_equal(in130[key], again[key]), key                 # run to run
        assert np.array_equal(in130["counts"], again["counts"])


# ------------------------------------------------------------------ 5. streaming
def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_streaming_equals_one_update(g12, name):
    import peclr_amd

    g, _ = g12
    gt, pred = _dev(g["in/130/gt"], name), _dev(g["in/130/pred"], name)
    one = peclr_amd.PoseEvaluator(130, dtype=DTYPES[name], device=DEV)
    one.update(pred, gt)
    whole = one.compute()
    ev = peclr_amd.PoseEvaluator(130, dtype=DTYPES[name], device=DEV)
    for _ in range(2):
        for lo, hi in ((0, 5), (5, 6), (6, 130)):
            ev.update(pred[lo:hi], gt[lo:hi])
        _same(ev.compute(), whole)
        with pytest.raises(ValueError, match="capacity"):
            ev.update(pred[:1], gt[:1])
        with pytest.raises(Exception, match="no CPU path"):
            ev.update(pred[:1].cpu(), gt[:1].cpu())
        assert ev._asked == [130, 0]                                           # a call that raised asked for nothing
        _same(ev.compute(), whole)                                             # the refused batch left nothing behind
        ev.reset()


# ------------------------------------------------------------------ 6. no host synchronisation; a hipGraph replays it
def test_update_has_no_host_sync_and_the_graph_appends_on_replay(g12):
    import peclr_amd

    g, _ = g12
    gt, pred = _dev(g["in/130/gt"], "f64"), _dev(g["in/130/pred"], "f64")
    b = 8
    eager = peclr_amd.PoseEvaluator(64, device=DEV)
    eager.update(pred[:b], gt[:b])                                             # (first launch: loads the code object)
    eager.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager.update(pred[:b], gt[:b])
        eager.update(pred[b:2 * b], gt[b:2 * b])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    want = eager.compute()

    ev = peclr_amd.PoseEvaluator(64, device=DEV)
    sp, sg = torch.zeros_like(pred[:b]), torch.zeros_like(gt[:b])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.update(sp, sg)
    for lo in (0, b):
        sp.copy_(pred[lo:lo + b])
        sg.copy_(gt[lo:lo + b])
        graph.replay()
    _same(ev.compute(), want)                                                  # rows 0..7 and 8..15: the device cursor moved
    for x, y in zip(ev.distances(2 * b), eager.distances(2 * b)):
        assert torch.equal(x, y)
    # replays past the capacity write nothing, and compute() says so
    small = peclr_amd.PoseEvaluator(b, device=DEV)
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        small.update(sp, sg)
    g2.replay()
    g2.replay()
    with pytest.raises(RuntimeError, match="capacity is 8"):
        small.compute()


# ------------------------------------------------------------------ 7. dim = 2
@pytest.mark.parametrize("name", ["f32", "f64"])
def test_two_dimensional_statistics(g12, name):
    import peclr_amd

    g, meta = g12
    for b in CASES:
        gt, pred = g[f"in/{b}/gt"], g[f"in/{b}/pred"]
        ref = meta["cases"][str(b)][name]["raw_2d"]
        st = peclr_amd.epe_statistics(_dev(pred, name), _dev(gt, name), 2)
        _assert_ulp(st["eucledian_dist"].cpu().numpy(), g[f"{name}/{b}/dist_2d"], name, f"B={b} 2D distances")
        assert abs(float(st["mean"]) - ref["mean"]) <= 1e-6 * ref["mean"]
        for k in ("median", "min", "max"):
            _assert_ulp(float(st[k]), ref[k], name, k)
        ev = peclr_amd.PoseEvaluator(b, dtype=DTYPES[name], device=DEV)
        ev.update(_dev(pred, name), _dev(gt, name))
        ev.update_2d(_dev(pred[:, :, :2], name), _dev(gt[:, :, :2], name))
        m = ev.compute()
        assert abs(float(m["Mean_EPE_2D"]) - ref["mean"]) <= 1e-6 * ref["mean"]
        _assert_ulp(float(m["Median_EPE_2D"]), ref["median"], name, "Median_EPE_2D")


# ------------------------------------------------------------------ 8. the tool
def test_pred_freihand_tool_scores_a_training_split(tmp_path, monkeypatch, capsys):
    """tools/pred_freihand.py on a three-image fake split, in this process: --split training --eval writes the reference's keys
    with the values of a PoseEvaluator fed the same predictions; the default invocation writes the submission it always wrote."""
    from PIL import Image

    import peclr_amd
    from peclr_amd import pose
    from tests.test_pose_gpu import _images, _k_and_scale, _prediction_model

    spec = importlib.util.spec_from_file_location("pred_freihand_tool", os.path.join(ROOT, "tools", "pred_freihand.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)

    data = tmp_path / "fh"
    imgs = _images(3, seed=4)
    K, scale = _k_and_scale(3, seed=4)
    rng = np.random.default_rng(4)
    xyz_gt = rng.standard_normal((3, 21, 3)) * 0.04 + [0.0, 0.0, 0.6]
    for split in ("evaluation", "training"):
        (data / split / "rgb").mkdir(parents=True)
        for i in range(3):
            Image.fromarray(imgs[i]).save(str(data / split / "rgb" / f"{i:08d}.jpg"), quality=95)
        (data / f"{split}_K.json").write_text(json.dumps(K.tolist()))
        (data / f"{split}_scale.json").write_text(json.dumps(scale.tolist()))
    Image.fromarray(imgs[0]).save(str(data / "training" / "rgb" / f"{3:08d}.jpg"))     # more images than K entries: ignored
    (data / "training_xyz.json").write_text(json.dumps(xyz_gt.tolist()))
    ckpt = tmp_path / "rn50_peclr_yt3d-fh_pt_fh_ft.pth"
    torch.save({"state_dict": _prediction_model().state_dict()}, ckpt)

    seen = []
    predict = pose.FreiHANDPredictor.predict

    def recording(self, *a):
        out = predict(self, *a)
        seen.append(out.clone())
        return out

    monkeypatch.setattr(pose.FreiHANDPredictor, "predict", recording)
    monkeypatch.chdir(tmp_path)
    base = ["--model_path", str(ckpt), "--data", str(data), "--batch", "2"]
    tool.main(base + ["--split", "training", "--eval"])
    printed = capsys.readouterr().out
    with open(tmp_path / "out" / "eval_rn50.json") as f:
        written = json.load(f)
    assert list(written)[:6] == list(REF_KEYS) and all(k + ":" in printed for k in REF_KEYS)
    assert not (tmp_path / "out" / "pred_rn50.json").exists()
    assert [len(s) for s in seen] == [2, 1]
    ev = peclr_amd.PoseEvaluator(3, device=DEV)
    for s, lo in zip(seen, (0, 2)):
        ev.update(s, torch.from_numpy(xyz_gt[lo:lo + len(s)]).to(DEV))
    want = ev.compute()
    for k, v in want.items():
        assert np.array_equal(np.asarray(written[k]), np.asarray(v, dtype=np.float64)), k

    seen.clear()
    tool.main(base)
    assert "Dumped 3 joints and 3 verts predictions to" in capsys.readouterr().out
    got = (tmp_path / "out" / "pred_rn50.json").read_bytes()
    pose.write_freihand_submission(str(tmp_path / "expect" / "pred_rn50"), torch.cat(seen))
    assert got == (tmp_path / "expect" / "pred_rn50.json").read_bytes() and (tmp_path / "out" / "pred_rn50.zip").exists()
