"""Scoring pose predictions, the part that needs no GPU: the float64 NumPy restatement (tests/eval_ref.py) and the kernel's
numeric core compiled as host C++ (peclr_amd/csrc/procrustes.hpp through tests/eval_host_main.cpp) against the recorded
outputs of the reference (tests/golden/g12_pose_eval.*), argument errors of the entry point, the host-side AUC and the tool's
argument handling.

Measured here (tests/golden/make_golden_eval.py records them in the fixture's json):
  e_np64  = 4.272e-13  largest float64 difference of the NumPy restatement from the reference's float64 run (y_transform and
                       translation relative to normX, rot_mat absolute, scale over normX / normY); it is the x1000 row's
                       translation (|muY| = 6e5 against normX = 0.24), every other figure is below 1.5e-14
  gap_min = 1.980e-05  smallest relative distance of a reference distance to a non-zero threshold (bar 1e-5)
  e_ref32 (aligned, rot, scale): B = 1: 3.13e-08, 1.83e-07, 2.75e-08; B = 7: 2.34e-05, 3.33e-07, 1.19e-07;
                                 B = 130: 1.35e-07, 1.16e-06, 2.01e-07
  host C++ core against the float64 run: at most 8.6e-13 in the same units (the same row), else below 1.5e-14
"""
import importlib.util
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import eval_ref
from tests.conftest import GOLDEN, ROOT, load_golden

CASES = (1, 7, 130)
F64_FLOOR = 1e-13


@pytest.fixture(scope="module")
def g12():
    with open(os.path.join(GOLDEN, "g12_pose_eval.json")) as f:
        meta = json.load(f)
    return load_golden("g12_pose_eval.npz"), meta


def f64_bar(meta):
    return max(8 * meta["e_np64"], F64_FLOOR)


def procrustes_errors(g, b, aligned, rot, scale, trans):
    """The four float64 figures of the bars: aligned and trans relative to normX, rot absolute, scale over normX / normY."""
    gt, pred = g[f"in/{b}/gt"], g[f"in/{b}/pred"]
    *_, normX, normY = eval_ref.procrustes_transform(gt, pred)
    nx = normX.reshape(-1, 1, 1)
    p = f"f64/{b}/"
    return {"aligned": float((np.abs(aligned - g[p + "aligned"]) / nx).max()),
            "trans": float((np.abs(trans.reshape(-1, 1, 3) - g[p + "trans"]) / nx).max()),
            "rot": float(np.abs(rot - g[p + "rot"]).max()),
            "scale": float((np.abs(scale.reshape(-1) - g[p + "scale"].reshape(-1)) / (normX / normY)).max())}


def fixture_gap(g):
    """Smallest relative distance of any recorded distance (raw, aligned; float32, float64) to any non-zero threshold."""
    gap = np.inf
    for name, dt in (("f32", np.float32), ("f64", np.float64)):
        th = g["thresholds"].astype(dt).astype(np.float64)[1:]
        for b in CASES:
            for key in ("dist", "dist_aligned"):
                d = g[f"{name}/{b}/{key}"].astype(np.float64).reshape(-1, 1)
                gap = min(gap, float((np.abs(d - th[None]) / th[None]).min()))
    return gap


def test_fixture_keeps_distances_clear_of_the_thresholds(g12):
    g, meta = g12
    gap = fixture_gap(g)
    print(f"gap_min {gap:.3e} (recorded {meta['gap_min']:.3e})")
    assert gap >= 1e-5 and gap == pytest.approx(meta["gap_min"], rel=1e-12)


def test_numpy_restatement_matches_the_reference(g12):
    g, meta = g12
    worst = 0.0
    for b in CASES:
        gt, pred = g[f"in/{b}/gt"], g[f"in/{b}/pred"]
        yt, rot, scale, trans, _, _ = eval_ref.procrustes_transform(gt, pred)
        e = procrustes_errors(g, b, yt, rot, scale, trans)
        print(f"B={b}: e_np64 {e}")
        worst = max(worst, *e.values())
        p = f"f64/{b}/"
        for key, dim, ref in (("raw", 3, "dist"), ("raw_2d", 2, "dist_2d")):
            st = eval_ref.epe_statistics(pred, gt, dim)
            np.testing.assert_allclose(st["eucledian_dist"], g[p + ref], rtol=4 * 2.0 ** -52, atol=0)
            for k in ("mean", "median", "min", "max"):
                assert st[k] == pytest.approx(meta["cases"][str(b)]["f64"][key][k], rel=1e-14, abs=1e-18), (b, key, k)
        for name, dt in (("f32", np.float32), ("f64", np.float64)):
            for dkey, ckey, akey in (("dist", "pck", "auc"), ("dist_aligned", "pck_aligned", "auc_aligned")):
                curve = eval_ref.pck_curve(g[f"{name}/{b}/{dkey}"], g["thresholds"])
                assert curve.dtype == np.float32 and np.array_equal(curve, g[f"{name}/{b}/{ckey}"])
                np.testing.assert_array_equal(eval_ref.auc_from_curve(curve, g["thresholds"]), g[f"{name}/{b}/{akey}"])
    print(f"e_np64 = {worst:.3e} (recorded {meta['e_np64']:.3e})")
    # The recorded figure depends on the LAPACK behind np.linalg.svd to the last bits: only its order of magnitude is held
    # here.  The bound is the check: two float64 SVDs of the same matrices; the x1000 row's translation sets the figure.
    assert meta["e_np64"] / 10 <= worst <= meta["e_np64"] * 10
    assert worst < 1e-11


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_host_build_of_the_kernel_core_matches_the_reference(g12, tmp_path):
    """procrustes.hpp as plain C++: the arithmetic the kernel runs, on the CPU, against the reference's float64 run at the
    float64 bar of the GPU test, and its float32 rounding against the reference's own float32 error."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, g++, c++, clang++) on PATH")
    g, meta = g12
    exe = tmp_path / "eval_host_main"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), os.path.join(ROOT, "tests", "eval_host_main.cpp")],
                   check=True)
    bar = f64_bar(meta)
    for b in CASES:
        gt, pred = g[f"in/{b}/gt"], g[f"in/{b}/pred"]
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.int32(b).tobytes() + np.ascontiguousarray(gt).tobytes() + np.ascontiguousarray(pred).tobytes())
        subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
        o = np.fromfile(tmp_path / "out.bin").reshape(b, 97)
        rot, scale, trans, aligned, dist_al = o[:, :9].reshape(b, 3, 3), o[:, 9], o[:, 10:13], o[:, 13:76].reshape(b, 21, 3), o[:, 76:]
        e = procrustes_errors(g, b, aligned, rot, scale, trans)
        print(f"B={b}: host core against the float64 run {e} (bar {bar:.2e})")
        assert max(e.values()) <= bar, (b, e)
        np.testing.assert_allclose(np.linalg.det(rot), 1.0, atol=1e-14)
        np.testing.assert_allclose(dist_al, g[f"f64/{b}/dist_aligned"], rtol=0, atol=bar * np.abs(gt).max())
        # rounded once to float32 (the inputs are float32-exact): no further from the float64 run than the reference's float32 run
        e32 = meta["cases"][str(b)]["e_ref32"]
        for key, val in (("aligned", aligned), ("rot", rot), ("scale", scale)):
            err = np.abs(val.astype(np.float32).astype(np.float64).reshape(-1) - g[f"f64/{b}/{key}"].reshape(-1)).max()
            print(f"   float32 {key}: {err:.3e} (e_ref32 {e32[key]:.3e})")
            assert err <= e32[key], (b, key)


def test_entry_point_rejects_bad_arguments_before_launch():
    """Every case returns -1 without a launch (no GPU here): fake non-null pointers are never dereferenced."""
    from peclr_amd import _capi

    L = _capi.lib()
    P = 0x1000                     # any non-null value: the checks come before the launch
    F32, F64 = 0, 3

    def call(pred=P, gt=P, B=4, dtype=F64, dim=3, dist=P, aligned=None, rot=None, scale=None, trans=None, dist_al=None, thr=None,
             T=0, counts=None, status=P, cursor=None, cap=0):
        return L.peclr_pose_eval(pred, gt, B, dtype, dim, dist, aligned, rot, scale, trans, dist_al, thr, T, counts, status, cursor,
                                 cap, None)

    assert call(B=0) == -1 and call(B=-3) == -1
    assert call(pred=None) == -1 and call(gt=None) == -1
    assert call(dtype=1) == -1 and call(dtype=7) == -1 and call(dtype=-1) == -1
    assert call(dim=1) == -1 and call(dim=4) == -1 and call(dim=0) == -1
    for out in ("aligned", "rot", "scale", "trans", "dist_al"):
        assert call(dim=2, dtype=F32, **{out: P}) == -1, out
    assert call(T=-1) == -1
    assert call(T=5, thr=None, counts=P) == -1 and call(T=5, thr=P, counts=None) == -1
    assert call(dist=None) == -1 and call(status=None) == -1
    assert call(cursor=P, cap=3) == -1 and call(cursor=P, cap=0) == -1          # the batch must fit the streamed buffers


def test_cpu_tensors_have_no_path():
    import peclr_amd
    from peclr_amd import _capi

    a, b = torch.zeros(2, 21, 3), torch.ones(2, 21, 3)
    for fn in (lambda: peclr_amd.epe_statistics(a, b, 3), lambda: peclr_amd.procrustes_transform(a, b),
               lambda: peclr_amd.pck_curves(torch.zeros(2, 21)), lambda: peclr_amd.auc_joints(torch.zeros(2, 21)),
               lambda: peclr_amd.PoseEvaluator(4, device="cpu"), lambda: _capi.pose_eval(a, b)):
        with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
            fn()


def test_auc_from_integer_counts_reproduces_the_reference(g12):
    from peclr_amd import pose_eval

    g, meta = g12
    for b in CASES:
        for name in ("f32", "f64"):
            for dkey, ckey, akey in (("dist", "pck", "auc"), ("dist_aligned", "pck_aligned", "auc_aligned")):
                counts = eval_ref.pck_counts(g[f"{name}/{b}/{dkey}"], g["thresholds"])
                assert np.array_equal(counts, np.rint(g[f"{name}/{b}/{ckey}"].astype(np.float64) * b).astype(np.int64))
                assert np.array_equal(pose_eval.curve_from_counts(counts, b), g[f"{name}/{b}/{ckey}"])
                if dkey == "dist":
                    assert np.array_equal(pose_eval.curve_from_counts(counts, b, per_joint=False), g[f"{name}/{b}/pck_overall"])
                auc = pose_eval.auc_from_counts(counts, b, g["thresholds"])
                np.testing.assert_array_equal(auc, g[f"{name}/{b}/{akey}"])
                assert pose_eval.auc_from_counts(counts, b, g["thresholds"], per_joint=False) == np.mean(g[f"{name}/{b}/{akey}"])


def _tool():
    spec = importlib.util.spec_from_file_location("pred_freihand_tool", os.path.join(ROOT, "tools", "pred_freihand.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_arguments(tmp_path):
    tool = _tool()
    args = tool.parse_args(["--model_path", "rn50_x.pth", "--data", "/d"])
    assert vars(args) == {"model_path": "rn50_x.pth", "data": "/d", "batch": 128, "split": "evaluation", "eval": False}
    args = tool.parse_args(["--model_path", "m", "--data", "/d", "--batch", "7", "--split", "training", "--eval"])
    assert (args.batch, args.split, args.eval) == (7, "training", True)
    with pytest.raises(SystemExit):
        tool.parse_args(["--model_path", "m", "--data", "/d", "--split", "validation"])
    for split in ("evaluation", "training"):                  # no labels in the directory: a clear message, before any model work
        with pytest.raises(SystemExit) as exc:
            tool.main(["--model_path", "rn50_x.pth", "--data", str(tmp_path), "--split", split, "--eval"])
        assert f"{split}_xyz.json" in str(exc.value) and "--eval needs ground-truth joints" in str(exc.value)
