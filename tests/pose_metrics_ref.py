"""Float64 NumPy restatement of the metrics a supervised step logs (peclr_amd/pose_metrics.py, csrc/pose_metrics.hip), written
out from calculate_metrics' formula, and the INPUTS of the fixture tests/golden/g16_step_metrics.json.

The fixture holds results only (a few KB): its inputs, up to 1024 x 21 x 3 numbers a pair, are drawn here from the seed and
the kind the fixture names, by NumPy's `default_rng` -- the generator script tests/golden/make_golden_metrics.py imports this
module and feeds the reference exactly these float32 arrays.  The repository's own text; tests/test_pose_metrics_host.py holds
`metrics64` to the reference's float64 results at 1e-12.
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_step_metrics.json")
J = 21
# name -> the pairs of the case, each (kind, B, seed); a case with two pairs goes through the launch's two-pair form
CASES = {
    "b1": [("metres", 1, 1601)],                      # n = 21: odd, less than one wave
    "b2": [("metres", 2, 1602)],                      # n = 42: even, the lower median is sorted element 20
    "b3": [("metres", 3, 1603)],
    "b65": [("pixels", 65, 1665)],                    # n = 1365: not a multiple of 64
    "b128": [("pixels", 128, 1628), ("metres", 128, 1629)],
    "b1024": [("pixels", 1024, 1624), ("metres", 1024, 1625)],
    "all_equal": [("all_equal", 5, 1605)],
    "duplicates": [("duplicates", 4, 1604)],          # n = 84, rank 41 lies inside a run of equal distances
    "identical": [("identical", 3, 1633)],            # pred == truth
    "nan": [("nan", 3, 1643), ("metres", 3, 1644)],   # one NaN coordinate in the first pair, the second is untouched
    "nan_second": [("pixels", 3, 1645), ("nan", 3, 1646)],
    "inf": [("inf", 3, 1653)],                        # one inf coordinate: mean inf, median finite
    "scales": [("pixels", 8, 1608), ("metres", 8, 1609)],   # 2-D scale (~100) next to metre scale (~0.01)
    "wide": [("wide", 16, 1616)],                     # distances over more than 2^24 in ratio: every radix pass decides
}
EXACT_MEDIAN = ("all_equal", "duplicates", "identical")


def make_pair(kind, b, seed):
    """(pred, truth) [b,21,3] float32 of one pair of a case."""
    g = np.random.default_rng(seed)
    if kind in ("pixels", "nan", "inf"):
        truth = g.uniform(20.0, 200.0, (b, J, 3))
        pred = truth + g.standard_normal((b, J, 3)) * 8.0
        if kind != "pixels":
            at = (int(g.integers(b)), int(g.integers(J)), int(g.integers(3)))
            pred[at] = np.nan if kind == "nan" else np.inf
    elif kind == "metres":
        truth = g.standard_normal((b, J, 3)) * 0.05 + np.array([0.0, 0.0, 0.6])
        pred = truth + g.standard_normal((b, J, 3)) * 0.01
    elif kind == "wide":
        truth = g.uniform(-1.0, 1.0, (b, J, 3))
        pred = truth + g.standard_normal((b, J, 3)) * 10.0 ** g.uniform(-5.0, 4.0, (b, J, 1))
    elif kind == "identical":
        truth = g.standard_normal((b, J, 3))
        pred = truth.copy()
    else:  # small integers: every difference and every distance is exact in float32
        truth = g.integers(-50, 50, (b, J, 3)).astype(np.float64)
        if kind == "all_equal":
            offset = np.broadcast_to(np.array([3.0, 4.0, 0.0]), (b, J, 3))
        else:
            assert kind == "duplicates" and b * J == 84
            length = g.permutation(np.repeat([5.0, 10.0, 15.0], [30, 24, 30])).reshape(b, J, 1)   # rank 41: inside the 10s
            offset = length / 5.0 * np.array([3.0, 0.0, 4.0])
        pred = truth + offset
    return pred.astype(np.float32), truth.astype(np.float32)


def case_pairs(name):
    """The float32 inputs of a fixture case: a list of (pred, truth), one or two pairs."""
    return [make_pair(*spec) for spec in CASES[name]]


def load_fixture():
    with open(GOLDEN) as f:
        return json.load(f)


def distances64(pred, truth):
    """[B,21] float64 Euclidean distances of two [B,21,3] arrays."""
    d = np.asarray(pred, np.float64) - np.asarray(truth, np.float64)
    return np.sqrt((d * d).sum(axis=2))


def metrics64(pred, truth):
    """(mean, lower median) of the distances in float64; a NaN distance makes both NaN (torch.mean, torch.median)."""
    flat = distances64(pred, truth).reshape(-1)
    if np.isnan(flat).any():
        return float("nan"), float("nan")
    return float(flat.sum() / flat.size), float(np.sort(flat)[(flat.size - 1) // 2])


def ulp32(x):
    """The spacing of float32 at |x| (the float32 nearest to it)."""
    return float(np.spacing(np.abs(np.float32(x))))
