"""Host side of the step metrics (peclr_amd/pose_metrics.py): the float64 restatement the GPU tests use is held to the
reference's own float64 results (tests/golden/g16_step_metrics.json) at 1e-12, the bound the other restatements are held to;
the wrapper refuses what it cannot run before any device call; the key names are the reference's."""
import math

import numpy as np
import pytest
import torch

from tests import pose_metrics_ref as ref

FIX = ref.load_fixture()


def gold(value):
    return float(value)          # ("nan" / "inf" are written as strings)


def test_the_fixture_names_the_cases_the_restatement_draws():
    assert [c["name"] for c in FIX["cases"]] == list(ref.CASES)
    for c in FIX["cases"]:
        assert [(p["kind"], p["B"], p["seed"]) for p in c["pairs"]] == list(ref.CASES[c["name"]])
    sizes = {p["B"] for c in FIX["cases"] for p in c["pairs"]}
    assert {1, 2, 3, 65, 128, 1024} <= sizes


@pytest.mark.parametrize("case", FIX["cases"], ids=lambda c: c["name"])
def test_restatement_against_the_reference_in_float64(case):
    for entry, (pred, truth) in zip(case["pairs"], ref.case_pairs(case["name"])):
        assert pred.dtype == np.float32 and pred.shape == (entry["B"], 21, 3)
        for got, key in zip(ref.metrics64(pred, truth), ("mean", "median")):
            want = gold(entry["gold64"][key])
            if math.isfinite(want):
                assert abs(got - want) <= 1e-12 * max(abs(want), 1e-300), (case["name"], entry["kind"], key, got, want)
            else:
                assert (math.isnan(got) and math.isnan(want)) or got == want, (case["name"], entry["kind"], key, got, want)


def test_fixture_semantics():
    by = {c["name"]: c["pairs"] for c in FIX["cases"]}
    assert all(math.isnan(gold(by["nan"][0][g][k])) for g in ("gold32", "gold64") for k in ("mean", "median"))
    assert math.isinf(gold(by["inf"][0]["gold64"]["mean"])) and math.isfinite(gold(by["inf"][0]["gold64"]["median"]))
    assert by["identical"][0]["gold32"] == {"mean": 0.0, "median": 0.0}
    assert by["all_equal"][0]["gold32"] == {"mean": 5.0, "median": 5.0} and by["duplicates"][0]["gold32"]["median"] == 10.0
    d = ref.distances64(*ref.case_pairs("wide")[0])
    assert d.max() / d.min() > 2.0 ** 24
    d = np.sort(ref.distances64(*ref.case_pairs("duplicates")[0]).reshape(-1))
    assert d[40] == d[41] == d[42] == 10.0                       # the run of equal distances straddles rank (84 - 1) // 2


def test_lower_median_is_sorted_element_n_minus_one_over_two():
    pred, truth = ref.case_pairs("b2")[0]
    d = np.sort(ref.distances64(pred, truth).reshape(-1))
    assert ref.metrics64(pred, truth)[1] == d[20] and d[20] < d[21]


def test_wrapper_refuses_before_any_device_call(monkeypatch):
    from peclr_amd import _capi, calculate_metrics, step_metrics

    def no_launch(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_capi, "_launch", no_launch)
    monkeypatch.setattr(_capi, "lib", no_launch)
    ok = torch.zeros(2, 21, 3)
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        calculate_metrics(ok, ok)
    with pytest.raises(_capi.PeclrHipError, match="no CPU path"):
        step_metrics(ok, ok, ok, ok)
    for bad in (torch.zeros(2, 21, 2), torch.zeros(2, 20, 3), torch.zeros(42, 3), torch.zeros(0, 21, 3), torch.zeros(1025, 21, 3)):
        with pytest.raises(ValueError):
            calculate_metrics(bad, bad)
    with pytest.raises(ValueError, match="differ in shape"):
        calculate_metrics(ok, torch.zeros(3, 21, 3))
    with pytest.raises(ValueError, match="second pair"):
        step_metrics(ok, ok, ok, None)
    with pytest.raises(ValueError, match="same number of samples"):
        step_metrics(ok, ok, torch.zeros(3, 21, 3), torch.zeros(3, 21, 3))
    with pytest.raises(TypeError):
        calculate_metrics(np.zeros((2, 21, 3)), ok)


@pytest.mark.parametrize("step", ["train", "val"])
def test_key_names_are_the_references(monkeypatch, step):
    from peclr_amd import pose_metrics

    monkeypatch.setattr(pose_metrics, "step_metrics", lambda p, t: torch.tensor([1.0, 2.0, 0.0, 0.0]))
    out = pose_metrics.calculate_metrics(torch.zeros(1, 21, 3), torch.zeros(1, 21, 3), step=step)
    assert list(out) == [f"EPE_mean_{step}", f"EPE_median_{step}"]
    assert float(out[f"EPE_mean_{step}"]) == 1.0 and float(out[f"EPE_median_{step}"]) == 2.0


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    """Argument validation happens before the launch, so it is checkable on the CPU."""
    from peclr_amd import _capi

    L = _capi.lib()
    assert L.peclr_pose_step_metrics_f32(None, None, None, None, 4, None, None, None) == -1
    one = 1    # any non-null address: refused before it is read
    assert L.peclr_pose_step_metrics_f32(one, one, None, None, 0, one, one, None) == -2
    assert L.peclr_pose_step_metrics_f32(one, one, None, None, 1025, one, one, None) == -2
    assert L.peclr_pose_step_metrics_f32(one, one, one, None, 4, one, one, None) == -1
