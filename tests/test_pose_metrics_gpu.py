"""The step metrics on the device (csrc/pose_metrics.hip, peclr_amd/pose_metrics.py) against the reference's own results
(tests/golden/g16_step_metrics.json) and the float64 restatement tests/pose_metrics_ref.py (held to the reference at 1e-12 by
tests/test_pose_metrics_host.py).

The bounds.  The kernel evaluates the distances and their sum in float64 and rounds once; the median is selected, not computed.
Against the float64 restatement ON THE SAME INPUTS the mean and the median may each differ by at most 1 float32 ulp (another
summation order and contraction in float64, then one rounding); on the cases whose distances are exact the median is exact.
Against the reference's float32 result the bound is max(1 ulp, e_ref), e_ref = |gold32 - gold64| as the fixture records it.
The `parity` lines this module prints are profiles/pose_step_metrics_parity.txt.
"""
import math

import numpy as np
import pytest
import torch

from tests import pose_metrics_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIX = ref.load_fixture()
SENTINEL = -7.0


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def run_case(name):
    """The case through the launch's one- or two-pair form -> float32 [4] on the host (entries never written: SENTINEL)."""
    from peclr_amd import step_metrics

    pairs = ref.case_pairs(name)
    out = torch.full((4,), SENTINEL, device=DEV)
    args = [dev32(a) for pair in pairs for a in pair]
    assert step_metrics(*args, out=out) is out
    return out.cpu().numpy(), pairs


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("case", FIX["cases"], ids=lambda c: c["name"])
def test_every_fixture_case(case):
    got, pairs = run_case(case["name"])
    assert got.dtype == np.float32
    for i, (entry, (pred, truth)) in enumerate(zip(case["pairs"], pairs)):
        r64 = ref.metrics64(pred, truth)
        for key, dev, want in zip(("mean", "median"), got[2 * i:2 * i + 2], r64):
            g32, g64 = float(entry["gold32"][key]), float(entry["gold64"][key])
            tag = f"{case['name']} pair {i} ({entry['kind']}, B = {entry['B']}) {key}"
            if not math.isfinite(want):
                assert (math.isnan(dev) and math.isnan(want) and math.isnan(g32)) or dev == want == g32, (tag, dev, want, g32)
                print(f"parity {tag}: {dev} (restatement {want}, reference {g32})")
                continue
            ulp = ref.ulp32(want)
            e_dev, e_dev32 = abs(float(dev) - want), abs(float(dev) - g32)
            line = f"parity {tag}: |dev - float64| = {e_dev / ulp:.3f} ulp"
            if "e_ref" in entry:
                bound = max(ulp, entry["e_ref"][key])
                line += f", |dev - reference32| / max(1 ulp, e_ref) = {e_dev32 / bound:.3f} (e_ref = {entry['e_ref'][key] / ulp:.3f} ulp)"
            print(line)
            assert e_dev <= ulp, (tag, float(dev), want)
            if key == "median" and case["name"] in ref.EXACT_MEDIAN:
                assert float(dev) == want == g64 and not np.signbit(dev), (tag, float(dev), want)
            if "e_ref" in entry:
                assert e_dev32 <= bound, (tag, float(dev), g32, bound)
    if len(pairs) == 1:
        assert (got[2:] == SENTINEL).all()


def test_nan_and_inf_semantics():
    got, _ = run_case("nan")
    assert np.isnan(got[:2]).all() and np.isfinite(got[2:]).all()
    from peclr_amd import step_metrics

    second = ref.case_pairs("nan")[1]
    assert np.array_equal(got[2:], step_metrics(dev32(second[0]), dev32(second[1])).cpu().numpy()[:2])   # untouched by the NaN next to it
    got, _ = run_case("nan_second")
    assert np.isfinite(got[:2]).all() and np.isnan(got[2:]).all()
    got, _ = run_case("inf")
    assert np.isposinf(got[0]) and np.isfinite(got[1])
    got, _ = run_case("identical")
    assert (got[:2] == 0).all() and not np.signbit(got[:2]).any()


def test_median_is_torch_median_of_the_rounded_float64_distances():
    """200 random (B, seed), B in 1 .. 64: selection does no arithmetic, so this is exact."""
    from peclr_amd import step_metrics

    g = np.random.default_rng(77)
    ours, theirs = [], []
    for _ in range(200):
        b, seed = int(g.integers(1, 65)), int(g.integers(1 << 30))
        pred, truth = (dev32(a) for a in ref.make_pair(("pixels", "metres", "wide")[seed % 3], b, seed))
        d32 = ((pred.double() - truth.double()) ** 2).sum(2).sqrt().float()
        ours.append(step_metrics(pred, truth)[1])
        theirs.append(torch.median(d32))
    assert torch.equal(bits(torch.stack(ours)), bits(torch.stack(theirs)))


def test_a_null_second_pair_leaves_its_outputs_unwritten():
    from peclr_amd import step_metrics

    (p1, t1), (p2, t2) = ([dev32(a) for a in pair] for pair in ref.case_pairs("scales"))
    both = step_metrics(p1, t1, p2, t2)
    out = torch.full((4,), SENTINEL, device=DEV)
    step_metrics(p1, t1, out=out)
    assert torch.equal(bits(out[:2]), bits(both[:2])) and (out[2:] == SENTINEL).all()
    swapped = step_metrics(p2, t2, p1, t1)
    assert torch.equal(bits(swapped), bits(torch.cat([both[2:], both[:2]])))


def test_eager_runs_and_a_graph_replay_agree_bit_for_bit():
    from peclr_amd import step_metrics

    (p1, t1), (p2, t2) = ([dev32(a) for a in pair] for pair in ref.case_pairs("b128"))
    a = step_metrics(p1, t1, p2, t2).clone()
    b = step_metrics(p1, t1, p2, t2).clone()
    assert torch.equal(bits(a), bits(b))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step_metrics(p1, t1, p2, t2)
    captured.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(captured), bits(a))
    with torch.no_grad():                    # the replay reads its inputs where they lie
        p1.copy_(p2)
        t1.copy_(t2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(captured[:2]), bits(a[2:])) and torch.equal(bits(captured[2:]), bits(a[2:]))


def test_the_call_does_not_synchronise_with_the_host():
    from peclr_amd import calculate_metrics, step_metrics

    (p1, t1), (p2, t2) = ([dev32(a) for a in pair] for pair in ref.case_pairs("scales"))
    step_metrics(p1, t1, p2, t2)                 # (first use: allocator, library load)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step_metrics(p1, t1, p2, t2)
        calculate_metrics(p1, t1, step="val")
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_the_call_is_one_launch():
    from peclr_amd import _capi, step_metrics

    (p1, t1), (p2, t2) = ([dev32(a) for a in pair] for pair in ref.case_pairs("scales"))
    _capi.EVENT_LOG = {}
    try:
        step_metrics(p1, t1, p2, t2)
        torch.cuda.synchronize()
        log = {k: [e[4] for e in v] for k, v in _capi.EVENT_LOG.items()}
    finally:
        _capi.EVENT_LOG = None
    assert log == {"pose_step_metrics": ["1 launch"]}
