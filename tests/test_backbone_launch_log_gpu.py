"""peclr_amd/bn2d.py routes exactly as the commit tests/golden/backbone_launch_log.json was recorded from: per case (a ResNet, a
routing, an autocast dtype: tools/backbone_launch_log.py) one forward + backward launches the same in-tree kernels in the same
order, hands MIOpen the same convolutions, and computes the same bits -- output, input gradient and every parameter gradient, by
sha256, except the hashes two recordings of that commit did not agree on (arms that are not fixed-order: the file names them).
A change that is meant to alter a route re-records the file."""
import json
import os
import sys

import pytest

from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "backbone_launch_log.json")) as f:
    _GOLDEN = json.load(f)


def test_the_golden_covers_every_case_of_the_tool():
    tool = _tool()
    assert _GOLDEN["recorded_from"] and [c["case"] for c in _GOLDEN["cases"]] == list(tool.CASES)
    assert all(c["launches"] and c["aten"] for c in _GOLDEN["cases"])


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import backbone_launch_log
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return backbone_launch_log


@pytest.mark.parametrize("want", _GOLDEN["cases"], ids=[c["case"] for c in _GOLDEN["cases"]])
def test_one_forward_and_backward_launches_and_computes_what_the_recorded_commit_did(want):
    got = json.loads(json.dumps(_tool().record_case(want["case"])))          # tuples -> lists, as in the file
    assert got["launches"] == want["launches"]
    assert got["aten"] == want["aten"]
    differ = [k for k, v in want["hashes"].items() if got["hashes"].get(k) != v]
    assert not differ, differ
