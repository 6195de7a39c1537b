"""peclr_amd/_capi.py marshals exactly as the commit tests/golden/capi_launch_log.json was recorded from: the same entry points
with the same argument values in the same order, the same null pointers, the same timed tags / bytes / flops / kernel names.

tools/capi_launch_log.py drives every wrapper once per branch on small seeded inputs and summarises what reaches
libpeclr_hip.so (pointers by role, not by address).  The golden file is that log from the last commit before the binding's
calls went through `_launch`; a change that is meant to alter what a wrapper passes re-records it."""
import json
import os
import sys

import pytest

from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def test_every_wrapper_hands_the_library_what_the_recorded_commit_handed_it():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import capi_launch_log
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    with open(os.path.join(GOLDEN, "capi_launch_log.json")) as f:
        golden = json.load(f)
    assert golden["recorded_from"] and not golden["errors"]
    log = json.loads(json.dumps(capi_launch_log.record()))          # tuples -> lists, as in the file
    assert not log["errors"], log["errors"]
    assert [c["case"] for c in log["cases"]] == [c["case"] for c in golden["cases"]]
    for got, want in zip(log["cases"], golden["cases"]):
        assert got["native"] == want["native"], got["case"]
        assert got["timed"] == want["timed"], got["case"]
