"""Golden results for the metrics of a supervised step (peclr_amd/pose_metrics.py, csrc/pose_metrics.hip).

Run where the reference checkout is present (tests/golden/_ref_import.py names its place):

    python tests/golden/make_golden_metrics.py

Calls the reference's own `calculate_metrics` (src/models/utils.py) on the float32 inputs that tests/pose_metrics_ref.py
draws for each case (the fixture records no input: the tests draw the same arrays from the same seeds) and on .double() copies
of them.

Fixture: g16_step_metrics.json, numbers only.  Per case `pairs`, one entry per (prediction, truth) pair:

  kind, B, seed   what `make_pair` is called with
  gold32          {"mean", "median"}: the reference on the float32 tensors (a float32, written as the double it equals)
  gold64          the same on the float64 copies
  e_ref           {"mean", "median"}: |gold32 - gold64|, the reference's own float32 deviation (finite cases only)

Non-finite results are the strings "nan" / "inf".
"""
import json
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ref_import  # noqa: E402

_ref_import.install_stubs()
from src.models.utils import calculate_metrics  # noqa: E402

from tests import pose_metrics_ref as ref  # noqa: E402


def number(x):
    x = float(x)
    return x if math.isfinite(x) else ("nan" if math.isnan(x) else "inf")


def run(pred, truth):
    out = calculate_metrics(pred, truth, step="gold")
    return {"mean": number(out["EPE_mean_gold"]), "median": number(out["EPE_median_gold"])}


def main():
    torch.set_num_threads(1)
    cases = []
    for name, specs in ref.CASES.items():
        pairs = []
        for (kind, b, seed), (pred, truth) in zip(specs, ref.case_pairs(name)):
            p, t = torch.from_numpy(pred), torch.from_numpy(truth)
            entry = {"kind": kind, "B": b, "seed": seed, "gold32": run(p, t), "gold64": run(p.double(), t.double())}
            if all(isinstance(entry[g][k], float) for g in ("gold32", "gold64") for k in ("mean", "median")):
                entry["e_ref"] = {k: abs(entry["gold32"][k] - entry["gold64"][k]) for k in ("mean", "median")}
            pairs.append(entry)
        cases.append({"name": name, "pairs": pairs})
    path = os.path.join(HERE, "g16_step_metrics.json")
    with open(path, "w") as f:
        json.dump({"cases": cases}, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases")
    for c in cases:
        for p in c["pairs"]:
            print(c["name"], p["kind"], p["B"], p["gold64"], p.get("e_ref"))


if __name__ == "__main__":
    main()
