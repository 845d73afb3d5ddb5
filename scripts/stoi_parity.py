#!/usr/bin/env python
"""The figure the gate of tests/test_stoi_gpu.py is set from, one JSON line:
    python scripts/stoi_parity.py [--out profiles/stoi_parity.json]
Runs every case of that test once (the test module's own measure_10k and measure_16k: one list of cases) and reports, per finite row,
|gpu - twin| of stoi and estoi, and the largest of them.  The rule: gate = 8 x the largest, rounded up to a power of ten, never above
1e-9; a largest difference above 1.25e-10 means something other than rounding differs."""
import argparse
import importlib.util
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stoi_parity needs the MI355X: the figure is the GPU's distance from the float64 twin")
    spec = importlib.util.spec_from_file_location("test_stoi_gpu", os.path.join(ROOT, "tests", "test_stoi_gpu.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    rows = []
    for group, recs in (("sr10000", t.measure_10k()), ("sr16000", t.measure_16k())):
        for r in recs:
            row = dict(case=r["label"], group=group, n_kept=int(r["got"][2]), n_segments=int(r["got"][3]),
                       counts_equal=bool(r["got"][2] == r["want"]["n_kept"] and r["got"][3] == r["want"]["n_segments"]))
            for c, key in enumerate(("stoi", "estoi")):
                if math.isfinite(r["want"][key]):
                    row[key] = float(r["got"][c])
                    row[key + "_abs_diff"] = abs(float(r["got"][c]) - r["want"][key])
            rows.append(row)
    diffs = [row[k] for row in rows for k in ("stoi_abs_diff", "estoi_abs_diff") if k in row]
    worst = max(diffs)
    gate = min(1e-9, 10.0 ** math.ceil(math.log10(8.0 * worst))) if worst > 0 else 1e-16
    res = dict(bench="stoi_parity", device=torch.cuda.get_device_name(0), finite_scores=len(diffs), max_abs_diff=worst,
               gate_rule="8 x max_abs_diff rounded up to a power of ten, at most 1e-9", gate=gate, within_rounding=bool(worst <= 1.25e-10),
               all_counts_equal=all(row["counts_equal"] for row in rows), rows=rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
