#!/usr/bin/env python
"""The figure the gate of tests/test_bss_gpu.py is set from, one JSON line:
    python scripts/bss_parity.py [--out profiles/bss_parity.json]
Runs every case of that test once (the test module's own measure()) and reports, per row, |gpu - twin| in dB of every finite score and
the relative difference of every finite non-zero sum, and the largest of them.  The rule: gate = 8 x the largest, rounded up to a power
of ten, and never above one thousandth of the off-by-one sensitivity tests/test_bss_cpu.py prints."""
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
        raise SystemExit("bss_parity needs the MI355X: the figure is the GPU's distance from the float64 twin")
    spec = importlib.util.spec_from_file_location("test_bss_gpu", os.path.join(ROOT, "tests", "test_bss_gpu.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    recs = t.measure()
    rows = []
    for r in recs:
        got, want = r["got"], r["want"]
        rows.append(dict(case=r["label"], n_sources=int(got[8]), status=int(got[9]),
                         counts_equal=bool(got[8] == want["n_sources"] and got[9] == want["status"]),
                         sdr_db=float(got[5]), sir_db=float(got[6]), sar_db=float(got[7]),
                         twin=[want["sdr_db"], want["sir_db"], want["sar_db"]]))
    diffs = t.differences(recs)
    by = {}
    for d, label, key in diffs:
        by.setdefault(label, {})[key] = d
    for row in rows:
        row["diff"] = by.get(row["case"], {})
    worst = max(diffs)
    worst_score = max(d for d in diffs if d[2] in t.tw.SCORES)
    worst_sum = max(d for d in diffs if d[2] in t.tw.SUMS)
    gate = 10.0 ** math.ceil(math.log10(8.0 * worst[0])) if worst[0] > 0 else 1e-16
    res = dict(bench="bss_parity", device=torch.cuda.get_device_name(0), finite_values=len(diffs), max_diff=worst[0], max_diff_at=list(worst[1:]),
               max_score_diff_db=worst_score[0], max_score_diff_at=list(worst_score[1:]), max_sum_rel_diff=worst_sum[0],
               max_sum_rel_diff_at=list(worst_sum[1:]), gate_rule="8 x max_diff rounded up to a power of ten", gate=gate,
               all_counts_equal=all(row["counts_equal"] for row in rows), rows=rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
