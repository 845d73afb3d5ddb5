#!/usr/bin/env python
"""The figures the gates of tests/test_figures_gpu.py are set from, one JSON line:
    python scripts/figures_parity.py [--out profiles/figures_parity.json]
Runs every spectrogram case of that test once (the test module's own measure_planes: one list of cases) and reports, per case, the
largest |gpu - twin| of the magnitude plane (dB) and of the phase plane (rad) over the finite elements, the same in LUT-index units
(256 |difference| / (vmax - vmin) of the twin's plane), and the number of pixels whose colour differs.  The rule, fixed beforehand:
gate = 8 x the largest, rounded up to a power of ten; it has to come out at or below M / 10 = 1e-6 in index units and in radians.

    python scripts/figures_parity.py --seeds
needs no GPU: for every case of tests/figures_twin.py it prints the smallest seed whose signal keeps every unwrap decision and all but
a handful of pixels at least M = 1e-5 away from a boundary (what tests/test_figures_cpu.py asserts of the committed seeds)."""
import argparse
import importlib.util
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def search_seeds():
    import figures_twin as tw
    seeds, special = {}, {}
    for length in tw.LENGTHS:
        for nfft, noverlap in tw.PARAMS:
            seed = 0
            while not tw.case_ok(tw.tone_noise(length, seed), nfft, noverlap):
                seed += 1
            seeds[(length, nfft, noverlap)] = seed
    for name in ("silent", "nan", "overlap"):
        seed = 0
        while True:
            tw.SPECIAL_SEEDS[name] = seed
            rows = tw.overlap_rows() if name == "overlap" else [tw.special_row(name)]
            if all(tw.case_ok(r, 256, 128) for r in rows):
                break
            seed += 1
        special[name] = seed
    print("SEEDS =", seeds)
    print("SPECIAL_SEEDS =", special)


def gate_of(worst):
    return 10.0 ** math.ceil(math.log10(8.0 * worst)) if worst > 0 else 1e-16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seeds", action="store_true")
    a = ap.parse_args()
    if a.seeds:
        search_seeds()
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("figures_parity needs the MI355X: the figures are the GPU's distance from the float64 twin")
    spec = importlib.util.spec_from_file_location("test_figures_gpu", os.path.join(ROOT, "tests", "test_figures_gpu.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    rows = t.measure_planes()
    worst = {k: max(r[k] for r in rows) for k in ("mag_db_abs_diff", "phase_rad_abs_diff", "mag_index_diff", "phase_index_diff")}
    res = dict(bench="figures_parity", device=torch.cuda.get_device_name(0), cases=len(rows), **{"max_" + k: v for k, v in worst.items()},
               gate_rule="8 x the largest difference rounded up to a power of ten; at most 1e-6 in index units and in radians",
               gate_mag_db=gate_of(worst["mag_db_abs_diff"]), gate_phase_rad=gate_of(worst["phase_rad_abs_diff"]),
               gate_index=gate_of(max(worst["mag_index_diff"], worst["phase_index_diff"])),
               pixels_differing=sum(r["mag_pixels_differing"] + r["phase_pixels_differing"] for r in rows),
               all_segment_counts_equal=all(r["segments_equal"] for r in rows), rows=rows)
    res["within_margin"] = bool(res["gate_index"] <= 1e-6 and res["gate_phase_rad"] <= 1e-6)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
