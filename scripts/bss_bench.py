#!/usr/bin/env python
"""Micro-benchmark of the BSS-eval scores (csrc/bss_eval.hip), one JSON line:
    python scripts/bss_bench.py [--iters 5] [--repeats 5] [--out profiles/bss_bench.json]
Every figure is the median over `repeats` of HIP events on the stream around `iters` back-to-back calls, after 2 warm-up calls, in
microseconds.  maavss_amd.bss_eval_metrics(est, ref, others, 512) with one other source (1024 unknowns per row) at 32 x 8448 and
256 x 8448 samples and on one row of 960 000; next to each, maavss_amd.wave_metrics on the same rows in the same run, the figure to
orient by.  `fma_per_row` = (J L)^3 / 3, the factorisation's multiply-adds; `factor_gfma_per_s` divides all rows' by the whole call, so
it understates the factorisation's own rate (the per-kernel times are in profiles/bss_kernels.txt, from a kernel trace of this
script).  No speed gate is set."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maavss_amd  # noqa: E402
from maavss_amd.bss import BSS_WORKSPACE_CAP  # noqa: E402
from maavss_amd._lib import query  # noqa: E402


def timed(fn, iters, repeats, warm=2):
    for _ in range(warm):
        fn()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / iters)
    return round(statistics.median(us), 1), round(min(us), 1), round(max(us), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bss_bench needs the MI355X: nothing here can be measured on a CPU")
    g = torch.Generator(device="cuda").manual_seed(3)
    filt, k = 512, 1
    res = dict(bench="bss_eval", device=torch.cuda.get_device_name(0), iters=a.iters, repeats=a.repeats, filt_len=filt, others=k, rows=[])
    for b, n in ((32, 8448), (256, 8448), (1, 960000)):
        ref = 0.1 * torch.randn(b, n, device="cuda", generator=g)
        oth = 0.1 * torch.randn(b, k, n, device="cuda", generator=g)
        est = ref + 0.3 * oth[:, 0] + 0.005 * torch.randn(b, n, device="cuda", generator=g)
        us, lo, hi = timed(lambda: maavss_amd.bss_eval_metrics(est, ref, oth, filt), a.iters, a.repeats)
        wus, wlo, whi = timed(lambda: maavss_amd.wave_metrics(est, ref, 256), a.iters, a.repeats)
        out = maavss_amd.bss_eval_metrics(est, ref, oth, filt)["raw"].cpu()
        per_row = int(query("maavss_bss_eval_ws_bytes", 1, n, k, filt))
        unknowns = (k + 1) * filt
        res["rows"].append(dict(shape=[b, n], unknowns=unknowns, bss_us=us, bss_us_min=lo, bss_us_max=hi, launches=7 + 2 * (unknowns // 64),
                                row_groups=-(-b // max(1, min(b, BSS_WORKSPACE_CAP // per_row))), workspace_bytes_per_row=per_row,
                                wave_metrics_us=wus, wave_metrics_us_min=wlo, wave_metrics_us_max=whi, bss_over_wave_metrics=round(us / wus, 1),
                                fma_per_row=unknowns ** 3 // 3, factor_gfma_per_s=round(b * unknowns ** 3 / 3 / us / 1e3, 1),
                                status_ok=int((out[:, 9] == 0).sum()), mean_sdr_db=round(float(out[:, 5].mean()), 3),
                                mean_sir_db=round(float(out[:, 6].mean()), 3), mean_sar_db=round(float(out[:, 7].mean()), 3)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
