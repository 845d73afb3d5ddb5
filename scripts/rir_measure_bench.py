#!/usr/bin/env python
"""Micro-benchmark of maavss_amd.Reverb.measure and of make_room_rirs(calibrate=), one JSON line:
    python scripts/rir_measure_bench.py [--iters 20] [--repeats 5] [--out profiles/rir_measure_bench.json]
`measure`: tables of 256 rows x K = 4096 and 8192 taps (Reverb.make_rirs' decaying noise, rt60 0.2 to 0.8 s), and 4096 rows x 8192
for what the chip does when every CU has several rows.  `us`: the median over `repeats` of HIP events around `iters` back-to-back
Python calls (host checks and the output allocation included), after 2 warm-up calls.  `bytes`: the table read twice (totals, then
crossings) plus the output; `tb_per_s` that over `us`, to set against the 8 TB/s HBM roof (a 256-row table, 8 MiB, stays in the
cache between the two passes: the figure is a rate of traffic asked for, not of HBM traffic measured).
`calibrate`: ONE make_room_rirs(calibrate="t20") of 64 rooms x 4 sources drawn by sample_rooms (default ranges) with requested times
of 0.2 to 0.8 s, stored K = 8192, default measure_len: wall-clock milliseconds (it synchronises once a round), the rounds it took,
how many rooms converged, the worst relative miss, and for orientation the uncalibrated call's wall time on the same rooms."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maavss_amd  # noqa: E402

SR = 16000


def timed(fn, iters, repeats):
    for _ in range(2):
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
    return round(statistics.median(us), 1)


def measure_case(rows, k, iters, repeats):
    rv = maavss_amd.Reverb(k, sr=SR)
    rv.make_rirs(rows, seed=3)
    us = timed(rv.measure, iters, repeats)
    nbytes = 2 * rows * k * 4 + rows * 6 * 8
    res = dict(rows=rows, taps=k, us=us, bytes=nbytes, tb_per_s=round(nbytes / (us * 1e-6) / 1e12, 3))
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 2)


def calibrate_case(rooms=64, sources=4, k=8192):
    rv = maavss_amd.Reverb(k, sr=SR)
    dims, mic, src, rt60 = rv.sample_rooms(rooms, torch.Generator().manual_seed(0), sources=sources)
    rv.make_room_rirs(dims, mic, src, rt60=rt60)                                        # warm-up: the library, the allocator
    plain_ms = wall_ms(lambda: rv.make_room_rirs(dims, mic, src, rt60=rt60))
    nominal = rv.measure()["t20"].reshape(rooms, sources).mean(dim=1).cpu()
    ms = wall_ms(lambda: rv.make_room_rirs(dims, mic, src, rt60=rt60, calibrate="t20"))
    miss = ((rv.room_measured - rt60).abs() / rt60)
    res = dict(rooms=rooms, sources=sources, taps=k, measure_len=rv.check_calibration(dims, rt60, None, "t20", 0.02, 12, None), ms=ms,
               rounds=rv.calibration_rounds, converged=int(rv.room_converged.sum()), worst_relative_miss=round(float(miss.max()), 5),
               uncalibrated_ms=plain_ms, uncalibrated_ratio_min=round(float((nominal / rt60).min()), 3),
               uncalibrated_ratio_max=round(float((nominal / rt60).max()), 3))
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    measure = [measure_case(rows, k, a.iters, a.repeats) for rows, k in ((256, 4096), (256, 8192), (4096, 8192))]
    line = json.dumps(dict(bench="rir_measure", device=torch.cuda.get_device_name(0), sr=SR, iters=a.iters, repeats=a.repeats, measure=measure,
                           calibrate=calibrate_case()))
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
