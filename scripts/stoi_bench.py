#!/usr/bin/env python
"""Micro-benchmark of the intelligibility scores (csrc/stoi.hip), one JSON line:
    python scripts/stoi_bench.py [--iters 50] [--repeats 9] [--out profiles/stoi_bench.json]
Every figure is the median over `repeats` of HIP events on the stream around `iters` back-to-back calls, after 3 warm-up calls, in
microseconds.  maavss_amd.stoi_metrics(est, ref, sr) at 32 x 5280, 256 x 5280 and 1 x 600 000 samples at sr = 10000, and at 32 x 8448 at
sr = 16000 (both arrays through the device resampler first); next to each, maavss_amd.wave_metrics on the same rows in the same run, the
figure to orient by.  A call also allocates its output and workspace and asks the library for the workspace size, so at the small shapes
the figure is the host's time per call (six launches, and two resampler calls before them at 16 kHz), not the kernels'.  `transforms` = workgroups of the bands
kernel, each two 512-point f64 transforms in LDS: the device work is theirs.  No speed gate is set."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maavss_amd  # noqa: E402


def timed(fn, iters, repeats, warm=3):
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
    return round(statistics.median(us), 2), round(min(us), 2), round(max(us), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stoi_bench needs the MI355X: nothing here can be measured on a CPU")
    g = torch.Generator(device="cuda").manual_seed(3)
    res = dict(bench="stoi", device=torch.cuda.get_device_name(0), iters=a.iters, repeats=a.repeats, rows=[])
    for b, n, sr in ((32, 5280, 10000), (256, 5280, 10000), (1, 600000, 10000), (32, 8448, 16000)):
        # speech-like level changes, so that the mask and the clipping have something to do: noise under a slow envelope
        t = torch.arange(n, device="cuda") / sr
        ref = 0.3 * (0.55 + 0.45 * torch.sin(2 * torch.pi * 3.0 * t)) * torch.randn(b, n, device="cuda", generator=g)
        est = ref + 0.1 * torch.randn(b, n, device="cuda", generator=g)
        us, lo, hi = timed(lambda: maavss_amd.stoi_metrics(est, ref, sr=sr), a.iters, a.repeats)
        wus, wlo, whi = timed(lambda: maavss_amd.wave_metrics(est, ref, 256), a.iters, a.repeats)
        out = maavss_amd.stoi_metrics(est, ref, sr=sr)["raw"].cpu()
        n10 = n if sr == 10000 else -(-n * 10000 // sr)
        frames = len(range(0, n10 - 256, 128))
        res["rows"].append(dict(shape=[b, n], sr=sr, stoi_us=us, stoi_us_min=lo, stoi_us_max=hi, launches=6, resampler_calls=0 if sr == 10000 else 2,
                                wave_metrics_us=wus, wave_metrics_us_min=wlo, wave_metrics_us_max=whi, stoi_over_wave_metrics=round(us / wus, 2),
                                frames_per_row=frames, transforms=int(out[:, 2].clamp(min=1).sub(1).sum()), segments=int(out[:, 3].sum()),
                                mean_stoi=round(float(out[:, 0].mean()), 4), mean_estoi=round(float(out[:, 1].mean()), 4)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
