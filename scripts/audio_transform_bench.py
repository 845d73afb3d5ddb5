#!/usr/bin/env python
"""Micro-benchmark of maavss_audio_transform (AudioTransform) on the GPU box, one JSON line:
    python scripts/audio_transform_bench.py [--iters 20] [--out profiles/audio_transform_bench.json]
Stereo int16 at 48 000 and 44 100 Hz -> 16 kHz mono f32, with and without contrast, for the benched batch (32 clips of
input_length(8448, sr) samples, cropped to 8448) and a 60 s recording: kernel time per call (HIP events around `iters` back-to-back calls
of the C entry point after 3 warm-up calls, buffers allocated once), the algorithmic bytes (input read once + output written) and the GB/s
they imply.  For scale, the same arithmetic in torch on the host (tests/audio_twin.py, min(16, cpus) threads, best of 3)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audio_twin as tw  # noqa: E402
import maavss_amd  # noqa: E402
from maavss_amd import _lib  # noqa: E402


def gpu_case(name, x, sr, length, contrast, iters):
    t = maavss_amd.AudioTransform(16000, compress_audio=contrast)
    b, c, l0 = x.shape
    orig, new = t._ratio(sr)
    taps, first, s, width = t._device_table(sr, x.device)
    out = torch.empty(b, length, device="cuda")
    args = (_lib.ptr(x), 1, b, c, l0, x.stride(0), x.stride(1), _lib.ptr(taps), _lib.ptr(first), orig, new, s, width, 0, int(contrast),
            _lib.ptr(out), length, length, None, 0, _lib.stream_ptr())
    for _ in range(3):
        _lib.call("maavss_audio_transform", *args)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        _lib.call("maavss_audio_transform", *args)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    moved = x.numel() * 2 + out.numel() * 4
    return dict(case=name, sr=sr, clips=b, channels=c, in_samples=l0, out_samples=length, contrast=contrast, kernel_us=round(us, 2),
                bytes=moved, gbps=round(moved / us / 1e3, 1))


def cpu_ms(x, sr, length, contrast):
    xc = x.cpu()
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        tw.chain(xc, sr, compress_audio=contrast, length=length)
        best = min(best, time.perf_counter() - t0)
    return round(best * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    threads = min(16, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    t = maavss_amd.AudioTransform(16000)
    gpu, cpu = [], []
    for sr in (48000, 44100):
        for name, b, n_out in (("benched batch", 32, 8448), ("60 s recording", 1, 60 * 16000)):
            x = tw.signal(b, 2, t.input_length(n_out, sr), sr + b, torch.int16).cuda()
            for contrast in (False, True):
                gpu.append(gpu_case(name, x, sr, n_out, contrast, a.iters))
                cpu.append(dict(case=name, sr=sr, contrast=contrast, ms=cpu_ms(x, sr, n_out, contrast)))
    line = json.dumps(dict(bench="audio_transform", device=torch.cuda.get_device_name(0), gpu=gpu, cpu_torch=dict(threads=threads, cases=cpu)))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
