#!/usr/bin/env python
"""Micro-benchmark of the mixed front end (maavss_amd.Mixer) against the plain STFT call on the same clips, one JSON line:
    python scripts/mix_bench.py [--iters 20] [--repeats 9] [--out profiles/mix_bench.json]
B = 32 and 256 clips of 8448 samples, 512-point STFT (hop 66, 128 frames, 257 bins), K = 1 and 4 interferers from the batch, in-kernel
noise.  Timed at the C entry points with buffers allocated once: `plain` = maavss_stft_fwd writing y and x; `mixed` = maavss_stft_fwd
writing y only + maavss_mix_gains + maavss_stft_mix_fwd, what Mixer.__call__ launches.  Each figure is the median over `repeats` of HIP
events on the stream around `iters` back-to-back calls, after 3 warm-up calls; the three kernels of the mixed path are also timed one by
one, and `call_*_us` time the Python calls themselves (`stft(audio, seed=)` and `mixer(audio, partners, snr_db, seed=)`: allocation of the
outputs, host checks and the pinned staging copy of partners and SNR factors included).  `bytes` are the algorithmic ones (every input row read once per kernel that reads it, every output written once)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maavss_amd  # noqa: E402
from maavss_amd import _lib  # noqa: E402
from oracle import stft_ref_cpu as sref  # noqa: E402

FFT, HOP, LENGTH = 512, 66, 8448


def timed(fn, iters, repeats):
    for _ in range(3):
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
    return round(statistics.median(us), 2)


def case(b, k, iters, repeats):
    st = maavss_amd.STFT(FFT, HOP, noise_std=0.1, device="cuda")
    mixer = maavss_amd.Mixer(st, k)
    audio = sref.synthetic_audio(b, LENGTH, 31).cuda()
    partners, snr = mixer.sample(b, torch.Generator().manual_seed(1))
    partners_d = partners.cuda()
    factor_d = torch.pow(10.0, -snr.double() / 20.0).float().cuda()
    t, f = LENGTH // HOP, st.n_bins()
    y = torch.empty(b, 2, t, f, device="cuda")
    x = torch.empty_like(y)
    gain = torch.empty(b, device="cuda")
    sp = _lib.stream_ptr()
    p = _lib.ptr

    def stft(with_x):
        _lib.call("maavss_stft_fwd", p(audio), b, LENGTH, LENGTH, p(st.window), FFT, HOP, t, f, p(y), p(x) if with_x else None, None,
                  0.1, 5, None, sp)

    def gains():
        _lib.call("maavss_mix_gains", p(audio), b, LENGTH, LENGTH, p(audio), b, LENGTH, p(partners_d), k, p(factor_d), p(gain), sp)

    def mix():
        _lib.call("maavss_stft_mix_fwd", p(audio), b, LENGTH, LENGTH, p(partners_d), k, b, p(st.window), FFT, HOP, t, f, p(y), p(x), None,
                  0.1, 5, p(gain), None, sp)

    def mixed():
        stft(False)
        gains()
        mix()

    clip, spec = 4 * b * LENGTH, 4 * y.numel()
    plain_us, mixed_us = timed(lambda: stft(True), iters, repeats), timed(mixed, iters, repeats)
    plain_bytes = clip + 2 * spec
    mixed_bytes = (clip + spec) + (1 + k) * clip + (k * clip + 2 * spec)
    return dict(clips=b, interferers=k, plain_us=plain_us, mixed_us=mixed_us, ratio=round(mixed_us / plain_us, 2),
                stft_y_only_us=timed(lambda: stft(False), iters, repeats), mix_gains_us=timed(gains, iters, repeats),
                stft_mix_us=timed(mix, iters, repeats), call_plain_us=timed(lambda: st(audio, seed=5), iters, repeats),
                call_mixed_us=timed(lambda: mixer(audio, partners, snr, seed=5), iters, repeats), plain_bytes=plain_bytes, mixed_bytes=mixed_bytes,
                bytes_ratio=round(mixed_bytes / plain_bytes, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cases = [case(b, k, a.iters, a.repeats) for b in (32, 256) for k in (1, 4)]
    line = json.dumps(dict(bench="mix", device=torch.cuda.get_device_name(0), n_fft=FFT, hop=HOP, samples=LENGTH, iters=a.iters,
                           repeats=a.repeats, cases=cases))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
