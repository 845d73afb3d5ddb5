#!/usr/bin/env python
"""Micro-benchmark of maavss_amd.Reverb, one JSON line:
    python scripts/reverb_bench.py [--iters 10] [--repeats 7] [--out profiles/reverb_bench.json] [--parity profiles/reverb_parity.json]
B = 32 and 256 clips of 8448 samples, K = 4096 and 8192 taps, 64 rooms.  `bank_us`: Reverb.bank_clips on a ClipBank of 16 recordings of
20 s (clips of 16 frames, one every 16 frames), the clips drawn at random, so nearly every one has K - 1 samples of history;
`zero_us`: Reverb.__call__ on the same clips cut dry, from zero state (about K / (2 L) of the terms fall in front of the clip);
`make_rirs_us`: make_rirs(64) drawing its normals.  Each figure is the median over `repeats` of HIP events on the stream around
`iters` back-to-back Python calls (host checks, output allocation and the pinned staging copy included), after 3 warm-up calls.
`macs` counts the f64 multiply-adds of the definition from the tables (the terms with p >= floor), `vector_share` is macs / time over
39.3e12 multiply-adds a second (the f64 vector rate: half the 157.3 TFLOP/s f32 one).  `conv1d_f32_us`, for orientation only:
torch.nn.functional.conv1d in f32 on the zero-padded dry clips with ONE room for the whole batch (another definition: f32 sums in an
unstated order, no history), timed the same way with fewer iterations.
--parity: how many taps of a 16 x 8192 table made from given normals are identical to tests/reverb_twin.py's (the rest are one f32
ulp away: the device's exp is not numpy's)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import maavss_amd  # noqa: E402
import reverb_twin as tw  # noqa: E402

T, HPF, HOP, S, FRAME_HOP = 16, 8, 66, 16, 16
LENGTH = HPF * HOP * T                 # 8448
VECTOR_MACS = 39.3e12
ROOMS = 64


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


def make_bank():
    frames, samples, recs = 600, 320000, 16
    bank = maavss_amd.ClipBank(S, T, FRAME_HOP, HPF, HOP, capacity_frames=frames * recs, capacity_samples=samples * recs)
    g = torch.Generator().manual_seed(0)
    for _ in range(recs):
        bank.add_recording((torch.rand(samples, generator=g) - 0.5).cuda(), maps=torch.rand(frames, (S // 8) ** 2, generator=g).cuda())
    return bank


def macs(start, floor, k):
    n = torch.arange(LENGTH, dtype=torch.int64)
    return int(torch.clamp((start - floor)[:, None] + n[None, :] + 1, max=k).sum())


def case(bank, b, k, iters, repeats):
    rv = maavss_amd.Reverb(k)
    rv.make_rirs(ROOMS, seed=1)
    indices = torch.randint(0, len(bank), (b,), generator=torch.Generator().manual_seed(b + k))
    index = rv.sample_index(b, torch.Generator().manual_seed(2))
    _, start = bank.check_indices(indices)
    floor = maavss_amd.reverb.bank_floor(bank, indices)
    _, dry = bank.batch(indices)
    out = torch.empty(b, LENGTH, device="cuda")
    bank_us = timed(lambda: rv.bank_clips(bank, indices, index, out=out), iters, repeats)
    zero_us = timed(lambda: rv(dry, index), iters, repeats)
    bank_macs, zero_macs = macs(start, floor, k), macs(start, start, k)
    res = dict(clips=b, taps=k, bank_us=bank_us, bank_macs=bank_macs, bank_vector_share=round(bank_macs / (bank_us * 1e-6) / VECTOR_MACS, 3),
               zero_us=zero_us, zero_macs=zero_macs, zero_vector_share=round(zero_macs / (zero_us * 1e-6) / VECTOR_MACS, 3))
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res, dry, rv


def conv1d_us(dry, rv, k, iters, repeats):
    x = torch.nn.functional.pad(dry, (k - 1, 0))[:, None, :]
    w = rv.rirs[0].flip(0)[None, None, :].contiguous()
    return timed(lambda: torch.nn.functional.conv1d(x, w), iters, repeats)


def parity(path):
    k, rows, sr = 8192, 16, 16000
    rng = np.random.default_rng(0)
    noise = rng.standard_normal((rows, k)).astype(np.float32)
    rt60, drr, pre = np.linspace(0.1, 0.8, rows), np.linspace(0.0, 12.0, rows), np.linspace(16, 80, rows).astype(np.int64)
    got = maavss_amd.Reverb(k, sr=sr).make_rirs(rows, rt60=torch.from_numpy(rt60), drr_db=torch.from_numpy(drr), predelay=torch.from_numpy(pre),
                                                  noise=torch.from_numpy(noise).cuda()).cpu().numpy()
    want = np.stack([tw.rir(noise[r], tw.lam_of(rt60[r], sr), 10.0 ** (drr[r] / 10.0), pre[r])[0] for r in range(rows)])
    d = tw.ulp_distance_f32(got, want)
    line = json.dumps(dict(check="reverb_parity", device=torch.cuda.get_device_name(0), rows=rows, taps=k, taps_total=int(d.size),
                           taps_identical=int((d == 0).sum()), taps_one_ulp=int((d == 1).sum()), max_ulps=int(d.max())))
    print(line)
    with open(path, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parity", default=None)
    a = ap.parse_args()
    if a.parity:
        parity(a.parity)
    bank = make_bank()
    cases, kept = [], []
    for b in (32, 256):
        for k in (4096, 8192):
            res, dry, rv = case(bank, b, k, a.iters, a.repeats)
            cases.append(res)
            kept.append((dry, rv, k))
    synth = {str(k): timed(lambda: maavss_amd.Reverb(k).make_rirs(ROOMS, seed=3), a.iters, a.repeats) for k in (4096, 8192)}

    def emit():
        line = json.dumps(dict(bench="reverb", device=torch.cuda.get_device_name(0), samples=LENGTH, rooms=ROOMS, iters=a.iters, repeats=a.repeats,
                               vector_macs_per_s=VECTOR_MACS, make_rirs_us=synth, cases=cases))
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    emit()                                           # the library's figures are on disk before torch's convolution is tried
    for res, (dry, rv, k) in zip(cases, kept):
        res["conv1d_f32_us"] = conv1d_us(dry, rv, k, 3, 3)
        print(json.dumps(res), file=sys.stderr, flush=True)
        emit()
    print(emit())


if __name__ == "__main__":
    main()
