#!/usr/bin/env python
"""What the per-clip crop and flip of the clip bank's maps costs (ClipBank.batch(boxes=, flip=); maavss_bank_warp_maps), one JSON line:
    python scripts/bank_warp_bench.py [--iters 20] [--repeats 9] [--out profiles/bank_warp_bench.json]
On one MI355X, alone on the card.  Shapes of bench.py: clips of 16 frames at 224^2 and 8448 samples (hops_per_frame 8, hop 66).

B = 32 and 256 clips cut at seeded random positions from a bank of 64 recordings of 64 frames (synthetic maps), both storages, boxes and
flips from BankCrop(flip=0.5).  In ONE process and alternating, repeat by repeat: `plain_us`, HIP events around `iters` back-to-back
bank.batch(indices, out=..) calls (the path this feature does not touch), and `warped_us`, the same around
bank.batch(indices, boxes=, flip=, out=..); each the median over `repeats`, after 3 warm-up calls of both.  `*_host_us` is the host
clock per call of those loops (which end before the device does): the box check, the larger staging tensor and the workspace
allocation are host work.  `warp_us` times the C entry point alone with tables and workspace allocated once.  `warp_bytes` are
counted: four taps of 2 or 4 bytes per output value at most (they hit L2), the value written, read and written again (frame_norm);
`warp_share` = warp_bytes / the plain batch's bytes."""
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
from maavss_amd import _lib  # noqa: E402

T, S, HPF = 16, 224, 8
HOP, LENGTH, _ = maavss_amd.calc_hop_size(T, HPF, 30, 16000)


def event_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def host_us(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    us = (time.perf_counter() - t0) * 1e6 / iters
    torch.cuda.synchronize()
    return us


def case(b, storage, iters, repeats):
    n_rec, n_frames, frame_hop = 64, 64, 4
    n_samples = round((n_frames - T) * 16000 / 30) + LENGTH + 1
    bank = maavss_amd.ClipBank(S, T, frame_hop, HPF, HOP, capacity_frames=n_rec * n_frames, capacity_samples=n_rec * n_samples, storage=storage)
    g = torch.Generator().manual_seed(1)
    for _ in range(n_rec):
        bank.add_recording(torch.randn(n_samples, generator=g).cuda(), maps=torch.rand(n_frames, bank.frame_elems, generator=g).cuda())
    indices = torch.randint(0, len(bank), (b,), generator=g)
    boxes, flip = maavss_amd.BankCrop(flip=0.5).sample(b, S, g)
    attn = torch.empty(b, 1, T, S, S, device="cuda")
    audio = torch.empty(b, LENGTH, device="cuda")
    starts = bank.check_indices(indices)
    staged = bank._stage(*starts, bank.check_warp(b, boxes, flip))
    ws = torch.empty(b * T, bank.frame_elems, device="cuda")
    sp, p, code = _lib.stream_ptr(), _lib.ptr, 1 if storage == "u16" else 0

    def plain():
        bank.batch(indices, out=(attn, audio))

    def warped():
        bank.batch(indices, boxes=boxes, flip=flip, out=(attn, audio))

    def warp():
        _lib.call("maavss_bank_warp_maps", p(bank.maps), code, p(staged[2 * b:]), p(staged[4 * b:]), p(staged[8 * b:]), b, bank.n_frames, T, S,
                  1, p(ws), sp)

    for _ in range(3):
        plain(), warped(), warp()
    rows = {k: [] for k in ("plain_us", "warped_us", "warp_us", "plain_host_us", "warped_host_us")}
    for _ in range(repeats):                             # alternating: a drift of the clocks reaches every figure alike
        rows["plain_us"].append(event_us(plain, iters))
        rows["warped_us"].append(event_us(warped, iters))
        rows["warp_us"].append(event_us(warp, iters))
        rows["plain_host_us"].append(host_us(plain, iters))
        rows["warped_host_us"].append(host_us(warped, iters))
    res = {k: round(statistics.median(v), 2) for k, v in rows.items()}
    esz = bank.maps.element_size()
    warp_bytes = ws.numel() * (4 * esz + 12) + 24 * b
    batch_bytes = attn.numel() * 4 + 2 * ws.numel() * esz + 2 * audio.numel() * 4 + 20 * b
    return dict(clips=b, storage=storage, bank_clips=len(bank), **res, extra_us=round(res["warped_us"] - res["plain_us"], 2),
                extra_host_us=round(res["warped_host_us"] - res["plain_host_us"], 2), warp_bytes=warp_bytes, batch_bytes=batch_bytes,
                warp_share=round(warp_bytes / batch_bytes, 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(bench="bank_warp", device=torch.cuda.get_device_name(0), frames=T, framesize=S, samples=LENGTH, iters=a.iters, repeats=a.repeats,
               batch=[case(b, storage, a.iters, a.repeats) for b in (32, 256) for storage in ("f32", "u16")])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
