#!/usr/bin/env python
"""Micro-benchmark of maavss_video_transform (VideoTransform) on the GPU box, one JSON line:
    python scripts/video_transform_bench.py [--frames 512] [--clip_frames 16] [--size 256] [--iters 20] [--hd_frames 512]
For 512 uint8 frames of 360x640 and of 1080x1920, cropped by sample_boxes (seed 0) and resized to size^2, all four
(antialias x autocontrast) combinations: kernel time per call (HIP events around `iters` back-to-back calls of the C entry point,
buffers allocated once), the compulsory bytes (the source pixels the resize needs read once, the f32 frames written; autocontrast reads and
writes them once more) and the GB/s they imply next to the ~6.3 TB/s a device copy reaches on MI355X.  For context, the same
transform in torch on the host CPU (F.interpolate + Normalize [+ autocontrast], min(16, cpus) threads), per frame, measured on a
few frames (best of 5)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import maavss_amd  # noqa: E402
from maavss_amd import _lib  # noqa: E402

COPY_GBPS = 6300.0


def gpu_case(h0, w0, frames, cf, size, aa, ac, iters, video):
    t = maavss_amd.VideoTransform(size, antialias=aa, autocontrast=ac)
    boxes = t.sample_boxes(frames // cf, h0, w0, torch.Generator().manual_seed(0))
    out = torch.empty(frames, 3, size, size, device="cuda")
    nbytes = _lib.query("maavss_video_transform_ws_bytes", frames, cf, h0, w0, size, int(aa), int(ac))
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    dev_boxes = boxes.cuda()
    args = (_lib.ptr(video), _lib.ptr(dev_boxes), boxes.data_ptr(), _lib.ptr(out), _lib.ptr(ws), nbytes, frames, cf, h0, w0, size,
            *t.mean, *t.std, int(aa), int(ac), _lib.stream_ptr())
    for _ in range(3):
        _lib.call("maavss_video_transform", *args)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        _lib.call("maavss_video_transform", *args)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    # source bytes a resize must read: the whole crop with antialias; without it only the <= 2 S rows and columns next to the samples
    hb, wb = boxes[:, 2].long(), boxes[:, 3].long()
    if not aa:
        hb, wb = hb.clamp(max=2 * size), wb.clamp(max=2 * size)
    crop = int((hb * wb).sum()) * cf * 3
    written = frames * 3 * size * size * 4
    moved = crop + written * (3 if ac else 1)
    # the Python entry point end to end (box copy through pinned memory, workspace allocation), host wall time per call
    t(video, boxes=boxes, clip_frames=cf, out=out)
    torch.cuda.synchronize()
    w0_ = time.perf_counter()
    for _ in range(iters):
        t(video, boxes=boxes, clip_frames=cf, out=out)
    torch.cuda.synchronize()
    call_ms = (time.perf_counter() - w0_) * 1e3 / iters
    return dict(src=f"{h0}x{w0}", frames=frames, clip_frames=cf, size=size, antialias=aa, autocontrast=ac, kernel_ms=round(ms, 4),
                python_call_ms=round(call_ms, 4), bytes=moved, gbps=round(moved / ms / 1e6, 1),
                frac_of_copy=round(moved / ms / 1e6 / COPY_GBPS, 3))


def cpu_ms_per_frame(h0, w0, size, aa, ac, n=8):
    t = maavss_amd.VideoTransform(size)
    top, left, h, w = t.sample_boxes(1, h0, w0, torch.Generator().manual_seed(0))[0].tolist()
    video = torch.randint(0, 256, (n, h0, w0, 3), dtype=torch.uint8)
    mean, std = torch.tensor(t.mean)[:, None, None], torch.tensor(t.std)[:, None, None]

    def run():
        x = (video.permute(0, 3, 1, 2).float() / 255)[:, :, top:top + h, left:left + w]
        x = F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False, antialias=aa)
        x = (x - mean) / std
        if ac:
            lo, hi = x.amin((-2, -1), keepdim=True), x.amax((-2, -1), keepdim=True)
            scale = 1.0 / (hi - lo)
            bad = ~torch.isfinite(scale)
            lo[bad], scale[bad] = 0, 1
            x = ((x - lo) * scale).clamp(0, 1)
        return x
    run()
    best = float("inf")
    for _ in range(5):
        t0 = time.perf_counter()
        run()
        best = min(best, time.perf_counter() - t0)
    return round(best * 1e3 / n, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--clip_frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--hd_frames", type=int, default=512)
    a = ap.parse_args()
    threads = min(16, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    g = torch.Generator(device="cuda").manual_seed(0)
    cases, cpu = [], []
    for (h0, w0, frames) in ((360, 640, a.frames), (1080, 1920, a.hd_frames)):
        video = torch.randint(0, 256, (frames, h0, w0, 3), device="cuda", dtype=torch.uint8, generator=g)
        for aa in (False, True):
            for ac in (False, True):
                cases.append(gpu_case(h0, w0, frames, a.clip_frames, a.size, aa, ac, a.iters, video))
                cpu.append(dict(src=f"{h0}x{w0}", antialias=aa, autocontrast=ac, ms_per_frame=cpu_ms_per_frame(h0, w0, a.size, aa, ac)))
        del video
    print(json.dumps(dict(bench="video_transform", device=torch.cuda.get_device_name(0), copy_gbps_reference=COPY_GBPS, gpu=cases,
                          cpu_torch=dict(threads=threads, cases=cpu))))


if __name__ == "__main__":
    main()
