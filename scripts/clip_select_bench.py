#!/usr/bin/env python
"""Measurements of the clip activity pass (maavss_amd.ClipBank.activity, csrc/clip_select.hip), one JSON line:
    python scripts/clip_select_bench.py [--recordings 64] [--frames 2048] [--iters 5] [--repeats 7] [--out profiles/clip_select_bench.json]
On one MI355X, alone on the card.  Shapes of bench.py: clips of 16 frames at 224^2 (784 map values a frame) and 8448 samples
(hops_per_frame 8, hop 66: 128 segments a clip).

A synthetic bank of `recordings` recordings of `frames` frames (noise and uniform maps made on the device through maps=: the time of
a reduction does not depend on the values), both storages, with frame_hop 2 (clips overlap eightfold) and frame_hop = clip_frames
(clips tile the recording).  Per case: `level_us`, `motion_us`, `clips_us` time the three C entry points with tables and outputs
allocated once, `select_us` the threshold kernel, `activity_us` ClipBank.activity() itself with its cache cleared (index arithmetic on
the host, the pinned staging copy and the allocations included) -- each the median over `repeats` of HIP events around `iters`
back-to-back calls, after 3 warm-up calls.  Bytes are counted, not measured: `*_bytes_unique` counts every banked sample / map value
once and every table and output entry once (what has to come from HBM), `*_bytes_issued` what the kernels ask the memory system for
(overlapping clips re-read their samples, every map value is read for two pairs); `*_roof` = unique bytes / time / 8 TB/s and
`*_issued_roof` the same for the issued bytes (it may pass 1: those reads are served by L2).
`torch_*_us`: for orientation only, the same statistics as torch ops on the same GPU (gathers of 2048 clips at a time, f64 sums),
timed the same way with iters = 1; the torch path is checked against the table to 1e-9 relative before it is timed."""
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

T, S, HPF, ROOF = 16, 224, 8, 8e12
HOP, LENGTH, _ = maavss_amd.calc_hop_size(T, HPF, 30, 16000)
J = HPF * T


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


def torch_stats(bank, frame_start, sample_start, rec, floor_factor):
    """The table in torch ops -> (level, D, energy, peak, n_active, motion_mean, motion_peak)."""
    audio = bank.audio[:bank.n_samples]
    level = torch.stack([(audio[q[1]:q[1] + q[3]].double() ** 2).sum() for q in bank.recordings])
    n_rec = torch.tensor([q[3] for q in bank.recordings], device="cuda", dtype=torch.float64)
    maps = bank.unpacked_maps().double()
    D = (maps[1:] - maps[:-1]).abs().mean(1)
    win = D.unfold(0, T - 1, 1)[frame_start.long()]
    floor_p = (level / n_rec * floor_factor)[rec.long()]
    ar = torch.arange(LENGTH, device="cuda")
    energy, peak, active = [], [], []
    for c0 in range(0, sample_start.numel(), 2048):
        x = audio[sample_start[c0:c0 + 2048, None] + ar]
        sq = x.double() ** 2
        energy.append(sq.sum(1))
        peak.append(x.abs().amax(1))
        active.append(((sq.view(-1, J, HOP).sum(2) / HOP) >= floor_p[c0:c0 + 2048, None]).sum(1))
    return level, D, torch.cat(energy), torch.cat(peak), torch.cat(active), win.mean(1), win.amax(1)


def case(storage, frame_hop, n_rec, n_frames, iters, repeats):
    n_samples = round((n_frames - T) * 16000 / 30) + LENGTH + 1
    bank = maavss_amd.ClipBank(S, T, frame_hop, HPF, HOP, capacity_frames=n_rec * n_frames, capacity_samples=n_rec * n_samples, storage=storage)
    g = torch.Generator(device="cuda").manual_seed(1)
    for _ in range(n_rec):
        bank.add_recording(0.1 * torch.randn(n_samples, generator=g, device="cuda"), maps=torch.rand(n_frames, bank.frame_elems, generator=g, device="cuda"))
    c, r = len(bank), n_rec
    act = bank.activity()
    frame_start, sample_start = bank.check_indices(torch.arange(c))
    rec = bank.clip_recordings()
    chunks = [_lib.query("maavss_bank_level_chunks", q[3]) for q in bank.recordings]
    first = [sum(chunks[:i]) for i in range(r)]
    rec_tab = torch.tensor([[q[1] for q in bank.recordings], [q[3] for q in bank.recordings], first], dtype=torch.int64)
    d_tab, d_sample, d_frame, d_rec = rec_tab.cuda(), sample_start.cuda(), frame_start.cuda(), rec.cuda()
    f64 = [torch.empty(c, device="cuda", dtype=torch.float64) for _ in range(5)]
    peak = torch.empty(c, device="cuda")
    n_bad, n_active = (torch.empty(c, device="cuda", dtype=torch.int32) for _ in range(2))
    partials, level = torch.empty(sum(chunks), device="cuda", dtype=torch.float64), torch.empty(r, device="cuda", dtype=torch.float64)
    D = torch.empty(bank.n_frames - 1, device="cuda", dtype=torch.float64)
    reasons = torch.empty(c, device="cuda", dtype=torch.uint8)
    sp, p, code, factor = _lib.stream_ptr(), _lib.ptr, 1 if storage == "u16" else 0, 1e-4

    def level_fn():
        _lib.call("maavss_bank_recording_level", p(bank.audio), bank.n_samples, p(d_tab), p(rec_tab), r, p(partials), sum(chunks), p(level), sp)

    def motion_fn():
        _lib.call("maavss_bank_frame_motion", p(bank.maps), code, bank.n_frames, bank.frame_elems, p(D), sp)

    def clips_fn():
        _lib.call("maavss_bank_clip_activity", p(bank.audio), bank.n_samples, p(D), bank.n_frames, p(level), p(d_tab), r, p(d_sample), p(d_frame),
                  p(d_rec), p(sample_start), p(frame_start), p(rec), c, T, HPF, HOP, factor, *(p(t) for t in f64), p(peak), p(n_bad), p(n_active), sp)

    def select_fn():
        _lib.call("maavss_bank_clip_select", p(f64[1]), p(f64[2]), p(n_active), p(f64[3]), p(f64[4]), p(peak), p(n_bad), c, 127, -50.0, -20.0,
                  0.5 * J, 1e-3, 0.5, 1.0, p(reasons), sp)

    def activity_fn():
        bank._activity = None
        bank.activity()

    us = dict(level_us=timed(level_fn, iters, repeats), motion_us=timed(motion_fn, iters, repeats), clips_us=timed(clips_fn, iters, repeats),
              select_us=timed(select_fn, iters, repeats), activity_us=timed(activity_fn, iters, repeats))
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(f64, (act[k] for k in ("energy", "rms_db", "rel_db", "motion_mean", "motion_peak"))))
    want = torch_stats(bank, d_frame, d_sample, d_rec, factor)
    got = (level, D, f64[0], peak, n_active, f64[3], f64[4])
    for name, a, b in zip(("level", "D", "energy", "peak", "n_active", "motion_mean", "motion_peak"), got, want):
        assert bool(((a.double() - b.double()).abs() <= 1e-9 * b.double().abs()).all()), f"the torch formulation disagrees on {name}"
    torch_us = timed(lambda: torch_stats(bank, d_frame, d_sample, d_rec, factor), 1, max(3, repeats // 2))
    elem = bank.maps.element_size()
    level_b = 4 * bank.n_samples + 16 * sum(chunks) + 8 * r
    motion_u, motion_i = bank.n_frames * bank.frame_elems * elem + 8 * D.numel(), 2 * D.numel() * bank.frame_elems * elem + 8 * D.numel()
    clips_u = 4 * bank.n_samples + 8 * D.numel() + (16 + 52) * c
    clips_i = 4 * c * LENGTH + 8 * c * (T - 1) + (16 + 52) * c
    total_u, total_i = level_b + motion_u + clips_u, level_b + motion_i + clips_i
    kernels_us = us["level_us"] + us["motion_us"] + us["clips_us"]

    def roof(nbytes, t_us):
        return round(nbytes / (t_us * 1e-6) / ROOF, 3)

    return dict(storage=storage, frame_hop=frame_hop, recordings=r, bank_frames=bank.n_frames, bank_samples=bank.n_samples, clips=c, **us,
                kernels_us=round(kernels_us, 2), torch_us=torch_us, level_bytes=level_b, motion_bytes_unique=motion_u, motion_bytes_issued=motion_i,
                clips_bytes_unique=clips_u, clips_bytes_issued=clips_i, pass_bytes_unique=total_u, pass_bytes_issued=total_i,
                level_roof=roof(level_b, us["level_us"]), motion_roof=roof(motion_u, us["motion_us"]), motion_issued_roof=roof(motion_i, us["motion_us"]),
                clips_roof=roof(clips_u, us["clips_us"]), clips_issued_roof=roof(clips_i, us["clips_us"]), pass_roof=roof(total_u, kernels_us),
                pass_issued_roof=roof(total_i, kernels_us), torch_over_kernels=round(torch_us / kernels_us, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cases = [case(s, fh, a.recordings, a.frames, a.iters, a.repeats) for s in ("f32", "u16") for fh in (2, T)]
    line = json.dumps(dict(bench="clip_select", device=torch.cuda.get_device_name(0), frames=T, framesize=S, samples=LENGTH, segments=J,
                           iters=a.iters, repeats=a.repeats, cases=cases))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
