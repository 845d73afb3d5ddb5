#!/usr/bin/env python
"""Measurements of the device-resident clip bank (maavss_amd.ClipBank), one JSON line:
    python scripts/clip_bank_bench.py [--iters 20] [--repeats 9] [--steps 20] [--rounds 3] [--out profiles/clip_bank_bench.json]
On one MI355X, alone on the card.  Shapes of bench.py: clips of 16 frames at 224^2 and 8448 samples (hops_per_frame 8, hop 66).

`batch`: B = 32 and 256 clips cut at seeded random positions from a bank of 64 recordings of 64 frames (synthetic maps through
maps=: a gather's time does not depend on the values), both storages.  `attn_us` / `audio_us` time the two C entry points with the
tables and outputs allocated once; each is the median over `repeats` of HIP events around `iters` back-to-back calls, after 3
warm-up calls.  `call_us` is the same around bank.batch(indices, out=..) itself (index arithmetic on the host, the pinned staging
copy and the workspace allocation included) and `call_host_us` the host clock per call of that loop, which ends before the device
does.  `*_bytes` are counted, not measured: every output element written once, every map value of the batch read once by the
clip-maximum pass and once by the gather (2 or 4 bytes), every sample read once; `*_roof` = bytes / time / 8 TB/s.

`add_recording`: frames/s of add_recording(frames=) over `rounds` recordings of 512 frames at 224^2 (the ViT, pass 1 and for u16
the pack), after one warm-up recording, between two device synchronisations on the host clock.

`training`: the bench.py step (AV_Fusion_Model_Frames + TrainStep, B = 32) fed by ClipPipeline(bank=) + submit_clips against the
same step fed by the ViT pipeline, same model object, same box, `rounds` alternating runs of `steps` steps after 3 warm-up steps,
each on the host clock between two device synchronisations; `ratio` = median ViT-fed ms / median bank-fed ms."""
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

T, S, HPF, FFT, ROOF = 16, 224, 8, 512, 8e12
HOP, LENGTH, T_A = maavss_amd.calc_hop_size(T, HPF, 30, 16000)


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


def host_timed(fn, iters, repeats):
    us = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        us.append((time.perf_counter() - t0) * 1e6 / iters)
        torch.cuda.synchronize()
    return round(statistics.median(us), 2)


def batch_case(b, storage, iters, repeats):
    n_rec, n_frames, frame_hop = 64, 64, 4
    n_samples = round((n_frames - T) * 16000 / 30) + LENGTH + 1
    bank = maavss_amd.ClipBank(S, T, frame_hop, HPF, HOP, capacity_frames=n_rec * n_frames, capacity_samples=n_rec * n_samples, storage=storage)
    g = torch.Generator().manual_seed(1)
    for _ in range(n_rec):
        bank.add_recording(torch.randn(n_samples, generator=g).cuda(), maps=torch.rand(n_frames, bank.frame_elems, generator=g).cuda())
    indices = torch.randint(0, len(bank), (b,), generator=g)
    frame_start, sample_start = bank.check_indices(indices)
    frames_d, samples_d = frame_start.cuda(), sample_start.cuda()
    attn = torch.empty(b, 1, T, S, S, device="cuda")
    audio = torch.empty(b, LENGTH, device="cuda")
    rcp = torch.empty(b, device="cuda")
    sp, p, code = _lib.stream_ptr(), _lib.ptr, 1 if storage == "u16" else 0

    def attn_clips():
        _lib.call("maavss_bank_attn_clips", p(bank.maps), code, p(frames_d), b, bank.n_frames, T, S, S, 0, p(rcp), p(attn), sp)

    def audio_clips():
        _lib.call("maavss_bank_audio_clips", p(bank.audio), bank.n_samples, p(samples_d), b, LENGTH, p(audio), LENGTH, sp)

    def call():
        bank.batch(indices, out=(attn, audio))

    attn_bytes = attn.numel() * 4 + 2 * b * T * bank.frame_elems * bank.maps.element_size() + 12 * b
    audio_bytes = 2 * audio.numel() * 4 + 8 * b
    attn_us, audio_us = timed(attn_clips, iters, repeats), timed(audio_clips, iters, repeats)
    return dict(clips=b, storage=storage, bank_clips=len(bank), attn_us=attn_us, audio_us=audio_us, call_us=timed(call, iters, repeats),
                call_host_us=host_timed(call, iters, repeats), attn_bytes=attn_bytes, audio_bytes=audio_bytes,
                attn_roof=round(attn_bytes / (attn_us * 1e-6) / ROOF, 3), audio_roof=round(audio_bytes / (audio_us * 1e-6) / ROOF, 4))


def add_case(va, storage, rounds, frames, audio):
    n = frames.shape[0]
    bank = maavss_amd.ClipBank(S, T, 8, HPF, HOP, capacity_frames=(rounds + 1) * n, capacity_samples=(rounds + 1) * audio.shape[0], storage=storage)
    bank.add_recording(audio, frames=frames, video_attention=va)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(rounds):
        bank.add_recording(audio, frames=frames, video_attention=va)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return bank, dict(storage=storage, frames_per_recording=n, recordings=rounds, frames_per_s=round(rounds * n / dt, 1))


def training_case(va, bank, steps, rounds, b=32):
    stft = maavss_amd.STFT(FFT, HOP, noise_std=0.1, device="cuda")
    n_bins = FFT // 2 + 1
    try:
        model = maavss_amd.AV_Fusion_Model_Frames([b, 2, T_A, n_bins], [b, 1, T, S, S], HPF)
    except ValueError:
        model = maavss_amd.AV_Fusion_Model_Frames([b, 2, T_A, n_bins], [b, 1, T, S, S], HPF, spatial_match="adaptive")
    step_fn = maavss_amd.TrainStep(model.cuda().train(), lr=1e-5, loss_coeff=0.001, num_seq=1)
    g = torch.Generator().manual_seed(2)
    frames = torch.rand(b * T, 3, S, S, generator=g).cuda()
    audio = (0.3 * torch.randn(b, LENGTH, generator=g)).clamp(-1, 1).cuda()
    fed = maavss_amd.ClipPipeline(va, stft, T)
    banked = maavss_amd.ClipPipeline(None, stft, T, bank=bank)
    order = torch.Generator().manual_seed(3)

    def run(pipe, n):
        def submit(i):
            if pipe is fed:
                pipe.submit(frames, audio, seed=i)
            else:
                pipe.submit_clips(torch.randperm(len(bank), generator=order)[:b], seed=i)
        submit(0)
        for i in range(n):
            submit(i + 1)
            x_v, x_stft, y_stft = pipe.get()
            step_fn(x_stft, x_v, y_stft[:, :, (T // 2) * HPF:(T // 2 + 1) * HPF, :], x_v[:, :, T // 2])
            pipe.release()
        pipe.get()                                   # the batch submitted last is not trained on
        pipe.release()

    ms = {"vit": [], "bank": []}
    for _ in range(rounds):
        for name, pipe in (("vit", fed), ("bank", banked)):
            run(pipe, 3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pipe, steps)
            torch.cuda.synchronize()
            ms[name].append(round((time.perf_counter() - t0) * 1e3 / steps, 3))
    fed.drain()
    banked.drain()
    vit, bk = statistics.median(ms["vit"]), statistics.median(ms["bank"])
    return dict(clips=b, steps=steps, vit_fed_ms=ms["vit"], bank_fed_ms=ms["bank"], vit_fed_ms_median=vit, bank_fed_ms_median=bk,
                ratio=round(vit / bk, 2), bank_clips=len(bank), storage=bank.storage)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    batch = [batch_case(b, s, a.iters, a.repeats) for b in (32, 256) for s in ("f32", "u16")]
    va = maavss_amd.VideoAttention(path_to_weights="dino_deitsmall8_pretrain.pth")          # random init when absent
    g = torch.Generator().manual_seed(4)
    n = 512
    frames = torch.rand(n, 3, S, S, generator=g).cuda()
    audio = torch.randn(round((n - T) * 16000 / 30) + LENGTH + 1, generator=g).cuda()
    banks, add = {}, []
    for storage in ("f32", "u16"):
        banks[storage], row = add_case(va, storage, a.rounds, frames, audio)
        add.append(row)
    del frames
    training = [training_case(va, banks[s], a.steps, a.rounds) for s in ("f32", "u16")]
    line = json.dumps(dict(bench="clip_bank", device=torch.cuda.get_device_name(0), frames=T, framesize=S, samples=LENGTH, iters=a.iters,
                           repeats=a.repeats, batch=batch, add_recording=add, training=training))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
