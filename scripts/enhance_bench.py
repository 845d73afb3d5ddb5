#!/usr/bin/env python
"""Whole-recording inference (maavss_amd.Enhancer) on the GPU box, one JSON line:
    python scripts/enhance_bench.py [--seconds 60] [--fps 30] [--size 224] [--fft_len 512] [--hops_per_frame 8] [--num_frames 16]
                                    [--num_seq 4] [--batch 32] [--repeats 3] [--out profiles/enhance_bench.json]
A synthetic recording (seconds * fps frames of size^2, seconds * 16 kHz samples) through the bench model shape (bench.py: batch 32 =
windows_per_launch, 16-frame windows, 224^2 with spatial_match="adaptive", 512-point STFT, a = 8) with seeded weights and the randomly
initialised ViT-S/8, target_offset = num_frames // 2 (bench.py's convention).  HIP events at the Enhancer's stage boundaries split the
call into: the ViT pass (every recording frame once, pass 1 of the map post-process, clip scales), the batched clip STFT, the window
gathers (attention + STFT windows), the eval forwards, the stitches and the inverse STFT.  Best of `repeats` calls after one warm-up
call; the total is the wall time of the call, and the real-time factor is the recording's duration over it."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import maavss_amd  # noqa: E402
from oracle import avse_ref_cpu as orc, stft_ref_cpu as sref, vit_ref_cpu as vref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--fps", type=int, default=30)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--fft_len", type=int, default=512)
    ap.add_argument("--hops_per_frame", type=int, default=8)
    ap.add_argument("--num_frames", type=int, default=16)
    ap.add_argument("--num_seq", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32, help="the model's batch = windows per eval forward")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    sr, n, s, a, w, b = 16000, args.num_frames, args.num_seq, args.hops_per_frame, args.size, args.batch
    hop, _, t_a = maavss_amd.calc_hop_size(n, a, args.fps, sr)
    n_bins = args.fft_len // 2 + 1
    n_frames, n_samples = int(round(args.seconds * args.fps)), int(round(args.seconds * sr))
    shapes = ([b, 2, t_a, n_bins], [b, 1, n, w, w], a)
    try:
        model, spatial = maavss_amd.AV_Fusion_Model_Frames(*shapes), "exact"
        twin = orc.AVFusionFramesRef(*shapes)
    except ValueError:
        model, spatial = maavss_amd.AV_Fusion_Model_Frames(*shapes, spatial_match="adaptive"), "adaptive"
        twin = orc.AVFusionFramesRef(*shapes, spatial_match="adaptive")
    model.load_state_dict(orc.seeded_state_dict(twin, 1234), strict=True)
    model = model.cuda().eval()
    va = maavss_amd.VideoAttention(path_to_weights="dino_deitsmall8_pretrain.pth")       # random init: no network
    stft = maavss_amd.STFT(args.fft_len, hop, normalize_output_fft=True, device="cuda")
    frames = torch.empty(n_frames, 3, w, w, device="cuda")
    for f0 in range(0, n_frames, 256):                                                     # synthetic frames, 256 at a time on the host
        f1 = min(n_frames, f0 + 256)
        frames[f0:f1] = vref.synthetic_frames(f1 - f0, w, 7 + f0).cuda()
    audio = sref.synthetic_audio(1, n_samples, 8)[0].cuda()
    enh = maavss_amd.Enhancer(model, stft, n, s, a, video_attention=va, fps=args.fps, sr=sr, target_offset=n // 2)
    n_clips, _ = enh.tiling(n_samples, n_frames)

    enh(audio, frames=frames)                                                              # warm-up: first launches, allocator
    torch.cuda.synchronize()
    best = None
    for _ in range(args.repeats):
        enh._marks = []
        t0 = time.perf_counter()
        wave, start = enh(audio, frames=frames)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        stages = {}
        for (_, e0), (name, e1) in zip(enh._marks, enh._marks[1:]):
            stages[name] = stages.get(name, 0.0) + e0.elapsed_time(e1)
        if best is None or total < best[0]:
            best = (total, stages)
    enh._marks = None
    total, st = best
    ms = {"vit_pass": st["vit"], "clip_stft": st["stft"], "window_gathers": st["gather"], "eval_forwards": st["forward"],
          "stitch": st["stitch"], "inverse": st["inverse"]}
    res = dict(bench="enhance", device=torch.cuda.get_device_name(0), seconds=args.seconds, fps=args.fps, sr=sr, frames=n_frames,
               samples=n_samples, size=w, fft_len=args.fft_len, hops_per_frame=a, num_frames=n, num_seq=s, windows_per_launch=b,
               spatial_match=spatial, clips=n_clips, windows=n_clips * s, eval_launches=-(-n_clips * s // b),
               output_samples=int(wave.shape[0]), start=start, stage_ms={k: round(v, 3) for k, v in ms.items()},
               total_ms=round(total, 2), stage_sum_ms=round(sum(ms.values()), 2),
               eval_forward_share=round(ms["eval_forwards"] / total, 4), realtime_factor=round(args.seconds * 1e3 / total, 1),
               ms_per_window_forward=round(ms["eval_forwards"] / (n_clips * s), 4), repeats=args.repeats,
               peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
