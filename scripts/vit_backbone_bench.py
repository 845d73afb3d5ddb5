"""Extraction rate of the two DINO patch-8 backbones: VideoAttention(architecture=...).attention_frames on 512 frames at 224^2
(one launch group, clip normalisation over 16-frame clips, the deferred range check of the training loop).  Time per call from HIP
events around each call after a warm-up; the median is reported.  Prints one JSON line:

  {"frames": 512, "size": 224, "<arch>": {"ms_per_512_frames", "frames_per_s", "gflop_per_frame", "tflop_per_call", "tflop_per_s",
   "peak_fraction"}, ..., "b_over_s": time ratio (when both ran)}

gflop_per_frame is analytic (2 FLOP per multiply-add): the dense layers, Q K^T and P V of the 11 full blocks, q and k of the last
block and the patch embedding -- 41.6 GFLOP for ViT-S/8 and 145 for ViT-B/8 at 785 tokens.  peak_fraction is against the
2.5 PFLOP/s dense 16-bit MFMA peak of the MI355X."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import maavss_amd  # noqa: E402
from maavss_amd.video_attention import PATCH, VIT_SPECS  # noqa: E402

PEAK = 2.5e15


def gflop_per_frame(arch, size):
    d, _, mlp, depth, _ = VIT_SPECS[arch]
    n = (size // PATCH) ** 2 + 1
    block = 2 * n * (3 * d * d + d * d + 2 * d * mlp) + 2 * 2 * n * n * d
    return ((depth - 1) * block + 2 * n * 2 * d * d + 2 * n * 192 * d) / 1e9


def run(arch, frames, size, warmup, reps):
    va = maavss_amd.VideoAttention(architecture=arch, path_to_weights="/nonexistent.pth")
    g = torch.Generator(device="cuda").manual_seed(0)
    x = (torch.rand(frames, 3, size, size, device="cuda", generator=g) - 0.45) / 0.226
    out = torch.empty(frames, 1, size, size, device="cuda")
    for _ in range(warmup):
        va.attention_frames(x, clip_frames=16, out=out, finite_check="deferred")
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        va.attention_frames(x, clip_frames=16, out=out, finite_check="deferred")
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    va.check_finite()
    ms = statistics.median(times)
    gf = gflop_per_frame(arch, size)
    tflop = gf * frames / 1e3
    return {"ms_per_512_frames": round(ms * 512 / frames, 3), "frames_per_s": round(frames / ms * 1e3, 1), "gflop_per_frame": round(gf, 2),
            "tflop_per_call": round(tflop, 2), "tflop_per_s": round(tflop / ms * 1e3, 1), "peak_fraction": round(tflop * 1e12 / (ms * 1e-3) / PEAK, 4),
            "ms_min": round(min(times), 3), "ms_max": round(max(times), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--arch", choices=["both", *VIT_SPECS], default="both")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    archs = list(VIT_SPECS) if a.arch == "both" else [a.arch]
    res = {"frames": a.frames, "size": a.size, "device": torch.cuda.get_device_name(0)}
    for arch in archs:
        res[arch] = run(arch, a.frames, a.size, a.warmup, a.reps)
    if len(archs) == 2:
        res["b_over_s"] = round(res["vit_base"]["ms_per_512_frames"] / res["vit_small"]["ms_per_512_frames"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
