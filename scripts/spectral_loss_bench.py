#!/usr/bin/env python
"""Micro-benchmark of the power-law compressed spectral loss (csrc/spectral_loss.hip), one JSON line:
    python scripts/spectral_loss_bench.py [--iters 50] [--repeats 9] [--out profiles/spectral_loss_bench.json]
Every figure is the median over `repeats` of HIP events on the stream around `iters` back-to-back calls, after 3 warm-up calls, in
microseconds.
  pair        ops.spectral_loss_pair (loss and both gradients; four launches) at [32, 2, 8, 257] and [256, 2, 128, 257] with attention
              operands [B, 1, 224, 224], beside ops.mse_pair on the same operands in the same run (three launches), and the forward-only
              form (want_grads=False).  A call also allocates its outputs and workspace: at the small shape the figure is the host's time
              per call.  `pow_per_us` = the four f64 pows per bin over the time of the pair call minus mse_pair's (the attention term and the
              launches are in both).
  train_step  TrainStep.sliding_window_step at bench.py's shape (num_seq 1) with audio_loss=SpectralLoss() against the default, two models
              of the same weights, alternating
No speed gate is derived from this."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maavss_amd  # noqa: E402
from maavss_amd import ops  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--framesize", type=int, default=224)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spectral_loss_bench needs the MI355X: nothing here can be measured on a CPU")
    g = torch.Generator(device="cuda").manual_seed(3)
    loss = maavss_amd.SpectralLoss()
    res = dict(bench="spectral_loss", device=torch.cuda.get_device_name(0), iters=a.iters, repeats=a.repeats,
               loss=dict(compress=loss.compress, mix=loss.mix, eps=loss.eps), pair=[])
    for shape in ((32, 2, 8, 257), (256, 2, 128, 257)):
        tgt = 0.3 * torch.randn(*shape, device="cuda", generator=g)
        pred = tgt + 0.1 * torch.randn(*shape, device="cuda", generator=g)
        v_tgt = torch.rand(shape[0], 1, 224, 224, device="cuda", generator=g)
        v_pred = torch.rand(shape[0], 1, 224, 224, device="cuda", generator=g)
        row = dict(shape=list(shape), attention_shape=list(v_pred.shape), bins=pred.numel() // 2)
        for key, fn in (("spectral_loss_pair_us", lambda: ops.spectral_loss_pair(pred, tgt, v_pred, v_tgt, 0.001, loss)),
                        ("mse_pair_us", lambda: ops.mse_pair(pred, tgt, v_pred, v_tgt, 0.001)),
                        ("spectral_loss_pair_forward_only_us", lambda: ops.spectral_loss_pair(pred, tgt, v_pred, v_tgt, 0.001, loss, want_grads=False)),
                        ("mse_pair_forward_only_us", lambda: ops.mse_pair(pred, tgt, v_pred, v_tgt, 0.001, want_grads=False))):
            row[key], row[key + "_min"], row[key + "_max"] = timed(fn, a.iters, a.repeats)
        extra = row["spectral_loss_pair_us"] - row["mse_pair_us"]
        row["over_mse_pair_us"] = round(extra, 2)
        row["pow_per_us"] = round(4 * row["bins"] / extra, 1) if extra > 0 else None
        res["pair"].append(row)

    b, t, w, hpf, fft = a.batch, a.frames, a.framesize, 8, 512
    _, _, t_a = maavss_amd.calc_hop_size(t, hpf, 30, 16000)
    n_bins = fft // 2 + 1
    shapes = ([b, 2, t_a, n_bins], [b, 1, t, w, w], hpf)

    def build():
        torch.manual_seed(1234)
        try:
            model = maavss_amd.AV_Fusion_Model_Frames(*shapes)
        except ValueError:
            model = maavss_amd.AV_Fusion_Model_Frames(*shapes, spatial_match="adaptive")
        return model.to("cuda").train()

    gc = torch.Generator().manual_seed(7)
    x_stft = torch.randn(b, 2, t_a, n_bins, generator=gc).cuda()
    y_stft = torch.randn(b, 2, t_a, n_bins, generator=gc).cuda()
    attn = torch.rand(b, 1, t, w, w, generator=gc).cuda()
    steps = {"default_us": maavss_amd.TrainStep(build(), lr=1e-5, loss_coeff=0.001, num_seq=1),
             "spectral_us": maavss_amd.TrainStep(build(), lr=1e-5, loss_coeff=0.001, num_seq=1, audio_loss=loss)}
    runs = {k: [] for k in steps}
    it = max(3, a.iters // 10)
    for _ in range(3):
        for k, step in steps.items():
            runs[k].append(timed(lambda: step.sliding_window_step(x_stft, y_stft, attn, attn, t, hpf), it, 3, warm=2)[0])
    v = dict(shape=dict(batch=b, frames=t, framesize=w, fft_len=fft, hops_per_frame=hpf, num_seq=1), audio_output=[b, 2, hpf, n_bins])
    for k, r in runs.items():
        v[k] = round(statistics.median(r), 1)
        v[k + "_runs"] = r
    v["spectral_over_default"] = round(v["spectral_us"] / v["default_us"], 4)
    res["train_step"] = v

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
