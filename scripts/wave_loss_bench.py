#!/usr/bin/env python
"""Micro-benchmark of the waveform loss (csrc/wave_loss.hip), one JSON line:
    python scripts/wave_loss_bench.py [--iters 50] [--repeats 9] [--out profiles/wave_loss_bench.json]
Every figure is the median over `repeats` of HIP events on the stream around `iters` back-to-back calls, after 3 warm-up calls, in
microseconds; the forms of a shape alternate inside every repeat.
  op          WaveformLoss at [32, 2, 32, 129] (the reference's defaults: fft 256, hop 66, 4 windows of 8 hops), [32, 2, 128, 257]
              (fft 512) and [256, 2, 128, 257]: forward only (8 launches for si_sdr, 6 for snr) and with the gradient (2 more: the
              envelope and the adjoint).  `adjoint_us` = with gradient minus forward only, i.e. the envelope and the adjoint launch,
              beside STFT.__call__(want_x=False) on audio of the same B, T, N: the same transform, so the ratio is what the f64 loader
              (two waves, two coefficients and the envelope per sample) costs.  A call also allocates its outputs and workspace: where
              the figure does not grow with the shape it is the host's time per call ("launch_bound").  `gbytes_per_s` counts the
              bytes the kernels must move (pred and tgt in, the frame buffer out and in twice, the waves out and in three times, the
              gradient out) over the time of the call with gradient.
  train_step  TrainStep.sliding_window_step at bench.py's shape with num_seq windows, with wave_loss=WaveformLoss(...) against the
              default, two models of the same weights, alternating; torch.cuda.max_memory_allocated of each (the clip step keeps
              num_seq sets of saved activations alive).
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

ROOF_GBS = 8000.0


def timed_forms(forms, iters, repeats, warm=3):
    """forms: {key: fn} -> {key: (median, min, max)} in us; the forms alternate inside every repeat."""
    for fn in forms.values():
        for _ in range(warm):
            fn()
    us = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: (round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--framesize", type=int, default=224)
    ap.add_argument("--num_seq", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wave_loss_bench needs the MI355X: nothing here can be measured on a CPU")
    g = torch.Generator(device="cuda").manual_seed(3)
    res = dict(bench="wave_loss", device=torch.cuda.get_device_name(0), iters=a.iters, repeats=a.repeats, roof_gbytes_per_s=ROOF_GBS, op=[])
    hop = 66
    for b, t, n in ((32, 32, 256), (32, 128, 512), (256, 128, 512)):
        stft = maavss_amd.STFT(n, hop)
        f = stft.n_bins()
        tgt = 0.3 * torch.randn(b, 2, t, f, device="cuda", generator=g)
        pred = tgt + 0.1 * torch.randn(b, 2, t, f, device="cuda", generator=g)
        audio = 0.1 * torch.randn(b, hop * t, device="cuda", generator=g)
        si, snr = maavss_amd.WaveformLoss(stft, "si_sdr"), maavss_amd.WaveformLoss(stft, "snr")
        forms = {"si_sdr_forward_us": lambda: si(pred, tgt), "si_sdr_with_grad_us": lambda: si(pred, tgt, grad_scale=1.0 / b),
                 "snr_forward_us": lambda: snr(pred, tgt), "snr_with_grad_us": lambda: snr(pred, tgt, grad_scale=1.0 / b),
                 "stft_fwd_us": lambda: stft(audio, want_x=False), "istft_us": lambda: stft.inverse(pred)}
        row = dict(shape=[b, 2, t, f], fft_len=n, hop=hop, samples=hop * (t - 1))
        for k, (med, lo, hi) in timed_forms(forms, a.iters, a.repeats).items():
            row[k], row[k + "_min"], row[k + "_max"] = med, lo, hi
        row["adjoint_us"] = round(row["si_sdr_with_grad_us"] - row["si_sdr_forward_us"], 2)
        row["adjoint_over_stft_fwd"] = round(row["adjoint_us"] / row["stft_fwd_us"], 3)
        planes, frames, waves = b * 2 * t * f * 4, b * t * n * 4, b * hop * (t - 1) * 4
        nbytes = 2 * planes + 4 * frames + 2 * 4 * waves + planes
        row["bytes"] = nbytes
        row["gbytes_per_s"] = round(nbytes / row["si_sdr_with_grad_us"] * 1e-3, 1)
        row["of_roof"] = round(row["gbytes_per_s"] / ROOF_GBS, 4)
        res["op"].append(row)
    small, big = res["op"][1], res["op"][2]
    res["launch_bound"] = bool(big["si_sdr_with_grad_us"] < 4.0 * small["si_sdr_with_grad_us"])      # eight times the work

    b, t, w, hpf, fft, ns = a.batch, a.frames, a.framesize, 8, 512, a.num_seq
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
    x_stft = torch.randn(b, 2, hpf * (t + ns - 1), n_bins, generator=gc).cuda()
    y_stft = torch.randn(b, 2, hpf * (t + ns - 1), n_bins, generator=gc).cuda()
    attn = torch.rand(b, 1, t + ns - 1, w, w, generator=gc).cuda()
    wave = maavss_amd.WaveformLoss(maavss_amd.STFT(fft, hop))
    v = dict(shape=dict(batch=b, frames=t, framesize=w, fft_len=fft, hop=hop, hops_per_frame=hpf, num_seq=ns), clip_stft=[b, 2, hpf * ns, n_bins])
    base = torch.cuda.memory_allocated()
    steps = {}
    for key, kw in (("default", {}), ("wave", dict(wave_loss=wave, wave_weight=0.1))):
        steps[key] = maavss_amd.TrainStep(build(), lr=1e-5, loss_coeff=0.001, num_seq=ns, **kw)
    forms = {k + "_us": (lambda s=s: s.sliding_window_step(x_stft, y_stft, attn, attn, t, hpf)) for k, s in steps.items()}
    for k, (med, lo, hi) in timed_forms(forms, max(3, a.iters // 10), max(3, a.repeats // 3), warm=2).items():
        v[k], v[k + "_min"], v[k + "_max"] = med, lo, hi
    for k, fn in forms.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        v[k[:-3] + "_peak_bytes"] = int(torch.cuda.max_memory_allocated())
    v["resident_before_bytes"] = int(base)
    v["wave_over_default"] = round(v["wave_us"] / v["default_us"], 4)
    v["wave_peak_over_default"] = round(v["wave_peak_bytes"] / v["default_peak_bytes"], 4)
    v["wave_loss_db"] = round(float(steps["wave"].wave["loss"].cpu()), 4)
    res["train_step"] = v

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
