#!/usr/bin/env python
"""Micro-benchmark of the optimizer extension (csrc/optim.hip) on the real model's flat buffers, one JSON line:
    python scripts/optim_bench.py [--iters 20] [--repeats 3] [--out profiles/optim_bench.json]
The model is bench.py's config 2 (32 clips x 16 frames of 224^2, 512-point STFT, 8 hops per frame): 65 M f32 parameters in one flat
buffer, the gradient of one real TrainStep in the other.  Every figure is the median of HIP events on the stream around `iters`
back-to-back calls, after 3 warm-up calls, in microseconds; the forms alternate with the plain step in one process, three rounds.
  adam_plain_us            FusedAdam.step() with every new keyword off: the launches of the commit before this feature (28 B per parameter)
  adamw_decay_us           weight_decay only                                   (28 B per parameter)
  adamw_decay_ema_us       weight_decay + ema_decay                            (36 B per parameter)
  adamw_decay_ema_skip_us  + skip_nonfinite: the TensorStats norm pass (4 B per parameter more) in front of the step
  adamw_all_clip_us        + max_grad_norm: the same norm pass, now also the clip scale
  adam_clipped_us          the plain kernel with max_grad_norm, for the cost of the norm pass on its own
  swap_us                  maavss_swap_f32 of the parameter buffer and the average (16 B per parameter)
  trainstep_off_us / trainstep_on_us   the whole TrainStep on seeded random inputs of the bench shape, everything off / on, two models
`*_tbs` = the bytes the form moves (parameters x bytes per parameter) over its time, in TB/s."""
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
    return round(statistics.median(us), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--framesize", type=int, default=224)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs the MI355X: nothing here can be measured on a CPU")
    b, t, w, hpf, fft = a.batch, a.frames, a.framesize, 8, 512
    _, _, t_a = maavss_amd.calc_hop_size(t, hpf, 30, 16000)
    n_bins = fft // 2 + 1
    shapes = ([b, 2, t_a, n_bins], [b, 1, t, w, w], hpf)

    def build(**kw):
        torch.manual_seed(1234)
        try:
            model = maavss_amd.AV_Fusion_Model_Frames(*shapes)
        except ValueError:
            model = maavss_amd.AV_Fusion_Model_Frames(*shapes, spatial_match="adaptive")
        return maavss_amd.TrainStep(model.to("cuda").train(), lr=1e-5, loss_coeff=0.001, **kw)

    g = torch.Generator().manual_seed(7)
    x_a = torch.randn(b, 2, t_a, n_bins, generator=g).cuda()
    x_v = torch.rand(b, 1, t, w, w, generator=g).cuda()
    y_a = torch.randn(b, 2, hpf, n_bins, generator=g).cuda()
    y_v = torch.rand(b, 1, w, w, generator=g).cuda()

    plain = build()
    plain(x_a, x_v, y_a, y_v, optimizer_step=False)          # a real gradient in flat.grads, every trained parameter touched
    flat = plain.flat
    runs = plain.opt._runs()
    n_par = sum(min(hi, flat.total) - lo for lo, hi, _, _ in runs)
    res = dict(bench="optim", device=torch.cuda.get_device_name(0), shape=dict(batch=b, frames=t, framesize=w), iters=a.iters,
               repeats=a.repeats, flat_elements=flat.total, stepped_elements=n_par, tensors=len(flat.names), runs=len(runs))

    wd, d, big = 0.01, 0.999, 1e30
    forms = {
        "adam_plain_us": (plain.opt, 28),
        "adamw_decay_us": (maavss_amd.FusedAdam(flat, lr=1e-5, weight_decay=wd), 28),
        "adamw_decay_ema_us": (maavss_amd.FusedAdam(flat, lr=1e-5, weight_decay=wd, ema_decay=d), 36),
        "adamw_decay_ema_skip_us": (maavss_amd.FusedAdam(flat, lr=1e-5, weight_decay=wd, ema_decay=d, skip_nonfinite=True), 40),
        "adamw_all_clip_us": (maavss_amd.FusedAdam(flat, lr=1e-5, weight_decay=wd, ema_decay=d, skip_nonfinite=True, max_grad_norm=big), 40),
        "adam_clipped_us": (maavss_amd.FusedAdam(flat, lr=1e-5, max_grad_norm=big), 32),
    }
    rows = {k: [] for k in forms}
    for _ in range(3):
        for k, (opt, _) in forms.items():
            rows[k].append(timed(opt.step, a.iters, a.repeats))
    for k, (opt, bpp) in forms.items():
        res[k] = round(statistics.median(rows[k]), 2)
        res[k + "_runs"] = rows[k]
        res[k.replace("_us", "_tbs")] = round(n_par * bpp / res[k] / 1e6, 2)
        res[k.replace("_us", "_bytes_per_parameter")] = bpp
    res["decay_over_plain"] = round(res["adamw_decay_us"] / res["adam_plain_us"], 3)
    res["decay_ema_over_plain"] = round(res["adamw_decay_ema_us"] / res["adam_plain_us"], 3)
    res["byte_ratio_ema"] = round(36 / 28, 3)
    res["skipped_steps"] = int(forms["adamw_all_clip_us"][0].skipped_steps.item())

    ema = forms["adamw_decay_ema_us"][0].ema
    sw = [timed(lambda: ops.swap_f32(flat.params, ema), 2 * (a.iters // 2), a.repeats) for _ in range(3)]      # an even count: swapped back
    res["swap_us"], res["swap_us_runs"] = round(statistics.median(sw), 2), sw
    res["swap_tbs"] = round(flat.total * 16 / res["swap_us"] / 1e6, 2)

    # the whole step, two models, alternating
    on = build(weight_decay=wd, ema_decay=d, ema_warmup=True, skip_nonfinite=True, max_grad_norm=big)
    on.opt.schedule = maavss_amd.LRSchedule(1e-5, warmup_steps=100, total_steps=10000, kind="cosine")
    rows = {"trainstep_off_us": [], "trainstep_on_us": []}
    it = max(3, a.iters // 4)
    for _ in range(3):
        rows["trainstep_off_us"].append(timed(lambda: plain(x_a, x_v, y_a, y_v), it, 3, warm=2))
        rows["trainstep_on_us"].append(timed(lambda: on(x_a, x_v, y_a, y_v), it, 3, warm=2))
    for k, v in rows.items():
        res[k] = round(statistics.median(v), 1)
        res[k + "_runs"] = v
    res["trainstep_on_minus_off_us"] = round(res["trainstep_on_us"] - res["trainstep_off_us"], 1)
    res["trainstep_on_skipped_steps"] = int(on.opt.skipped_steps.item())

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
