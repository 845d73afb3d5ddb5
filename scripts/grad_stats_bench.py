#!/usr/bin/env python
"""Micro-benchmark of the gradient statistics (csrc/tensor_stats.hip) on the real model's flat buffers, one JSON line:
    python scripts/grad_stats_bench.py [--iters 20] [--repeats 9] [--out profiles/grad_stats_bench.json]
The model is bench.py's config 2 (32 clips x 16 frames of 224^2, 512-point STFT, 8 hops per frame): 65 M f32 parameters in one flat
buffer, the gradient of one real TrainStep in the other.  Every figure is the median over `repeats` of HIP events on the stream around
`iters` back-to-back calls, after 3 warm-up calls, in microseconds:
  (a) stats_us        pass 1 + finalize with a clip (TensorStats.run(hist=False, max_norm=...)); `share_of_hbm_roof` = the bytes of the
                      buffer once over 8 TB/s, over that time.  Back-to-back calls find most of the 261 MB buffer in the 256 MiB Infinity Cache;
                      (c) and (d) show the pass inside an optimizer step and inside a whole training step.
  (b) stats_hist_us   the same plus the 64-bin histogram pass (a second read of the buffer); hist_us = the difference
  (c) adam_plain_us / adam_clipped_us   FusedAdam.step() without and with max_grad_norm on the same buffers (all parameters touched);
                      the plain path issues exactly the launches of the commit before this feature (same kernel, same arguments)
  (d) trainstep_plain_us / trainstep_clipped_us   the whole TrainStep on seeded random inputs of the bench shape, two models, alternating
  (e) torch_clip_grad_norm_us / torch_histc_us    torch.nn.utils.clip_grad_norm_ and torch.histc(bins=64) per tensor over the same
                      views, as torch ops on the same GPU (for orientation: host clock around the calls, ended by a synchronise)"""
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

PEAK_HBM_GBS = 8000.0


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


def host_timed(fn, repeats, warm=1):
    for _ in range(warm):
        fn()
    us = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(us), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--framesize", type=int, default=224)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grad_stats_bench needs the MI355X: nothing here can be measured on a CPU")
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
    names = [n for r in plain.opt._runs() for n in r[3]]
    norm_ref = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(flat.grad_views[n].double()) for n in names])).item()
    n_bytes = 4 * sum(flat.tensors[n].numel() for n in flat.names)

    res = dict(bench="grad_stats", device=torch.cuda.get_device_name(0), shape=dict(batch=b, frames=t, framesize=w), iters=a.iters,
               repeats=a.repeats, flat_elements=flat.total, tensors=len(flat.names), buffer_bytes=n_bytes, grad_norm=norm_ref)

    stats = maavss_amd.TensorStats(flat, bins=64)
    res["chunks"] = stats.n_chunks
    # (a), (b)
    res["stats_us"], res["stats_us_min"], res["stats_us_max"] = timed(
        lambda: stats.run(flat.grads, names=names, hist=False, max_norm=0.5 * norm_ref), a.iters, a.repeats)
    res["share_of_hbm_roof"] = round(n_bytes / (PEAK_HBM_GBS * 1e3) / res["stats_us"], 3)
    res["stats_gbs"] = round(n_bytes / res["stats_us"] / 1e3, 1)
    got = stats.norm.item()
    res["norm_rel_err_vs_torch_f64"] = abs(got - norm_ref) / norm_ref
    res["stats_hist_us"], _, _ = timed(lambda: stats.run(flat.grads, names=names, hist=True, max_norm=0.5 * norm_ref), a.iters, a.repeats)
    res["hist_us"] = round(res["stats_hist_us"] - res["stats_us"], 2)
    res["stats_hist_params_us"], _, _ = timed(lambda: stats.run(flat.params, hist=True), a.iters, a.repeats)

    # (c) the optimizer step alone, alternating plain / clipped on the same buffers (moments and parameters move: 28 B per parameter either way)
    opt_c = maavss_amd.FusedAdam(flat, lr=1e-5, max_grad_norm=0.5 * norm_ref)
    rows = {"adam_plain_us": [], "adam_clipped_us": []}
    for _ in range(3):
        rows["adam_plain_us"].append(timed(plain.opt.step, a.iters, 3)[0])
        rows["adam_clipped_us"].append(timed(opt_c.step, a.iters, 3)[0])
    for k, v in rows.items():
        res[k] = round(statistics.median(v), 2)
        res[k + "_runs"] = v
    res["adam_clipped_over_plain"] = round(res["adam_clipped_us"] / res["adam_plain_us"], 3)
    res["clip_scale"] = opt_c.clip_scale.item()

    # (e) torch on the same views (clip_grad_norm_ with a bound far above the norm multiplies the gradients by 1: the values stay)
    params = [flat.tensors[n] for n in names]
    res["torch_clip_grad_norm_us"] = host_timed(lambda: torch.nn.utils.clip_grad_norm_(params, 1e30), 5)
    res["torch_histc_us"] = host_timed(lambda: [torch.histc(flat.grad_views[n].flatten(), bins=64) for n in flat.names], 3)
    watch = maavss_amd.ModelWatch(plain, log_freq=1, bins=64)
    res["model_watch_after_step_us"] = host_timed(watch.after_step, 3)          # both buffers, histograms, the copy and the host dicts

    # (d) the whole step, two models, alternating
    clipped = build(max_grad_norm=0.5 * norm_ref)
    rows = {"trainstep_plain_us": [], "trainstep_clipped_us": []}
    it = max(3, a.iters // 4)
    for _ in range(3):
        rows["trainstep_plain_us"].append(timed(lambda: plain(x_a, x_v, y_a, y_v), it, 3, warm=2)[0])
        rows["trainstep_clipped_us"].append(timed(lambda: clipped(x_a, x_v, y_a, y_v), it, 3, warm=2)[0])
    for k, v in rows.items():
        res[k] = round(statistics.median(v), 1)
        res[k + "_runs"] = v
    res["trainstep_clipped_minus_plain_us"] = round(res["trainstep_clipped_us"] - res["trainstep_plain_us"], 1)

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
