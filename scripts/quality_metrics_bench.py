#!/usr/bin/env python
"""Micro-benchmark of the quality metrics (csrc/quality_metrics.hip) and of a validation pass, one JSON line:
    python scripts/quality_metrics_bench.py [--iters 50] [--repeats 9] [--out profiles/quality_metrics_bench.json]
Every figure is the median over `repeats` of HIP events on the stream around `iters` back-to-back calls, after 3 warm-up calls, in
microseconds.  `share_of_hbm_roof` = the least time the bytes need at 8 TB/s over the measured time.
  wave      maavss_amd.wave_metrics(est, ref, seg_len=256) at 32 x 8448, 256 x 8448 and 1 x 960 000 samples, and at 4096 x 8448 (a size at
            which the bytes and not the four launches set the time): both arrays read in each of the two passes (2 x 2 x 4 B per sample).
            `workgroups` = chunks per pass: the long row is spread over the device.  A call also allocates its output and workspace and
            asks the library for the workspace size: at the small shapes the figure is the host's time per call, not the kernels'
            (`--kernels-only` under `rocprofv3 --kernel-trace` gives those: profiles/quality_metrics_kernels.txt).
  spectrum  maavss_amd.spectrum_metrics(pred, tgt) at [32, 2, 8, 257] and [256, 2, 128, 257]: two launches, both arrays read once; per
            frequency bin one f64 division and one f64 log10 besides the loads
  validation  Validator.add_clips (forward + metrics, no gradient) beside TrainStep.sliding_window_step (forward, loss, backward, Adam --
            the launches of the commit before this feature: only the window slicing moved into a shared function) on seeded inputs of
            bench.py's shape, num_seq 1, two models of the same weights, alternating
Back-to-back calls on these sizes find their inputs in the 256 MiB Infinity Cache: the shares are those of a warm cache."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maavss_amd  # noqa: E402
from maavss_amd import quality  # noqa: E402

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


def roof(n_bytes, us):
    return dict(bytes=n_bytes, gbs=round(n_bytes / us / 1e3, 1), share_of_hbm_roof=round(n_bytes / (PEAK_HBM_GBS * 1e3) / us, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--framesize", type=int, default=224)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="the metric calls alone, without the validation pass (for a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quality_metrics_bench needs the MI355X: nothing here can be measured on a CPU")
    g = torch.Generator(device="cuda").manual_seed(3)
    res = dict(bench="quality_metrics", device=torch.cuda.get_device_name(0), iters=a.iters, repeats=a.repeats, seg_len=256,
               wave_chunk=quality.wave_chunk(), wave=[], spectrum=[])

    for b, n in ((32, 8448), (256, 8448), (1, 960000), (4096, 8448)):
        ref = 0.3 * torch.randn(b, n, device="cuda", generator=g)
        est = ref + 0.03 * torch.randn(b, n, device="cuda", generator=g)
        us, lo, hi = timed(lambda: maavss_amd.wave_metrics(est, ref, 256), a.iters, a.repeats)
        row = dict(shape=[b, n], us=us, us_min=lo, us_max=hi, launches=4, workgroups=b * len(maavss_amd.plan_wave_chunks(n, 256, quality.wave_chunk())))
        row.update(roof(2 * 2 * 4 * b * n, us))
        res["wave"].append(row)

    for shape in ((32, 2, 8, 257), (256, 2, 128, 257)):
        tgt = torch.randn(*shape, device="cuda", generator=g)
        pred = tgt + 0.1 * torch.randn(*shape, device="cuda", generator=g)
        us, lo, hi = timed(lambda: maavss_amd.spectrum_metrics(pred, tgt), a.iters, a.repeats)
        row = dict(shape=list(shape), us=us, us_min=lo, us_max=hi, launches=2)
        row.update(roof(2 * 4 * pred.numel(), us))
        res["spectrum"].append(row)
        if shape[0] == 256:
            pa, ta = pred.view(256, -1), tgt.view(256, -1)
            us, lo, hi = timed(lambda: quality.sqerr_rows(pa, ta), a.iters, a.repeats)
            row = dict(shape=list(pa.shape), us=us, us_min=lo, us_max=hi, launches=2)
            row.update(roof(2 * 4 * pa.numel(), us))
            res["sqerr_rows"] = row

    if a.kernels_only:
        print(json.dumps(res))
        return

    # a validation pass beside a training step, bench.py's shape
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
        return model.to("cuda")

    gc = torch.Generator().manual_seed(7)
    x_stft = torch.randn(b, 2, t_a, n_bins, generator=gc).cuda()
    y_stft = torch.randn(b, 2, t_a, n_bins, generator=gc).cuda()
    attn = torch.rand(b, 1, t, w, w, generator=gc).cuda()
    step = maavss_amd.TrainStep(build().train(), lr=1e-5, loss_coeff=0.001, num_seq=1)
    val = maavss_amd.Validator(build().eval(), loss_coeff=0.001, num_seq=1)
    rows = {"sliding_window_step_us": [], "validator_add_clips_us": []}
    it = max(3, a.iters // 10)
    for _ in range(3):
        rows["sliding_window_step_us"].append(timed(lambda: step.sliding_window_step(x_stft, y_stft, attn, attn, t, hpf), it, 3, warm=2)[0])
        rows["validator_add_clips_us"].append(timed(lambda: val.add_clips(x_stft, y_stft, attn, attn, t, hpf), it, 3, warm=2)[0])
    v = dict(shape=dict(batch=b, frames=t, framesize=w, fft_len=fft, hops_per_frame=hpf, num_seq=1))
    for k, r in rows.items():
        v[k] = round(statistics.median(r), 1)
        v[k + "_runs"] = r
    v["add_clips_over_step"] = round(v["validator_add_clips_us"] / v["sliding_window_step_us"], 3)
    out = val.result()
    v["val_loss"], v["lsd_db"], v["n_windows"] = out["val_loss"], out["lsd_db"], out["n_windows"]
    res["validation"] = v

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
