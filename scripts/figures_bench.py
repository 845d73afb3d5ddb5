#!/usr/bin/env python
"""Micro-benchmark of the callback images (csrc/figures.hip), one JSON line:
    python scripts/figures_bench.py [--iters 20] [--repeats 9] [--matplotlib] [--out profiles/figures_bench.json]
The bench shape: fft 512 (257 bins), hops_per_frame 8, num_seq 4 (32 STFT frames, 2046 samples of audio at hop 66), 224 x 224 attention
and video frames.  Every figure is the median over `repeats` of HIP events on the stream around `iters` back-to-back calls, after 3
warm-up calls, in microseconds: one CallbackFigures call with a video, and each of its parts alone.  A call also allocates its outputs,
so where the device work is a few microseconds the figure is the host's time per call, not the kernels'.  `launches` counts kernel
launches: entry-point calls seen by the binding times the launches each makes (include/maavss.h), plus torch's own copy kernels
(torch.stack and .contiguous() in front of the inverse STFT), which are listed as torch_copies.
--matplotlib: for orientation only, the host time of the reference's six figures (utilities.stft_ae_image_callback,
plot_waveform_specgram twice, video_frames_image: the same matplotlib calls, restated here) from host arrays, median of 3, with the
threads the environment gives.  No speed gate is set."""
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

LAUNCHES = {"maavss_viridis_range": 1, "maavss_viridis_image": 1, "maavss_specgram": 1, "maavss_filmstrip": 2, "maavss_istft": 2}


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
    return dict(us=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2))


def count_calls(fn):
    names, real = [], _lib.lib().call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    _lib.lib().call = spy
    try:
        fn()
    finally:
        _lib.lib().call = real
    return names


def matplotlib_figures(y, yh, waves, a, ah, v):
    """The reference's six figures from host arrays, drawn (fig.canvas.draw()) as the reference draws them."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig = plt.figure(figsize=(6, 5))
    for k, p in enumerate((y[0], y[1], yh[0], yh[1])):
        plt.subplot(1, 4, k + 1)
        plt.axis("off")
        plt.imshow(p.T)
    fig.canvas.draw()
    plt.close()
    for w in waves:
        for mode in ("magnitude", "phase"):
            fig, ax = plt.subplots(1, 1)
            ax.specgram(w, mode=mode, Fs=16000)
            fig.canvas.draw()
            plt.close()
    fig = plt.figure()
    for k, (img, kw) in enumerate(((v, {}), (a, dict(vmin=-1, vmax=1)), (ah, dict(vmin=-1, vmax=1)))):
        plt.subplot(3, 1, k + 1)
        plt.axis("off")
        plt.imshow(img, **kw)
    fig.canvas.draw()
    plt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--matplotlib", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("figures_bench needs the MI355X: nothing here can be measured on a CPU")
    fft, hpf, ns, w, b = 512, 8, 4, 224, 4
    nf = 8
    t_tot = nf + ns - 1
    hop, length, _ = maavss_amd.calc_hop_size(t_tot, hpf, 30, 16000)
    stft = maavss_amd.STFT(fft, hop, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    audio = (0.3 * torch.randn(b, length, device="cuda", generator=g)).clamp(-1, 1)
    _, y_stft = stft(audio, seed=1)
    out_stft = y_stft[:, :, hpf * ((ns - 1) // 2):][:, :, :hpf * ns] + 0.05 * torch.randn(b, 2, hpf * ns, fft // 2 + 1, device="cuda", generator=g)
    attn = torch.rand(b, 1, t_tot, w, w, device="cuda", generator=g)
    out_attn = torch.rand(b, 1, ns, w, w, device="cuda", generator=g)
    video = torch.rand(b, 3, t_tot, w, w, device="cuda", generator=g)
    figures = maavss_amd.CallbackFigures(stft)
    mid = (ns - 1) // 2
    y, yh = y_stft[0, :, mid * hpf:(mid + ns) * hpf], out_stft[0]
    at, ath, vid = attn[0, :, mid:mid + ns], out_attn[0], video[0, :, mid:mid + ns]
    waves = stft.inverse(torch.stack((y, yh)))
    parts = {"callback_figures": lambda: figures(y_stft, out_stft, attn, out_attn, video=video),
             "stft_panels": lambda: maavss_amd.stft_panels(y, yh),
             "inverse_stft_both": lambda: stft.inverse(torch.stack((y, yh))),
             "specgram_images_both": lambda: maavss_amd.specgram_images(waves),
             "specgram_planes_both": lambda: maavss_amd.specgram_planes(waves),
             "filmstrip_image": lambda: maavss_amd.filmstrip_image(at, ath, vid),
             "filmstrip_image_no_video": lambda: maavss_amd.filmstrip_image(at, ath)}
    res = dict(bench="figures", device=torch.cuda.get_device_name(0), iters=a.iters, repeats=a.repeats,
               shape=dict(fft=fft, bins=fft // 2 + 1, stft_frames=hpf * ns, num_seq=ns, frame=[w, w], samples=int(waves.shape[1]),
                          specgram_segments=int(maavss_amd.specgram_planes(waves)[0].shape[2])), rows=[])
    for name, fn in parts.items():
        names = count_calls(fn)
        row = dict(part=name, **timed(fn, a.iters, a.repeats), entry_point_calls=len(names), launches=sum(LAUNCHES[n] for n in names),
                   torch_copies=2 if name in ("callback_figures", "inverse_stft_both") else 0)
        res["rows"].append(row)
    if a.matplotlib:
        try:
            host = [t.cpu().numpy() for t in (y, yh, waves, at, ath, vid)]
            strip = [host[3][0].transpose(1, 0, 2).reshape(w, -1), host[4][0].transpose(1, 0, 2).reshape(w, -1),
                     host[5].transpose(2, 1, 3, 0).reshape(w, -1, 3)]
            ms = []
            for _ in range(4):
                t0 = time.perf_counter()
                matplotlib_figures(host[0], host[1], host[2], *strip[:2], strip[2])
                ms.append((time.perf_counter() - t0) * 1e3)
            res["matplotlib_six_figures_host_ms"] = round(statistics.median(ms[1:]), 1)
            res["matplotlib_threads"] = torch.get_num_threads()
        except ImportError as e:
            res["matplotlib_six_figures_host_ms"] = None
            res["matplotlib_note"] = f"matplotlib does not import on this machine: {e}"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
