#!/usr/bin/env python
"""Micro-benchmark of maavss_vit_attn_masks (VideoAttention.attention_masks) on the GPU box, one JSON line:
    python scripts/attn_masks_bench.py [--iters 10] [--reps 7] [--agreement] [--out profiles/attn_masks_bench.json]
512 frames x 6 heads of softmax(randn) CLS attention at 224^2 (n = 784) and 384^2 (n = 2304), three forms each: patch resolution
(uint8), upsampled uint8, upsampled f32.  Kernel time per call = HIP events around `iters` back-to-back calls of the C entry point
after 3 warm-up calls, median of `reps` such windows; the calls of a window rotate over enough output buffers that their footprint
exceeds the 256 MB Infinity Cache, so the stores go to HBM.  Bytes = the att rows read once + the output written; `roof_share` = those
bytes over the time the 8 TB/s HBM roof needs for them.  Comparator on the same GPU: the reference's own lines (video_attention.py:
59-75) batched over all rows with torch ops -- sort, sum, cumsum, argsort, gather, float, interpolate.
--agreement additionally measures how far the 16-bit extractor moves the masks of the fp32 twin ViT (tests/test_attn_masks_gpu.py,
mask_disagreement: threshold 0.6, 224^2, seeds 3, 4, 5, both backbones, f16 and bf16): CPU-twin time, minutes."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from maavss_amd import _lib  # noqa: E402

HBM_ROOF = 8.0e12       # bytes / s
L3_BYTES = 256 << 20


def timed(fn, iters, reps):
    for _ in range(3):
        fn(0)
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(us), min(us), max(us)


def kernel_case(att, side, form, iters, reps):
    f, heads, n = att.shape
    upsample, dtype = form != "patch", torch.float32 if form == "up_f32" else torch.uint8
    elems = f * heads * (side * side if upsample else n)
    out_bytes = elems * (4 if dtype == torch.float32 else 1)
    outs = [torch.empty(elems, device="cuda", dtype=dtype) for _ in range(max(1, -(-2 * L3_BYTES // out_bytes)) if upsample else 1)]
    code, st = int(dtype == torch.float32), _lib.stream_ptr()

    def run(i):
        _lib.call("maavss_vit_attn_masks", att.data_ptr(), outs[i % len(outs)].data_ptr(), code, f, heads, side, side, 8, int(upsample), 0.6,
                  None, st)

    med, lo, hi = timed(run, iters, reps)
    moved = att.numel() * 4 + out_bytes
    return dict(side=side, n=n, frames=f, heads=heads, form=form, kernel_us=round(med, 2), min_us=round(lo, 2), max_us=round(hi, 2),
                bytes=moved, out_buffers=len(outs), tbps=round(moved / med / 1e6, 3), roof_share=round(moved / HBM_ROOF / (med * 1e-6), 4))


def torch_lines(att, side, upsample, as_float):
    """video_attention.py:59-75, every (frame, head) row at once."""
    f, heads, n = att.shape
    val, idx = torch.sort(att, dim=-1)
    val = val / val.sum(-1, keepdim=True)
    th = torch.cumsum(val, -1) > (1 - 0.6)
    th = torch.gather(th, -1, torch.argsort(idx, dim=-1)).view(f, heads, side // 8, side // 8)
    if as_float or upsample:
        th = th.float()
    if upsample:
        th = torch.nn.functional.interpolate(th, scale_factor=8, mode="nearest")
        if not as_float:
            th = th.to(torch.uint8)
    return th


def torch_case(att, side, form, iters, reps):
    med, lo, hi = timed(lambda i: torch_lines(att, side, form != "patch", form == "up_f32"), max(2, iters // 3), reps)
    return dict(side=side, form=form, torch_us=round(med, 1), min_us=round(lo, 1), max_us=round(hi, 1))


def agreement():
    import test_attn_masks_gpu as t
    rows = []
    for arch in ("vit_small", "vit_base"):
        for seed in (3, 4, 5):
            for act in ("f16", "bf16"):
                rows.append(dict(arch=arch, act=act, seed=seed, differing_share=t.mask_disagreement(arch, act, seed)))
                print(rows[-1], flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--agreement", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to time without one"
    kernel, comparator = [], []
    for side in (224, 384):
        n = (side // 8) ** 2
        att = torch.softmax(torch.randn(a.frames, 6, n, generator=torch.Generator().manual_seed(side)), -1).cuda()
        for form in ("patch", "up_u8", "up_f32"):
            kernel.append(kernel_case(att, side, form, a.iters, a.reps))
            print(kernel[-1], flush=True)
        for form in ("patch", "up_u8", "up_f32"):
            comparator.append(torch_case(att, side, form, a.iters, a.reps))
            print(comparator[-1], flush=True)
    res = dict(bench="attn_masks", device=torch.cuda.get_device_name(0), threshold=0.6, iters=a.iters, reps=a.reps, kernel=kernel,
               torch_reference_lines=comparator)
    if a.agreement:
        res["mask_agreement"] = agreement()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
