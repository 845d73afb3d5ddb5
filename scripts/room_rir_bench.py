#!/usr/bin/env python
"""Micro-benchmark of maavss_amd.Reverb.make_room_rirs, one JSON line:
    python scripts/room_rir_bench.py [--iters 5] [--repeats 5] [--out profiles/room_rir_bench.json]
Tables of 64 rooms x 4 sources at K = 4096 and 8192 taps, 16 kHz.  `default`: Reverb.sample_rooms' rooms (3-8 x 3-8 x 2.4-3.5 m) at a
nominal rt60 of 0.3 and of 0.8 s; `small`: 64 copies of one small reflective room (3 x 3 x 2.4 m, beta 0.95, the sources drawn), the
densest image lattice.  `us`: the median over `repeats` of HIP events around `iters` back-to-back Python calls (host checks, the
lattice bounds, output allocation and the pinned staging copy included), after 2 warm-up calls.  `images` and `contributions` are
counted on the host from tests/room_twin.py's enumeration: the images that reach a tap below K and their taps inside [0, K) (an
image whose amplitude is 0 counts: the kernel measures its distance before it knows).  `half_width_us`: the same table with
H = 1, 4 and 8 (2, 8 and 16 taps an image): what the time does when only the work per image changes.  `one_row_us`: a table of ONE
row of the case's first room, i.e. one workgroup per tile with the chip to itself -- the time of the heaviest tile, below which no
table of such rooms can finish.  `make_rirs_us`: Reverb.make_rirs (the decaying-noise table) of the same 256 x K, for orientation."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import maavss_amd  # noqa: E402
import room_twin as tw  # noqa: E402

ROOMS, SOURCES, SR, H = 64, 4, 16000, 8


def timed(fn, iters, repeats):
    for _ in range(2):
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
    return round(statistics.median(us), 1)


_counted = {}


def count(dims, mic, src, k):
    """-> (images that reach a tap in [0, K), their taps inside [0, K)) over all rows, from the twin's enumeration."""
    if (id(dims), k) in _counted:
        return _counted[id(dims), k]
    images = taps = 0
    for r in range(dims.shape[0]):
        for j in range(src.shape[1]):
            _, tau, _ = tw.images(dims[r].tolist(), mic[r].tolist(), src[r, j].tolist(), (1.0,) * 6, k, SR, H)
            k0 = np.floor(tau).astype(np.int64)
            images += int(tau.shape[0])
            taps += int((np.minimum(k0 + H, k - 1) - np.maximum(k0 - H + 1, 0) + 1).sum())
    _counted[id(dims), k] = images, taps
    return images, taps


def case(name, k, geometry, kw, iters, repeats):
    dims, mic, src = geometry
    rv = maavss_amd.Reverb(k, sr=SR)
    us = timed(lambda: rv.make_room_rirs(dims, mic, src, **kw), iters, repeats)
    one = dict(beta=kw["beta"][:1]) if "beta" in kw else dict(rt60=kw["rt60"][:1])
    one_row_us = timed(lambda: rv.make_room_rirs(dims[:1], mic[:1], src[:1, :1], **one), iters, repeats)
    by_h = {str(h): timed(lambda: rv.make_room_rirs(dims, mic, src, half_width=h, **kw), iters, repeats) for h in (1, 4, 8)}
    images, taps = count(dims, mic, src, k)
    res = dict(case=name, taps=k, rows=ROOMS * SOURCES, us=us, images=images, contributions=taps, images_per_s=round(images / (us * 1e-6), 0),
               contributions_per_s=round(taps / (us * 1e-6), 0), one_row_us=one_row_us, half_width_us=by_h)
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sampler = maavss_amd.Reverb(8192, sr=SR)
    dims, mic, src, _ = sampler.sample_rooms(ROOMS, torch.Generator().manual_seed(0), sources=SOURCES)
    small = torch.tensor([[3.0, 3.0, 2.4]], dtype=torch.float64).expand(ROOMS, 3).contiguous()
    _, s_mic, s_src, _ = sampler.sample_rooms(ROOMS, torch.Generator().manual_seed(1), sources=SOURCES, dims=((3.0, 3.0), (3.0, 3.0), (2.4, 2.4)))
    cases, synth = [], {}

    def emit():
        line = json.dumps(dict(bench="room_rir", device=torch.cuda.get_device_name(0), rooms=ROOMS, sources=SOURCES, sr=SR, half_width=H,
                               resolution=32, iters=a.iters, repeats=a.repeats, make_rirs_us=synth, cases=cases))
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    for k in (4096, 8192):
        for rt in (0.3, 0.8):
            cases.append(case(f"default_rt60_{rt}", k, (dims, mic, src), dict(rt60=torch.full((ROOMS,), rt, dtype=torch.float64)), a.iters, a.repeats))
            emit()
        cases.append(case("small_beta_0.95", k, (small, s_mic, s_src), dict(beta=torch.full((ROOMS, 6), 0.95, dtype=torch.float64)), a.iters, a.repeats))
        synth[str(k)] = timed(lambda: maavss_amd.Reverb(k).make_rirs(ROOMS * SOURCES, seed=3), a.iters, a.repeats)
        emit()
    print(emit())


if __name__ == "__main__":
    main()
