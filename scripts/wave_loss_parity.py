#!/usr/bin/env python
"""Measures K_WGRAD of tests/wave_loss_twin.py on the GPU, one JSON line:
    python scripts/wave_loss_parity.py [--out profiles/wave_loss_parity.json]
For every shape, kind and finite input of the twin's case list, per row: ||G - G_twin||_2 / (2^-24 (1 + sqrt(Sxx / (E + eps))) ||G_twin||_2),
G = WaveformLoss's gradient, G_twin = the float64 end-to-end twin's.  The gate of tests/test_wave_loss_gpu.py is eight times the largest
ratio, rounded up to a power of ten, capped at K_CAP."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import maavss_amd  # noqa: E402
import wave_loss_twin as tw  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wave_loss_parity needs the MI355X")
    cases, worst = [], 0.0
    for shape in tw.SHAPES:
        b, _, n, hop, trimmed, normalized = shape
        stft = maavss_amd.STFT(n, hop, normalized=normalized, trim_stft_end=trimmed)
        for kind in tw.KINDS:
            loss = maavss_amd.WaveformLoss(stft, kind=kind, eps=tw.EPS)
            for inp in tw.FINITE_INPUTS:
                pred, tgt = tw.make_case(shape, inp)
                r = tw.loss_and_grad(pred, tgt, shape, kind, tw.EPS, grad_scale=1.0 / b)
                got = loss(torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda(), grad_scale=1.0 / b)
                ratios = tw.grad_ratios(got["grad"].cpu().numpy(), r, tw.EPS)
                cases.append(dict(shape=list(shape), kind=kind, input=inp, ratio=max(ratios), loss_db=[round(float(v), 4) for v in r["rows"][:, 0]]))
                worst = max(worst, max(ratios))
    gate = min(tw.K_CAP, tw.round_up_to_power_of_ten(8.0 * worst))
    res = dict(parity="wave_loss", device=torch.cuda.get_device_name(0), eps=tw.EPS, k_wgrad_measured=worst, k_wgrad_gate=gate, k_cap=tw.K_CAP,
               in_twin=dict(K_WGRAD=tw.K_WGRAD, K_WGRAD_MEASURED=tw.K_WGRAD_MEASURED), cases=cases)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
