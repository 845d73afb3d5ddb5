#!/usr/bin/env python
"""Measures what the gates of tests/test_spectral_loss_gpu.py are derived from, one JSON line:
    python scripts/spectral_loss_parity.py [--out profiles/spectral_loss_parity.json]
Over every case of tests/spectral_loss_twin.py (shapes x parameters x data kinds), maavss_amd.SpectralLoss on the GPU against the float64
twin:
  grad_excess   the largest (|got - twin| - ulp_f32 / 2) / (2^-53 A) over the finite gradient elements   -> K_GRAD
  sum_excess    the largest (|S_gpu - S_twin| - (T F - 1) 2^-53 S) / (2^-53 Bsum) over the finite row sums   -> K_SUM
  identical     the smallest share of finite gradient elements that carry the bits of the twin rounded once to f32
  train_rel_l2  TrainStep(audio_loss=SpectralLoss(1, 1)) against the default TrainStep on the avse_S golden shape (precise, deterministic):
                the largest relative L2 over the gradient tensors   -> TRAIN_REL_L2
A gate is eight times its measurement, rounded up to a power of ten; the twin file holds the gates and their caps.  Where nothing left
the term in front of a K the gate is 10 (ten f64 roundings of the no-cancellation magnitude: room for another libm's pow), and the
gradient gate of the training step is at least 1e-7 (one f32 rounding)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import maavss_amd  # noqa: E402
import spectral_loss_twin as tw  # noqa: E402


def gate(measured, floor):
    return max(floor, tw.round_up_to_power_of_ten(8.0 * measured)) if measured > 0.0 else floor


def train_rel_l2():
    from oracle import avse_ref_cpu as orc
    z = np.load(os.path.join(ROOT, "tests", "golden", "avse_S.npz"), allow_pickle=False)
    m = {k[5:]: z[k].item() for k in z.files if k.startswith("meta_")}
    n_bins, t_a = m["fft_len"] // 2 + 1, m["hops_per_frame"] * m["frames"]
    shapes = ([m["batch"], 2, t_a, n_bins], [m["batch"], 1, m["frames"], m["width"], m["width"]], m["hops_per_frame"])
    batch = [x.cuda() for x in orc.synthetic_batch(m["batch"], m["frames"], m["width"], t_a, n_bins, m["hops_per_frame"], m["seed"] + 1)]
    prev = maavss_amd.set_deterministic(True)
    steps = []
    for audio_loss in (None, maavss_amd.SpectralLoss(1.0, 1.0)):
        net = maavss_amd.AV_Fusion_Model_Frames(*shapes, precise=True)
        net.load_state_dict(orc.seeded_state_dict(orc.AVFusionFramesRef(*shapes), m["seed"]), strict=True)
        steps.append(maavss_amd.TrainStep(net.to("cuda").train(), lr=m["lr"], loss_coeff=m["loss_coeff"], audio_loss=audio_loss))
        steps[-1](*batch, optimizer_step=False)
    maavss_amd.set_deterministic(prev)
    rel = {n: float((steps[1].flat.grad_views[n].double() - g.double()).norm() / g.double().norm()) for n, g in steps[0].flat.grad_views.items()}
    worst = max(rel, key=rel.get)
    return dict(largest=rel[worst], tensor=worst, losses_default=steps[0].losses.cpu().tolist(), losses_compress1_mix1=steps[1].losses.cpu().tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spectral_loss_parity needs the MI355X: the kernel is what is measured")
    worst = dict(grad_excess=(-np.inf, None), sum_excess=(-np.inf, None), identical=(1.0, None))
    elements = 0
    for shape in tw.SHAPES:
        for params in tw.PARAMS:
            loss = maavss_amd.SpectralLoss(*params)
            for kind in tw.KINDS:
                pred, tgt = tw.make_case(shape, kind)
                r = tw.loss_and_grad(pred, tgt, *params, grad_scale=1.0 / pred.size)
                res = loss(torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda(), grad_scale=1.0 / pred.size)
                got, rows = res["grad"].cpu().numpy(), res["rows"].cpu().numpy()
                case = [list(shape), list(params), kind]
                ex = float(tw.grad_excess(got, r["grad"], r["A"]).max())
                sx = float(tw.sum_excess(rows, r["rows"], r["Bsum"], shape[1] * shape[2]).max())
                fin = np.isfinite(r["grad"])
                with np.errstate(all="ignore"):
                    same = (got.view(np.uint32) == r["grad"].astype(np.float32).view(np.uint32))[fin]
                elements += int(fin.sum())
                if ex > worst["grad_excess"][0]:
                    worst["grad_excess"] = (ex, case)
                if sx > worst["sum_excess"][0]:
                    worst["sum_excess"] = (sx, case)
                if same.size and same.mean() < worst["identical"][0]:
                    worst["identical"] = (float(same.mean()), case)
    res = dict(bench="spectral_loss_parity", device=torch.cuda.get_device_name(0), cases=len(tw.SHAPES) * len(tw.PARAMS) * len(tw.KINDS),
               finite_gradient_elements=elements)
    for k, (v, case) in worst.items():
        res[k] = dict(value=None if v == -np.inf else v, case=case)       # None: no element left the term in front of the K
    ge, se = max(worst["grad_excess"][0], 0.0), max(worst["sum_excess"][0], 0.0)
    res["train_rel_l2"] = train_rel_l2()
    res["gates"] = dict(K_GRAD=gate(ge, 1e1), K_SUM=gate(se, 1e1), K_CAP=tw.K_CAP, TRAIN_REL_L2=gate(res["train_rel_l2"]["largest"], 1e-7),
                        REL_L2_CAP=tw.REL_L2_CAP, in_twin=dict(K_GRAD=tw.K_GRAD, K_SUM=tw.K_SUM, TRAIN_REL_L2=tw.TRAIN_REL_L2))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
