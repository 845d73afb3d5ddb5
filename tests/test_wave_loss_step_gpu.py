"""TrainStep(wave_loss=..., wave_weight=...) on the avse_S golden shape with three windows: sliding_window_step with the clip-level
waveform term against the plain step and against the same step driven by hand."""
import os

import numpy as np
import pytest
import torch

import maavss_amd
from maavss_amd import ops
from maavss_amd.trainer import FlatParams, sliding_windows

pytestmark = pytest.mark.gpu

S = 3
HOP = 66


@pytest.fixture(scope="module")
def small(golden_dir):
    from oracle import avse_ref_cpu as orc
    z = np.load(os.path.join(golden_dir, "avse_S.npz"), allow_pickle=False)
    m = {k[5:]: z[k].item() for k in z.files if k.startswith("meta_")}
    n_bins, t_a = m["fft_len"] // 2 + 1, m["hops_per_frame"] * m["frames"]
    shapes = ([m["batch"], 2, t_a, n_bins], [m["batch"], 1, m["frames"], m["width"], m["width"]], m["hops_per_frame"])

    def model(train):
        net = maavss_amd.AV_Fusion_Model_Frames(*shapes, precise=True)
        net.load_state_dict(orc.seeded_state_dict(orc.AVFusionFramesRef(*shapes), m["seed"]), strict=True)
        return net.to("cuda").train(train)

    x_a, x_v, y_a, y_v = (x.cuda() for x in orc.synthetic_batch(m["batch"], m["frames"], m["width"], t_a, n_bins, m["hops_per_frame"], m["seed"] + 1))
    hpf, frames = m["hops_per_frame"], m["frames"]
    g = torch.Generator().manual_seed(11)
    clip = dict(a=torch.cat([x_a, x_a[:, :, :hpf * (S - 1)]], dim=2).contiguous(),
                y=(0.3 * torch.randn(m["batch"], 2, hpf * (frames + S - 1), n_bins, generator=g)).cuda(),      # every window its own target
                v=torch.cat([x_v, x_v[:, :, :S - 1]], dim=2).contiguous())
    prev = maavss_amd.set_deterministic(True)
    yield dict(m=m, model=model, clip=clip, stft=maavss_amd.STFT(m["fft_len"], HOP))
    maavss_amd.set_deterministic(prev)


def _step(small, **kw):
    m = small["m"]
    return maavss_amd.TrainStep(small["model"](True), lr=m["lr"], loss_coeff=m["loss_coeff"], num_seq=S, **kw)


def _run(step, small, **kw):
    c, m = small["clip"], small["m"]
    return step.sliding_window_step(c["a"], c["y"], c["v"], c["v"], m["frames"], m["hops_per_frame"], **kw)


def _bn_state(model):
    return {k: v.clone() for k, v in model.named_buffers()}


def test_weight_zero_is_the_plain_step_and_reports_the_loss(small):
    m, hpf = small["m"], small["m"]["hops_per_frame"]
    loss = maavss_amd.WaveformLoss(small["stft"])
    plain, waved = _step(small), _step(small, wave_loss=loss, wave_weight=0.0)
    l0 = _run(plain, small)
    l1, out_a, out_v = _run(waved, small, collect=True)
    assert plain.flat.grads.abs().max().item() > 0
    assert torch.equal(waved.flat.grads, plain.flat.grads), "deferring the backward passes changes nothing"
    assert torch.equal(l0, l1) and torch.equal(waved.losses, plain.losses)
    assert torch.equal(waved.flat.params, plain.flat.params)
    bn0, bn1 = _bn_state(plain.model), _bn_state(waved.model)
    assert bn0.keys() == bn1.keys() and len(bn0) > 0 and all(torch.equal(bn0[k], bn1[k]) for k in bn0)
    # collect=True returns the stitched outputs, and the reported rows are the op's on them
    _, ref_a, ref_v = _run(_step(small), small, collect=True)
    assert out_a.shape == (m["batch"], 2, hpf * S, m["fft_len"] // 2 + 1) and torch.equal(out_a, ref_a) and torch.equal(out_v, ref_v)
    mid = (S - 1) // 2
    want = loss(out_a, small["clip"]["y"][:, :, hpf * mid:hpf * (mid + S)])
    assert set(waved.wave) == {"rows", "loss"} and waved.wave["rows"].dtype == torch.float64 and waved.wave["rows"].shape == (m["batch"], 5)
    assert torch.equal(waved.wave["rows"], want["rows"]) and torch.equal(waved.wave["loss"], want["loss"])
    assert torch.isfinite(waved.wave["rows"]).all()


@pytest.mark.parametrize("audio_loss", [None, "spectral"])
@pytest.mark.parametrize("kind", ["si_sdr", "snr"])
def test_the_step_is_the_windows_driven_by_hand(small, kind, audio_loss):
    m, c = small["m"], small["clip"]
    hpf, frames, coeff, b = m["hops_per_frame"], m["frames"], m["loss_coeff"], m["batch"]
    a_loss = maavss_amd.SpectralLoss() if audio_loss else None
    loss = maavss_amd.WaveformLoss(small["stft"], kind=kind)
    step = _step(small, wave_loss=loss, wave_weight=0.5, audio_loss=a_loss)
    got = _run(step, small)
    by_hand = small["model"](True)
    flat = FlatParams(by_hand)
    need = {n: bool(p.requires_grad) for n, p in by_hand.named_parameters()}
    saved, outs, d_as, d_vs = [], [], [], []
    for j, xa, xv, ya, yv in sliding_windows(c["a"], c["y"], c["v"], c["v"], frames, hpf, S):
        (a, v, _), sv = by_hand._engine_forward(xa, xv, train=True)
        if a_loss is None:
            losses, d_a, d_v = ops.mse_pair(a, ya.contiguous(), v, yv.contiguous(), coeff, num_seq=S)
        else:
            losses, d_a, d_v, _ = ops.spectral_loss_pair(a, ya.contiguous(), v, yv.contiguous(), coeff, a_loss, num_seq=S)
        saved.append(sv), outs.append(a), d_as.append(d_a), d_vs.append(d_v)
    mid = (S - 1) // 2
    res = loss(torch.cat(outs, dim=2), c["y"][:, :, hpf * mid:hpf * (mid + S)], grad_scale=0.5 / b)
    assert res["grad"].abs().max().item() > 0
    for j in range(S):
        d_a = d_as[j] + res["grad"][:, :, hpf * j:hpf * (j + 1)]
        by_hand._engine_backward(saved[j], d_a.contiguous(), d_vs[j], None, need, grads=flat.grad_views, accumulate=j > 0)
    assert torch.equal(step.flat.grads, flat.grads)
    assert torch.equal(got, losses) and torch.equal(step.losses, losses)
    assert torch.equal(step.wave["rows"], res["rows"]) and torch.equal(step.wave["loss"], res["loss"])
    # the wave term is in the gradient: the step without it differs
    plain = _step(small, audio_loss=a_loss)
    _run(plain, small)
    assert not torch.equal(plain.flat.grads, step.flat.grads)


def test_call_refuses_and_the_step_never_synchronises(small):
    c, m = small["clip"], small["m"]
    hpf, frames = m["hops_per_frame"], m["frames"]
    step = _step(small, wave_loss=maavss_amd.WaveformLoss(small["stft"]), wave_weight=0.1)
    with pytest.raises(ValueError, match="sliding_window_step"):
        step(c["a"][:, :, :hpf * frames], c["v"][:, :, :frames], c["y"][:, :, :hpf], c["v"][:, :, 0])
    _run(step, small)                                    # warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _run(step, small)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(step.wave["loss"]).item() and torch.isfinite(step.flat.params).all()
