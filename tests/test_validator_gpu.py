"""maavss_amd.Validator on the GPU, on the avse_S shape (the smallest model the GPU tests build: batch 2, 8 frames of 128^2, 256-point
STFT, 8 hops per frame) with the oracle's seeded weights.  Deterministic mode, so that two forwards of one batch give the same bytes
and sums can be compared exactly where the arithmetic is the same."""
import os

import numpy as np
import pytest
import torch

import maavss_amd
import quality_twin as tw
from maavss_amd import ops, quality

pytestmark = pytest.mark.gpu

S = 3          # num_seq of the clip and recording tests
MSE_BLK = 512  # csrc/elementwise.hip: the most workgroups of one maavss_mse_pair operand, 4096 elements each below that


@pytest.fixture(scope="module")
def small(golden_dir):
    from oracle import avse_ref_cpu as orc
    z = np.load(os.path.join(golden_dir, "avse_S.npz"), allow_pickle=False)
    m = {k[5:]: z[k].item() for k in z.files if k.startswith("meta_")}
    n_bins, t_a = m["fft_len"] // 2 + 1, m["hops_per_frame"] * m["frames"]
    shapes = ([m["batch"], 2, t_a, n_bins], [m["batch"], 1, m["frames"], m["width"], m["width"]], m["hops_per_frame"])
    model = maavss_amd.AV_Fusion_Model_Frames(*shapes, precise=True)
    model.load_state_dict(orc.seeded_state_dict(orc.AVFusionFramesRef(*shapes), m["seed"]), strict=True)
    model = model.to("cuda").eval()
    batch = [t.cuda() for t in orc.synthetic_batch(m["batch"], m["frames"], m["width"], t_a, n_bins, m["hops_per_frame"], m["seed"] + 1)]
    prev = maavss_amd.set_deterministic(True)
    yield dict(m=m, model=model, batch=batch, n_bins=n_bins, t_a=t_a)
    maavss_amd.set_deterministic(prev)


def _mse_bound(n):
    """Relative bound of maavss_mse_pair's f32 numerator against the f64 sum of the exact squares, u = 2^-24: a thread adds
    m = ceil(n / (256 G)) terms in f32, G = min(MSE_BLK, ceil(n / 4096)) workgroups (m u: every addition rounds a partial sum of
    non-negative terms), each term (pred - tgt)^2 with the difference rounded to f32 first (2 u); 6 additions of the wave reduction and 3
    across the waves (9 u); the f32 store of the loss (u).  The f64 side is within (n - 1) 2^-53, far below."""
    g = min(MSE_BLK, -(-n // 4096))
    m = -(-n // (256 * g))
    return (m + 12) * 2.0 ** -24


def test_add_windows_accumulates_the_numerators_of_mse_pair(small):
    model, (x_a, x_v, y_a, y_v), coeff = small["model"], small["batch"], small["m"]["loss_coeff"]
    with torch.no_grad():
        a, v, _ = model(x_a, x_v)
    losses, d_a, d_v = ops.mse_pair(a, y_a, v, y_v, coeff, 1, want_grads=False)
    assert d_a is None and d_v is None
    val = maavss_amd.Validator(model, loss_coeff=coeff)
    val.add_windows(x_a, x_v, y_a, y_v)
    res = val.result()
    la, lv, lt = (float(t) for t in losses.cpu())
    print(f"val_loss_stft {res['val_loss_stft']!r} mse_pair {la!r} bound {_mse_bound(a.numel()):.3g}; "
          f"val_loss_attn {res['val_loss_attn']!r} mse_pair {lv!r} bound {_mse_bound(v.numel()):.3g}")
    assert abs(res["val_loss_stft"] - la) <= _mse_bound(a.numel()) * la
    assert abs(res["val_loss_attn"] - lv) <= _mse_bound(v.numel()) * lv
    # the total: both terms' bounds, the f32 rounding of coeff inside the kernel and the f32 store
    assert abs(res["val_loss"] - lt) <= (max(_mse_bound(a.numel()), _mse_bound(v.numel())) + 2 * 2.0 ** -24) * lt
    assert res["val_loss"] == res["val_loss_stft"] + coeff * res["val_loss_attn"]
    assert res["n_windows"] == x_a.shape[0] and res["n_clips"] == 0
    # lsd_db is the mean over the windows of spectrum_metrics' rows
    lsd = quality.spectrum_metrics(a, y_a)["lsd_db"]
    assert abs(res["lsd_db"] - float(lsd.sum().cpu()) / x_a.shape[0]) <= 4 * tw.U53 * res["lsd_db"]


def test_batches_of_unequal_size_give_the_element_weighted_mean(small):
    model, (x_a, x_v, y_a, y_v) = small["model"], small["batch"]
    g = torch.Generator().manual_seed(3)
    x_a1, y_a1 = (x_a[:1] * 3).contiguous(), (y_a[:1] + torch.randn(y_a[:1].shape, generator=g).cuda()).contiguous()      # a worse batch of one
    x_v1, y_v1 = x_v[:1].contiguous(), (y_v[:1] + 2).contiguous()            # the sigmoid output is in (0, 1): a target far from it
    sums, elems = [], []
    with torch.no_grad():
        for xa, xv, ya, yv in ((x_a, x_v, y_a, y_v), (x_a1, x_v1, y_a1, y_v1)):
            a, v, _ = model(xa, xv)
            sums.append((float(quality.spectrum_metrics(a, ya)["sqerr"].sum().cpu()), float(quality.sqerr_rows(v, yv).sum().cpu())))
            elems.append((a.numel(), v.numel()))
    val = maavss_amd.Validator(model)
    val.add_windows(x_a, x_v, y_a, y_v)
    val.add_windows(x_a1, x_v1, y_a1, y_v1)
    res = val.result()
    for k, key in enumerate(("val_loss_stft", "val_loss_attn")):
        weighted = (sums[0][k] + sums[1][k]) / (elems[0][k] + elems[1][k])
        unweighted = 0.5 * (sums[0][k] / elems[0][k] + sums[1][k] / elems[1][k])
        assert abs(res[key] - weighted) <= 8 * tw.U53 * weighted, key
        assert abs(weighted - unweighted) > 1e-3 * weighted, "the two means must differ for the check to see the weighting"
    assert res["n_windows"] == 3


def test_validation_touches_no_parameter_buffer_or_gradient(small):
    m, (x_a, x_v, y_a, y_v) = small["m"], small["batch"]
    from oracle import avse_ref_cpu as orc
    shapes = ([m["batch"], 2, small["t_a"], small["n_bins"]], [m["batch"], 1, m["frames"], m["width"], m["width"]], m["hops_per_frame"])
    model = maavss_amd.AV_Fusion_Model_Frames(*shapes, precise=True)
    model.load_state_dict(orc.seeded_state_dict(orc.AVFusionFramesRef(*shapes), m["seed"]), strict=True)
    model = model.to("cuda").train()
    step = maavss_amd.TrainStep(model, lr=m["lr"], loss_coeff=m["loss_coeff"])
    step(x_a, x_v, y_a, y_v)                                   # gradients, moments and BatchNorm statistics hold something
    assert step.flat.grads.abs().max().item() > 0
    val = maavss_amd.Validator(model, loss_coeff=m["loss_coeff"])
    with pytest.raises(ValueError, match="training mode"):
        val.add_windows(x_a, x_v, y_a, y_v)
    model.eval()
    before = dict(params=step.flat.params.clone(), grads=step.flat.grads.clone(), touched=set(step.flat.touched),
                  buffers={k: b.clone() for k, b in model.named_buffers()})
    val.add_windows(x_a, x_v, y_a, y_v)
    clip_a = torch.cat([x_a, x_a[:, :, :8 * (S - 1)]], dim=2)
    clip_v = torch.cat([x_v, x_v[:, :, :S - 1]], dim=2)
    val3 = maavss_amd.Validator(model, num_seq=S)
    val3.add_clips(clip_a, clip_a, clip_v, clip_v, m["frames"], m["hops_per_frame"])
    assert val.result()["n_windows"] == m["batch"] and val3.result()["n_windows"] == S * m["batch"]
    assert torch.equal(step.flat.params, before["params"]) and torch.equal(step.flat.grads, before["grads"])
    assert step.flat.touched == before["touched"]
    for k, b in model.named_buffers():
        assert torch.equal(b, before["buffers"][k]), k
    for n, p in model.named_parameters():
        if n in step.flat.tensors:
            assert p.data_ptr() == step.flat.param_views[n].data_ptr() and p.grad.data_ptr() == step.flat.grad_views[n].data_ptr(), n


def test_add_clips_equals_add_windows_on_the_hand_sliced_windows(small):
    model, m = small["model"], small["m"]
    nf, hpf, w = m["frames"], m["hops_per_frame"], m["width"]
    g = torch.Generator().manual_seed(9)
    t_total = nf + S - 1
    x_stft = (0.5 * torch.randn(2, 2, hpf * t_total, small["n_bins"], generator=g)).cuda()
    y_stft = (0.3 * torch.randn(2, 2, hpf * t_total, small["n_bins"], generator=g)).cuda()
    x_attn = torch.rand(2, 1, t_total, w, w, generator=g).cuda()
    y_attn = torch.rand(2, 1, t_total, w, w, generator=g).cuda()
    clips = maavss_amd.Validator(model, num_seq=S)
    clips.add_clips(x_stft, y_stft, x_attn, y_attn, nf, hpf)
    hand = maavss_amd.Validator(model, num_seq=S)
    mid = (S - 1) // 2                                         # train_avse_frames.py:105
    for j in range(S):                                         # train_avse_frames.py:150-163, written out
        hand.add_windows(x_stft[:, :, hpf * j:hpf * (j + nf)], x_attn[:, :, j:j + nf],
                         y_stft[:, :, hpf * (j + mid):hpf * (j + mid + 1)], y_attn[:, :, j + mid])
    torch.cuda.synchronize()
    assert torch.equal(clips.acc, hand.acc)
    res = clips.result()
    assert res["n_windows"] == 2 * S and res["val_loss"] > 0


def test_add_recording_measures_the_estimate_and_the_noisy_input_over_the_same_span():
    from oracle import avse_ref_cpu as orc, stft_ref_cpu as sref
    t, w, fft, hpf = 8, 128, 256, 8
    hop, _, t_a = maavss_amd.calc_hop_size(t, hpf, 30, 16000)
    shapes = ([S, 2, t_a, fft // 2 + 1], [S, 1, t, w, w], hpf)
    model = maavss_amd.AV_Fusion_Model_Frames(*shapes, precise=True)
    model.load_state_dict(orc.seeded_state_dict(orc.AVFusionFramesRef(*shapes), 11), strict=True)
    model = model.cuda().eval()
    stft = maavss_amd.STFT(fft, hop, normalize_output_fft=True, device="cuda")
    enh = maavss_amd.Enhancer(model, stft, t, S, hpf)
    clip, step = hpf * hop * (t + S), S * hpf * hop
    length = step + clip + 37                                  # two clips and a tail
    clean = sref.synthetic_audio(1, length, 31)[0].cuda()
    g = torch.Generator().manual_seed(2)
    noisy = clean + 0.05 * torch.randn(length, generator=g).cuda()
    maps = torch.rand(14, 1, w, w, generator=g).cuda()         # per-frame attention maps: no ViT in this test
    prev = maavss_amd.set_deterministic(True)
    try:
        val = maavss_amd.Validator(model, num_seq=S, seg_len=256)
        val.add_recording(enh, noisy, clean, attn=maps)
        wave, start = enh(noisy, attn=maps)
        n = wave.shape[0]
        assert start == ((S - 1) // 2) * hpf * hop and n == enh.output_length(2) and n < length - start
        m_est = maavss_amd.wave_metrics(wave, clean[start:start + n])
        m_noisy = maavss_amd.wave_metrics(noisy[start:start + n], clean[start:start + n])
        res = val.result()
    finally:
        maavss_amd.set_deterministic(prev)
    assert res["n_clips"] == 1 and res["n_windows"] == 0
    for name in ("snr_db", "si_sdr_db", "seg_snr_db"):
        e, q = float(m_est[name].cpu()), float(m_noisy[name].cpu())
        print(f"{name}: estimate {e!r} noisy {q!r}")
        assert np.isfinite(e) and np.isfinite(q)
        assert res[name] == e and res["noisy_" + name] == q and res[name + "_improvement"] == e - q
        assert res[name + "_n_finite"] == 1 and res["noisy_" + name + "_n_finite"] == 1 and res[name + "_improvement_n_finite"] == 1
    # the noisy input against the clean one is what the twin says (the manual alignment, on the host)
    want = tw.wave_row(noisy[start:start + n].cpu().numpy(), clean[start:start + n].cpu().numpy(), 256)
    tw.check_wave_row(m_noisy["raw"].cpu().numpy()[0], want, n, label="noisy vs clean:")
    with pytest.raises(ValueError, match="another model"):
        maavss_amd.Validator(torch.nn.Linear(1, 1).eval()).add_recording(enh, noisy, clean, attn=maps)
