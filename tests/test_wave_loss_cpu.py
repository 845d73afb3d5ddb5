"""CPU-only part of the waveform loss (maavss_amd/wave_loss.py, csrc/wave_loss.hip): the float64 twin against torch.istft + torch.autograd,
the refusals of WaveformLoss, of TrainStep(wave_loss=, wave_weight=) and of the C entry (every call below fails before any launch), the
exports and the measured constants."""
import inspect
import types

import numpy as np
import pytest
import torch

import wave_loss_twin as tw
from maavss_amd import _lib


def _autograd(pred, tgt, shape, kind, eps):
    """torch.istft in float64 and autograd of the literal definition -> rows [B, 5], d(sum l)/d(pred) [B, 2, T, F]."""
    _, t, n, hop, trimmed, normalized = shape
    p = torch.from_numpy(pred).double().requires_grad_(True)
    win = torch.from_numpy(tw.window(n))

    def wave(z):
        c = torch.complex(z[:, 0], z[:, 1]).transpose(1, 2)                  # [B, F, T]
        if trimmed:
            c = torch.cat([c, torch.zeros_like(c[:, :1])], dim=1)
        return torch.istft(c, n, hop_length=hop, win_length=n, window=win, normalized=normalized, onesided=True, center=True)

    x, s = wave(p), wave(torch.from_numpy(tgt).double())
    assert x.shape[1] == hop * (t - 1)
    sxx, sss, sxs = (x * x).sum(1), (s * s).sum(1), (x * s).sum(1)
    if kind == "snr":
        e = ((x - s) ** 2).sum(1)
        l = 10 * torch.log10(e + eps) - 10 * torch.log10(sss + eps)
    else:
        alpha = sxs / (sss + eps)
        e = ((x - alpha[:, None] * s) ** 2).sum(1)
        l = 10 * torch.log10(e + eps) - 10 * torch.log10(alpha * alpha * sss + eps)
    l.sum().backward()
    rows = torch.stack([l, sxx, sss, sxs, e], dim=1).detach().numpy()
    return rows, p.grad.numpy(), x.detach().numpy()


def _rel_l2(a, b):
    return float(np.sqrt(np.sum((a - b) ** 2)) / np.sqrt(np.sum(b ** 2)))


@pytest.mark.parametrize("kind", tw.KINDS)
@pytest.mark.parametrize("shape", tw.SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_the_twin_is_torch_istft_and_autograd(shape, kind):
    for inp in tw.NOISY_INPUTS:
        pred, tgt = tw.make_case(shape, inp)
        rows, grad, x = _autograd(pred, tgt, shape, kind, tw.EPS)
        r = tw.loss_and_grad(pred, tgt, shape, kind, tw.EPS, grad_scale=1.0)
        e_wave, e_rows, e_grad = _rel_l2(r["x"], x), _rel_l2(r["rows"], rows), _rel_l2(r["grad"], grad)
        print(f"{inp}: relative L2 of the wave {e_wave:.3g}, of the rows {e_rows:.3g}, of the gradient {e_grad:.3g}; l {r['rows'][:, 0]}")
        assert e_wave <= 1e-10 and e_rows <= 1e-10 and e_grad <= 1e-10
        assert np.abs(r["rows"][:, 0] - rows[:, 0]).max() <= 1e-9
        assert (np.abs(r["rows"][:, 0]) <= 60.0).all()          # the noisy cases lie inside the range of the 1e-4 dB gate, read either way


@pytest.mark.parametrize("shape", tw.SHAPES[:7], ids=lambda s: "x".join(str(int(v)) for v in s))
def test_the_twins_waves_are_the_oracles_inverse(shape):
    from oracle import stft_ref_cpu as orc
    _, _, n, hop, trimmed, normalized = shape
    pred, _ = tw.make_case(shape, "k0.3")
    want = orc.istft_ref(torch.from_numpy(pred), n, hop, normalized=normalized, trim_stft_end=trimmed, dtype=torch.float64).numpy()
    got = tw.istft(pred, n, hop, normalized)
    assert got.shape == want.shape
    err = _rel_l2(got, want)
    print(f"the twin's wave against oracle.stft_ref_cpu.istft_ref in float64: relative L2 {err:.3g}")
    # the oracle's float64 window is the formula itself, the twin's its rounding to f32 (what the kernels read): each w[j] is off by at most
    # 2^-24 relative, which moves a frame's term by that and the envelope sum of w^2 by twice that
    assert err <= 3 * tw.U24


def test_exact_zeros_and_nan_rows():
    shape = tw.SHAPES[1]
    for kind in tw.KINDS:
        pred, tgt = tw.make_case(shape, "zero_pred")
        r = tw.loss_and_grad(pred, tgt, shape, kind)
        assert np.isfinite(r["rows"]).all() and np.isfinite(r["grad"]).all()
        if kind == "si_sdr":
            assert not r["grad"].any() and (r["rows"][:, 0] == 0.0).all()                    # the function's own saddle
        for inp in ("equal", "zero_tgt"):
            r = tw.loss_and_grad(*tw.make_case(shape, inp), shape, kind)
            assert np.isfinite(r["rows"]).all() and np.isfinite(r["grad"]).all(), (kind, inp)
        r = tw.loss_and_grad(*tw.make_case(shape, "nan"), shape, kind)
        assert np.isnan(r["rows"][-1]).all() and np.isnan(r["grad"][-1]).all() and np.isfinite(r["rows"][:-1]).all() and np.isfinite(r["grad"][:-1]).all()
        r = tw.loss_and_grad(*tw.make_case(shape, "inf"), shape, kind)
        assert np.isnan(r["rows"][0]).all() and np.isnan(r["grad"][0]).all() and np.isfinite(r["rows"][1:]).all() and np.isfinite(r["grad"][1:]).all()
        # the imaginary gradients of DC and Nyquist are zero
        r = tw.loss_and_grad(*tw.make_case(shape, "k0.3"), shape, kind)
        assert not r["grad"][:, 1, :, 0].any() and not r["grad"][:, 1, :, -1].any() and r["grad"][:, 0, :, 0].all()


def test_the_measured_constants_respect_their_caps():
    assert 0.0 < tw.K_WGRAD <= tw.K_CAP == 1e3
    if tw.K_WGRAD_MEASURED == tw.K_WGRAD_MEASURED:
        assert tw.K_WGRAD == min(tw.K_CAP, tw.round_up_to_power_of_ten(8.0 * tw.K_WGRAD_MEASURED))


def test_new_symbols_are_exported_and_the_abi_version_is_still_402():
    import maavss_amd
    assert hasattr(maavss_amd, "WaveformLoss")
    protos = _lib.parse_header()
    L = _lib.lib()
    for name in ("maavss_wave_loss_ws_bytes", "maavss_wave_loss"):
        assert name in protos and hasattr(L.cdll, name), name
    assert _lib.header_abi_version() == 402 == L.cdll.maavss_version()
    q = lambda *a: _lib.query("maavss_wave_loss_ws_bytes", *a)      # noqa: E731
    assert q(3, 5, 256, 66) > 0 and q(3, 5, 256, 66) % 256 == 0
    for bad in ((0, 5, 256, 66), (3, 1, 256, 66), (3, 5, 300, 66), (3, 5, 256, 0), (3, 5, 256, 257), (1 << 20, 1 << 20, 256, 66),
                (1, 1 << 24, 1024, 1024)):
        assert q(*bad) == 0, bad
    # the workspace holds the two waves, the frame buffer, the envelope and the chunk partials
    assert q(3, 5, 256, 66) >= 2 * 3 * 264 * 4 + 3 * 5 * 256 * 4 + 264 * 8 + 3 * 48 + 3 * 8 + 3 * 8 + 3 * 16


def test_waveform_loss_and_train_step_refuse_bad_parameters():
    import maavss_amd
    stft = maavss_amd.STFT(256, 66, device="cpu")
    loss = maavss_amd.WaveformLoss(stft)
    assert (loss.kind, loss.eps) == ("si_sdr", 1e-8) and maavss_amd.WaveformLoss(stft, "snr", 1).eps == 1.0
    sig = inspect.signature(maavss_amd.WaveformLoss.__init__).parameters
    assert (sig["kind"].default, sig["eps"].default) == ("si_sdr", 1e-8)
    with pytest.raises(ValueError, match="stft"):
        maavss_amd.WaveformLoss(None)
    for bad in (dict(kind="sdr"), dict(kind=None), dict(eps=0.0), dict(eps=-1e-8), dict(eps=float("inf")), dict(eps=float("nan")), dict(eps="1e-8"),
                dict(eps=True)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            maavss_amd.WaveformLoss(stft, **bad)
    x = torch.zeros(1, 2, 8, 129)
    with pytest.raises(ValueError, match=r"\[B, 2, T, F\]"):
        loss(torch.zeros(1, 3, 8, 129), torch.zeros(1, 3, 8, 129))
    with pytest.raises(ValueError, match=r"\[B, 2, T, F\]"):
        loss(x.double(), x.double())
    with pytest.raises(ValueError, match="differ in shape"):
        loss(x, torch.zeros(1, 2, 9, 129))
    with pytest.raises(ValueError, match="n_bins"):
        loss(torch.zeros(1, 2, 8, 128), torch.zeros(1, 2, 8, 128))
    with pytest.raises(ValueError, match="at least two frames"):
        loss(x[:, :, :1], x[:, :, :1])
    with pytest.raises(ValueError, match="grad_scale"):
        loss(x, x, grad_scale=float("nan"))
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        loss(x, x)
    # TrainStep: every refusal comes before the model is touched
    sig = inspect.signature(maavss_amd.TrainStep.__init__).parameters
    assert sig["wave_loss"].default is None and sig["wave_weight"].default == 1.0 and list(sig)[-2:] == ["wave_loss", "wave_weight"]
    model = types.SimpleNamespace(n_bins=129)
    with pytest.raises(ValueError, match="wave_loss must be None or a maavss_amd.WaveformLoss"):
        maavss_amd.TrainStep(model, wave_loss="si_sdr")
    with pytest.raises(ValueError, match="n_bins"):
        maavss_amd.TrainStep(model, wave_loss=maavss_amd.WaveformLoss(maavss_amd.STFT(256, 66, trim_stft_end=True, device="cpu")))
    for bad in (-0.5, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="wave_weight"):
            maavss_amd.TrainStep(model, wave_loss=loss, wave_weight=bad)


def _args(**over):
    """A call of maavss_wave_loss whose every argument passes (fake, aligned device addresses: never launched in these tests because one
    override makes a check fail)."""
    a = dict(pred=4100, tgt=4108, B=3, T=6, n_bins=129, window=4112, n_fft=256, hop=66, normalized=1, kind=0, eps=1e-8, grad_scale=1.0,
             d_pred=4116, d_frames=6, d_block_stride=0, accumulate=0, rows=8192, ws=8192, ws_bytes=1 << 24, stream=None)
    a.update(over)
    return tuple(a.values())


BAD = [(dict(pred=None), "null pointer"), (dict(tgt=None), "null pointer"), (dict(window=None), "null pointer"), (dict(rows=None), "null pointer"),
       (dict(ws=None), "null pointer"), (dict(B=0), "at least one row of two frames"), (dict(T=1), "at least one row of two frames"),
       (dict(n_fft=300), "n_fft must be 256, 512 or 1024"), (dict(n_bins=127), "n_bins must be"), (dict(n_bins=130), "n_bins must be"),
       (dict(hop=0), "hop must be in"), (dict(hop=257), "hop must be in"), (dict(kind=2), "kind must be"), (dict(kind=-1), "kind must be"),
       (dict(eps=0.0), "eps must be positive and finite"), (dict(eps=float("inf")), "eps must be positive and finite"),
       (dict(eps=float("nan")), "eps must be positive and finite"), (dict(grad_scale=float("nan")), "grad_scale must be finite"),
       (dict(grad_scale=float("inf")), "grad_scale must be finite"), (dict(B=1 << 20, T=1 << 20), "bad sizes"),
       (dict(pred=4101), "4-byte aligned"), (dict(d_pred=4118), "4-byte aligned"), (dict(rows=8196), "8-byte aligned"), (dict(ws=8196), "8-byte aligned"),
       (dict(d_frames=4), "does not divide"), (dict(d_frames=0), "does not divide"), (dict(d_frames=3, d_block_stride=100), "smaller than a block"),
       (dict(ws_bytes=64), "workspace of 64 bytes")]


@pytest.mark.parametrize("over,match", BAD, ids=[f"{next(iter(o))}-{i}" for i, (o, _) in enumerate(BAD)])
def test_wave_loss_refuses_bad_arguments_before_any_launch(over, match):
    with pytest.raises(_lib.MaavssError, match="wave_loss: .*" + match):
        _lib.call("maavss_wave_loss", *_args(**over))


def test_the_nullable_gradient_passes_the_checks():
    """d_pred may be null (the forward-only form), and then d_frames is not looked at: with every other argument valid the call would
    launch, so the checks are shown to pass by the one that comes after them all."""
    with pytest.raises(_lib.MaavssError, match="workspace of 8 bytes"):
        _lib.call("maavss_wave_loss", *_args(d_pred=None, d_frames=0, ws_bytes=8))
    with pytest.raises(_lib.MaavssError, match="workspace of 8 bytes"):
        _lib.call("maavss_wave_loss", *_args(d_frames=3, d_block_stride=3 * 2 * 3 * 129, accumulate=1, ws_bytes=8))
