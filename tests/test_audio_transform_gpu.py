"""AudioTransform on the device (maavss_audio_transform; av_dataset.py:203-215) against the torch CPU twin (tests/audio_twin.py).

Resampling: EVERY output element within a bound that follows from f32 arithmetic alone, against the twin run in float64 on the same
f32 taps and samples.  With u = 2^-24, a sum of n products formed in any order, with or without FMA, is within n u sum|tap_i x_i| of
the exact one; the downmix (C divisions and C - 1 additions) puts at most C u on each |x_i| = sum_c |x_c,i| / C; the result is rounded
once more.  Hence the bound (n_live + C + 2) u sum_i |tap_i| |x_i| + u |exact| per element, n_live = the live taps of the element's
phase.  Bit-exact cases: pass-through, int16 scaling, length=, out=, repeated calls, normalize.  Contrast: bound derived at
CONTRAST_BOUND.  Integration: ClipPipeline(audio_transform=) and Enhancer(audio_transform=) bit-identical to the stages run alone."""
import math

import pytest
import torch

import audio_twin as tw

pytestmark = pytest.mark.gpu

U = 2.0 ** -24

# contrast(x) = sin(t + 0.1 sin(4 t)), t = x pi/2, |x| <= 1, evaluated in f32 (operation by operation; a fused multiply-add only
# removes a rounding).  No document shipped with this ROCm installation states sinf's accuracy, so 2 ulp is taken, and an ulp is
# counted at its largest for |value| <= 1, 2^-23 = 2 u: E_SIN = 4 u.
#   t  = x * fl(pi/2)        constant and product rounded, |t| <= pi/2:                  d_t   = 2 u pi/2
#   s  = sinf(4 t)           4 t exact, |d sin| <= |d arg|:                              d_s   = 4 d_t + E_SIN
#   c  = fl(0.1) * s         constant and product rounded, |c| <= 0.1:                   d_c   = 0.1 d_s + 0.2 u
#   a  = t + c               one rounding at |a| <= pi/2 + 0.1:                          d_a   = d_t + d_c + (pi/2 + 0.1) u
#   y  = sinf(a)                                                                         d_y   = d_a + E_SIN
E_SIN = 4 * U
_D_T = 2 * U * math.pi / 2
_D_S = 4 * _D_T + E_SIN
_D_C = 0.1 * _D_S + 0.2 * U
CONTRAST_BOUND = _D_T + _D_C + (math.pi / 2 + 0.1) * U + E_SIN          # 10.7 u = 6.4e-7
CONTRAST_LIPSCHITZ = math.pi / 2 * (1 + 0.4)                              # |d/dx sin(t + 0.1 sin 4t)| <= pi/2 (1 + 0.4)


def _ratio(sr, new=16000):
    g = math.gcd(sr, new)
    return sr // g, new // g


def _lengths(t, sr):
    orig, _ = _ratio(sr)
    return [max(1, orig - 1), 7 * orig + (orig + 1) // 2, t.input_length(8448, sr)]      # < one frame; ends inside a frame; benched clip


def _resample_bound(x, sr, exact, extra=0):
    """Per-element bound of the module docstring for raw clips x [B, C, L0] (f32 or int16) and the float64 result `exact`; `extra`
    more roundings on every input sample."""
    orig, new = _ratio(sr)
    c = x.shape[1]
    kernel, width = tw.sinc_kernel(orig, new)
    absx = tw.to_float(x).double().abs().sum(dim=1) / c
    mag = tw.resample(absx, orig, new, kernel.abs(), width, torch.float64)
    n_live = (kernel != 0).sum(dim=1)
    n = n_live[torch.arange(exact.shape[1]) % new][None, :]
    return (n + c + 2 + extra) * U * mag[:, :exact.shape[1]] + U * exact.abs()


@pytest.mark.parametrize("dtype", (torch.float32, torch.int16), ids=("f32", "int16"))
@pytest.mark.parametrize("channels", (1, 2, 6))
@pytest.mark.parametrize("sr", (48000, 44100, 22050, 8000))
def test_resampling_every_element_within_the_f32_bound(sr, channels, dtype):
    import maavss_amd
    t = maavss_amd.AudioTransform(16000)
    worst, worst_f32 = 0.0, 0.0
    for k, l0 in enumerate(_lengths(t, sr)):
        for b in (1, 5):
            x = tw.signal(b, channels, l0, 1000 * k + 10 * b + channels + sr, dtype)
            got = t(x.cuda(), sr).cpu()
            exact = tw.chain(x, sr, dtype=torch.float64)
            assert got.shape == exact.shape == (b, t.output_length(l0, sr)) and got.dtype == torch.float32 and got.is_contiguous()
            bound = _resample_bound(x, sr, exact)
            err = (got.double() - exact).abs()
            ratio = (err / bound.clamp_min(1e-300)).max().item() if bool((bound > 0).any()) else 0.0
            assert bool((err[bound == 0] == 0).all())
            f32 = (got - tw.chain(x, sr)).abs().max().item()
            print(f"[audio resample] {sr} Hz C={channels} {str(dtype)[6:]} B={b} L0={l0}: worst error / bound {ratio:.3f}, "
                  f"max |error| {err.max().item():.2e}, max |difference to the f32 twin| {f32:.2e}")
            worst, worst_f32 = max(worst, ratio), max(worst_f32, f32)
            assert ratio <= 1.0, f"{sr} Hz C={channels} B={b} L0={l0}: error / bound = {ratio}"
    print(f"[audio resample] {sr} Hz C={channels} {str(dtype)[6:]}: worst error / bound over all cases {worst:.3f}; f32 twin {worst_f32:.2e}")


def test_bit_exact_cases():
    import maavss_amd
    t = maavss_amd.AudioTransform(16000)
    # pass-through: sr == samplerate
    x1 = tw.signal(3, 1, 8448, 1)
    assert torch.equal(t(x1.cuda(), 16000).cpu(), x1[:, 0])
    x2 = tw.signal(3, 2, 8448, 2)
    assert torch.equal(t(x2.cuda(), 16000).cpu(), tw.downmix(x2))                     # x / 2 exact, one rounding in the sum
    assert torch.equal(t(x2[0].cuda(), 16000).cpu(), tw.downmix(x2[:1]))              # [C, L0]
    assert torch.equal(t(x1[0, 0].cuda(), 16000).cpu(), x1[:1, 0])                    # [L0]
    # int16 against the same call on int16.float() / 32768
    for sr in (16000, 44100, 48000):
        xi = tw.signal(2, 2, 5000, 3 + sr, torch.int16).cuda()
        assert torch.equal(t(xi, sr), t(xi.float() / 32768, sr)), sr
    # length= against slicing the full result; two calls give identical bits
    x = tw.signal(2, 2, 23285, 4, torch.int16).cuda()
    full = t(x, 44100)
    assert full.shape == (2, 8449)
    assert torch.equal(full, t(x, 44100))
    for length in (8448, 257, 256, 1):
        assert torch.equal(t(x, 44100, length=length), full[:, :length]), length
    # a strided view of the input (clips cut out of a longer buffer)
    long = tw.signal(1, 2, 60000, 5).cuda()
    rows = long[0].as_strided((3, 2, 23285), (7000, 60000, 1))
    assert torch.equal(t(rows, 44100), t(rows.contiguous(), 44100))
    # out=: returned as is, nothing written outside [B, L]
    for sr, l0 in ((44100, 23285), (16000, 8448)):
        xs = tw.signal(2, 2, l0, 6 + sr).cuda()
        want = t(xs, sr, length=8448)
        guard = torch.full((4, 8448 + 64), 7.25, device="cuda")
        out = guard[1:3, 32:32 + 8448]
        ret = t(xs, sr, length=8448, out=out)
        assert ret is out and torch.equal(out, want)
        mask = torch.ones_like(guard, dtype=torch.bool)
        mask[1:3, 32:32 + 8448] = False
        assert bool((guard[mask] == 7.25).all()), sr


@pytest.mark.parametrize("channels", (1, 2))
def test_normalize_multiplies_by_the_exact_clip_maximum(channels):
    import maavss_amd
    t = maavss_amd.AudioTransform(16000, normalize=True)
    x = tw.signal(4, channels, 8448, 20 + channels)
    x[1] *= 0.125                                                                         # per clip, not per batch
    want = tw.normalize(tw.downmix(x))
    assert torch.equal(t(x.cuda(), 16000).cpu(), want)
    # resampled: the scaled clip through the resampler.  The clip maximum carries the downmix's C roundings and the scaling is one
    # more, so every input sample has C + 1 roundings more than in the plain bound, and all magnitudes are times the maximum m.
    xr = tw.signal(3, channels, 23285, 30 + channels)
    got = t(xr.cuda(), 44100).cpu()
    exact = tw.chain(xr, 44100, normalize_clip=True, dtype=torch.float64)
    m = tw.downmix(xr).abs().amax(dim=-1, keepdim=True).double()
    bound = (_resample_bound(xr, 44100, exact, extra=channels + 1) - U * exact.abs()) * m + U * exact.abs()
    ratio = ((got.double() - exact).abs() / bound).max().item()
    print(f"[audio normalize] C={channels}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_contrast_every_element_within_the_derived_bound():
    import maavss_amd
    t = maavss_amd.AudioTransform(16000, compress_audio=True)
    assert 1.0e-7 < CONTRAST_BOUND < 1e-6
    # pass-through path: |x| <= 1 including the ends and a dense sweep
    x = torch.cat([torch.linspace(-1, 1, 100001), tw.signal(1, 1, 50000, 40)[0, 0], torch.tensor([0.0, 1.0, -1.0])])[None, None]
    got = t(x.cuda(), 16000).cpu()
    exact = tw.contrast(x[:, 0].double())
    err = (got.double() - exact).abs().max().item()
    print(f"[audio contrast] pass-through: max |error| {err:.2e}, bound {CONTRAST_BOUND:.2e}, f32 twin "
          f"{(got - tw.contrast(x[:, 0])).abs().max().item():.2e}")
    assert err <= CONTRAST_BOUND
    # resampled path: the resampling bound through the map's Lipschitz constant, plus the map's own
    for sr, c, dtype in ((44100, 2, torch.int16), (48000, 1, torch.float32), (8000, 6, torch.float32)):
        xr = 0.8 * tw.signal(2, c, t.input_length(8448, sr), 41 + sr)                     # headroom: the resampled clip stays in [-1, 1]
        if dtype == torch.int16:
            xr = (xr * 32767).round().to(torch.int16)
        got = t(xr.cuda(), sr).cpu()
        lin = tw.chain(xr, sr, dtype=torch.float64)
        assert float(lin.abs().max()) <= 1.0                                              # the derivation's range
        exact = tw.contrast(lin)
        bound = CONTRAST_BOUND + CONTRAST_LIPSCHITZ * _resample_bound(xr, sr, lin)
        ratio = ((got.double() - exact).abs() / bound).max().item()
        print(f"[audio contrast] {sr} Hz C={c}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0


def test_pipeline_hands_out_the_stft_of_the_transformed_clips():
    import maavss_amd
    from oracle import vit_ref_cpu as vref
    b, tf, w, fft, hpf = 2, 8, 128, 256, 8
    hop, length, _ = maavss_amd.calc_hop_size(tf, hpf, 30, 16000)
    va = maavss_amd.VideoAttention(path_to_weights="/nonexistent.pth")
    va.load_state_dict(vref.seeded_vit_state(3))
    stft = maavss_amd.STFT(fft, hop, noise_std=0.1, device="cuda")
    at = maavss_amd.AudioTransform(16000)
    l0 = at.input_length(length, 44100)
    frames = [vref.synthetic_frames(b * tf, w, 300 + i).cuda() for i in range(3)]
    raw = [tw.signal(b, 2, l0, 400 + i, torch.int16).cuda() for i in range(3)]
    want = [stft(at(raw[i], 44100, length=length), seed=i) for i in range(3)]
    want = [(x.clone(), y.clone()) for x, y in want]
    torch.cuda.synchronize()
    pipe = maavss_amd.ClipPipeline(va, stft, tf, audio_transform=at, audio_length=length)
    for i in range(3):
        # inputs dropped right after submit(): the side stream must still read them (allocator reuse)
        pipe.submit(frames[i].clone(), raw[i].clone(), seed=i, audio_sr=44100)
        junk = [torch.full_like(raw[i], 12345) for _ in range(4)] + [torch.full_like(frames[i], float("nan")) for _ in range(2)]
        del junk
        if i >= 1:
            _, x_stft, y_stft = pipe.get()
            assert torch.equal(x_stft, want[i - 1][0]) and torch.equal(y_stft, want[i - 1][1]), f"batch {i - 1}"
            pipe.release()
    _, x_stft, y_stft = pipe.get()
    assert torch.equal(x_stft, want[2][0]) and torch.equal(y_stft, want[2][1]), "batch 2"
    pipe.release()
    pipe.drain()
    with pytest.raises(ValueError, match="exceeds"):
        pipe.submit(frames[0], raw[0][:, :, :l0 - 8], seed=0, audio_sr=44100)
    with pytest.raises(ValueError, match="audio_sr"):
        maavss_amd.ClipPipeline(va, stft, tf).submit(frames[0], raw[0], seed=0, audio_sr=44100)


def test_enhancer_on_a_raw_recording_equals_the_enhancer_on_the_transformed_audio():
    import maavss_amd
    from oracle import avse_ref_cpu as orc
    n, s, w, fft, hpf, n_frames = 8, 3, 128, 256, 8, 21
    hop, _, t_a = maavss_amd.calc_hop_size(n, hpf, 30, 16000)
    shapes = ([s, 2, t_a, fft // 2 + 1], [s, 1, n, w, w], hpf)
    model = maavss_amd.AV_Fusion_Model_Frames(*shapes)
    model.load_state_dict(orc.seeded_state_dict(orc.AVFusionFramesRef(*shapes), 11), strict=True)
    model = model.cuda().eval()
    stft = maavss_amd.STFT(fft, hop, normalize_output_fft=True, device="cuda")
    at = maavss_amd.AudioTransform(16000)
    clip, step = hpf * hop * (n + s), s * hpf * hop
    raw = tw.signal(1, 2, at.input_length(3 * step + clip + 100, 44100), 50, torch.int16)[0].cuda()      # [2, L0] stereo int16
    g = torch.Generator().manual_seed(51)
    attn = torch.rand(n_frames, 1, w, w, generator=g).cuda()
    prev = maavss_amd.set_deterministic(True)
    try:
        plain = maavss_amd.Enhancer(model, stft, n, s, hpf)
        enh = maavss_amd.Enhancer(model, stft, n, s, hpf, audio_transform=at)
        want, start = plain(at(raw, 44100)[0], attn=attn)
        got, start2 = enh(raw, attn=attn, audio_sr=44100)
        assert start == start2 and torch.equal(got, want) and want.numel() > 0
        x_a, x_v, amax = enh.window_inputs(raw, attn=attn, audio_sr=44100)
        x_a2, x_v2, amax2 = plain.window_inputs(at(raw, 44100)[0], attn=attn)
        assert torch.equal(x_a, x_a2) and torch.equal(x_v, x_v2) and torch.equal(amax, amax2)
    finally:
        maavss_amd.set_deterministic(prev)
