"""AudioTransform on the host (maavss_amd/audio_transform.py; av_dataset.py:203-215): the twin's dense sinc_interp_hann kernel against a
scalar evaluation, the compressed tap table the device kernel reads against that dense kernel, the length arithmetic, and every refusal
of AudioTransform, ClipPipeline(audio_transform=) and Enhancer(audio_transform=) -- all of it without a device."""
import math

import pytest
import torch

import audio_twin as tw

RATES = (48000, 44100, 22050, 11025, 8000, 32000)           # -> 16 000 Hz
S_EXPECTED = {48000: 37, 44100: 34, 22050: 17, 11025: 13, 8000: 13, 32000: 25}


def _ratio(sr, new=16000):
    g = math.gcd(sr, new)
    return sr // g, new // g


def _scalar_tap(p, i, orig, new, lpw=6, rolloff=0.99):
    base = min(orig, new) * rolloff
    width = math.ceil(lpw * orig / base)
    t = (-p / new + (i - width) / orig) * base
    t = max(-lpw, min(lpw, t))
    window = math.cos(t * math.pi / lpw / 2) ** 2
    tp = t * math.pi
    sinc = 1.0 if tp == 0 else math.sin(tp) / tp
    return sinc * (window * (base / orig))


@pytest.mark.parametrize("sr", (48000, 44100, 8000))
def test_twin_kernel_against_a_scalar_evaluation(sr):
    orig, new = _ratio(sr)
    dense, width = tw.sinc_kernel(orig, new, rounded=False)
    assert dense.dtype == torch.float64 and dense.shape == (new, 2 * width + orig)
    g = torch.Generator().manual_seed(sr)
    picks = {(0, width), (0, 0), (new - 1, dense.shape[1] - 1)}              # the centre tap (t = 0) and two clamped corners
    while len(picks) < min(48, dense.numel()):
        picks.add((int(torch.randint(new, (1,), generator=g)), int(torch.randint(dense.shape[1], (1,), generator=g))))
    worst = 0.0
    for p, i in picks:
        want, got = _scalar_tap(p, i, orig, new), dense[p, i].item()
        rel = abs(got - want) / abs(want) if want != 0 else abs(got)
        worst = max(worst, rel)
        assert rel <= 1e-15, (sr, p, i, got, want)
    assert dense[0, width].item() == min(orig, new) * 0.99 / orig              # sinc(0) = 1, window 1
    print(f"[audio twin] {sr}: {len(picks)} taps, worst relative difference to the scalar evaluation {worst:.1e}")


@pytest.mark.parametrize("sr", RATES)
def test_compressed_table_is_the_dense_table(sr):
    from maavss_amd.audio_transform import sinc_table
    orig, new = _ratio(sr)
    dense, width = tw.sinc_kernel(orig, new)
    taps, first, s, w = sinc_table(orig, new)
    assert w == width and s == math.ceil(2 * 6 * orig / (min(orig, new) * 0.99)) == S_EXPECTED[sr]
    assert taps.shape == (new, s) and taps.dtype == torch.float32 and first.shape == (new,) and first.dtype == torch.int32
    cols = first.to(torch.int64)[:, None] + torch.arange(s)[None, :]
    inside = (cols >= 0) & (cols < dense.shape[1])
    assert bool((taps[~inside] == 0).all())                                    # a stored tap past the dense row is a dead one
    rebuilt = torch.zeros_like(dense)
    rows = torch.arange(new)[:, None].expand(-1, s)
    rebuilt[rows[inside], cols[inside]] = taps[inside]
    live = dense != 0
    assert torch.equal(rebuilt[live], dense[live])                             # equal wherever the dense table is non-zero
    assert bool((rebuilt[~live] == 0).all())                                   # and nothing stored where it is exactly 0.0
    # the live taps of a phase are contiguous and at most S of them
    for p in range(new):
        nz = live[p].nonzero()[:, 0]
        assert 0 < nz.numel() <= s and int(nz[-1] - nz[0]) + 1 == nz.numel()
    # the property the kernel's staging relies on: first-tap positions of consecutive outputs never decrease
    n = torch.arange(2 * new + 256)
    start = (n // new) * orig + first.to(torch.int64)[n % new]
    assert bool((start[1:] >= start[:-1]).all())
    assert int((start[255:] - start[:-255]).max()) <= -(-255 * orig // new) + 1


def test_lengths():
    import maavss_amd
    t = maavss_amd.AudioTransform(16000)
    cases = [(44100, 23285, 8449), (44100, 23284, 8448), (44100, 441, 160), (44100, 1, 1), (48000, 25344, 8448), (48000, 25345, 8449),
             (22050, 11643, 8449), (8000, 4224, 8448), (16000, 8448, 8448), (16000, 1, 1), (32000, 3, 2), (11025, 441, 640)]
    for sr, n_in, n_out in cases:
        assert t.output_length(n_in, sr) == n_out == math.ceil(n_in * 16000 / sr), (sr, n_in)
    for sr, n_out, n_in in [(44100, 8448, 23285), (48000, 8448, 25344), (22050, 8448, 11643), (8000, 8448, 4224), (16000, 8448, 8448),
                            (44100, 1, 3), (44100, 960000, 2646000)]:
        assert t.input_length(n_out, sr) == n_in, (sr, n_out)
        assert t.output_length(n_in, sr) >= n_out                 # always enough; at 44.1 kHz one sample more than needed (8449)
    t2 = maavss_amd.AudioTransform(22050)
    assert t2.output_length(44100, 44100) == 22050 and t2.input_length(10, 44100) == 20


def test_table_is_built_once_per_rate_pair():
    import maavss_amd
    t = maavss_amd.AudioTransform()
    a, b = t.table(44100), t.table(44100)
    assert a[0] is b[0] and t.table(88200 // 2)[0] is a[0]
    assert t.table(48000)[0] is not a[0]


def test_refusals_of_the_transform():
    import maavss_amd
    AT = maavss_amd.AudioTransform
    for kw in (dict(samplerate=0), dict(samplerate=-16000), dict(samplerate=16000.0), dict(samplerate=True), dict(lowpass_filter_width=0),
               dict(lowpass_filter_width=2.5), dict(rolloff=0.0), dict(rolloff=1.01), dict(rolloff=-0.5), dict(rolloff="0.9")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            AT(**kw)
    t = AT(16000)
    x = torch.zeros(2, 3, 1000)
    for sr in (0, -1, 44100.0, None):
        with pytest.raises(ValueError, match="sr"):
            t.check(x, sr)
    with pytest.raises(ValueError, match="float32 or int16"):
        t.check(x.double(), 44100)
    with pytest.raises(ValueError, match="float32 or int16"):
        t.check([0.0, 1.0], 44100)
    with pytest.raises(ValueError, match=r"\[L0\], \[C, L0\] or \[B, C, L0\]"):
        t.check(torch.zeros(1, 2, 3, 4), 44100)
    with pytest.raises(ValueError, match="at least one"):
        t.check(torch.zeros(2, 0, 100), 44100)                    # no channel
    with pytest.raises(ValueError, match="at least one"):
        t.check(torch.zeros(2, 0), 44100)                          # no sample
    with pytest.raises(ValueError, match="layout"):
        t.check(torch.zeros(2, 1000, 3).transpose(1, 2), 44100)   # interleaved channels: last stride 3
    for bad in (0, -5, 2.0, True):
        with pytest.raises(ValueError, match="length"):
            t.check(x, 44100, length=bad)
    full = t.output_length(1000, 44100)
    t.check(x, 44100, length=full)
    with pytest.raises(ValueError, match="length"):
        t.check(x, 44100, length=full + 1)
    with pytest.raises(ValueError, match="length"):
        t.check(x, 16000, length=1001)
    for out in (torch.zeros(2, full, dtype=torch.float64), torch.zeros(3, full), torch.zeros(2, full + 1), torch.zeros(2 * full), "out"):
        with pytest.raises(ValueError, match="out"):
            t.check(x, 44100, out=out)
    with pytest.raises(ValueError, match="out layout"):
        t.check(x, 44100, out=torch.zeros(full, 2).t())
    with pytest.raises(ValueError, match="out layout"):
        t.check(x, 44100, length=10, out=torch.zeros(15).as_strided((2, 10), (5, 1)))          # overlapping rows
    raw, length = t.check(x, 44100, out=torch.zeros(2, full + 7)[:, :full])       # a view with padded rows is fine
    assert raw.shape == (2, 3, 1000) and length == full
    assert t.check(torch.zeros(1000, dtype=torch.int16), 48000)[0].shape == (1, 1, 1000)
    assert t.check(torch.zeros(2, 1000), 48000)[0].shape == (1, 2, 1000)
    assert t.check(torch.zeros(2, 1000), 48000, batched=True)[0].shape == (2, 1, 1000)


def test_table_size_and_ratio_refusals():
    import maavss_amd
    from maavss_amd.audio_transform import sinc_table
    t = maavss_amd.AudioTransform(16000)
    taps, first, s, _ = t.table(44101)                             # coprime rates: 16 000 phases, compressed about 2 MB
    assert taps.shape == (16000, s) and s == math.ceil(12 * 44101 / (16000 * 0.99)) and taps.numel() * 4 < 3 << 20
    with pytest.raises(ValueError, match=r"more than 2\^22"):
        maavss_amd.AudioTransform(400009).table(44101)             # 400009 phases x 13 taps > 2^22
    with pytest.raises(ValueError, match="1000001 -> 1000000"):
        sinc_table(1000001, 1000000)
    with pytest.raises(ValueError, match="ratio"):
        t.check(torch.zeros(1, 1, 4000), 2000000)                  # 125 : 1 -- more input per workgroup than the kernel stages
    with pytest.raises(ValueError, match="no table"):
        t.table(16000)


def test_cpu_tensors_raise():
    import maavss_amd
    t = maavss_amd.AudioTransform(16000)
    for sr in (16000, 44100):
        with pytest.raises(maavss_amd._lib.MaavssError, match="no CPU fallback"):
            t(torch.zeros(2, 1000), sr)
    with pytest.raises(maavss_amd._lib.MaavssError, match="no CPU fallback"):
        t(torch.zeros(1, 2, 1000, dtype=torch.int16), 48000, length=100, out=torch.zeros(1, 100))


def _bare_pipeline(audio_transform, audio_length):
    """A ClipPipeline without its side stream (the constructor opens one on the device): the host-side checks only."""
    import maavss_amd
    pipe = object.__new__(maavss_amd.ClipPipeline)
    pipe.audio_transform, pipe.audio_length = audio_transform, audio_length
    return pipe


def test_refusals_of_the_pipeline():
    import maavss_amd
    t = maavss_amd.AudioTransform(16000)
    # the constructor's refusals come before it opens the side stream
    with pytest.raises(ValueError, match="audio_length"):
        maavss_amd.ClipPipeline(None, None, 8, audio_transform=t)
    with pytest.raises(ValueError, match="audio_length"):
        maavss_amd.ClipPipeline(None, None, 8, audio_transform=t, audio_length=0)
    with pytest.raises(ValueError, match="audio_length"):
        maavss_amd.ClipPipeline(None, None, 8, audio_length=8448)
    plain = _bare_pipeline(None, None)
    assert plain.check_audio(torch.zeros(2, 8448), None) is None
    with pytest.raises(ValueError, match="audio_sr"):
        plain.check_audio(torch.zeros(2, 8448), 44100)
    pipe = _bare_pipeline(t, 8448)
    with pytest.raises(ValueError, match="audio_sr"):
        pipe.check_audio(torch.zeros(2, 2, 23285), None)
    with pytest.raises(ValueError, match=r"\[B, C, L0\] or \[B, L0\]"):
        pipe.check_audio(torch.zeros(23285), 44100)
    with pytest.raises(ValueError, match="length = 8448 exceeds the 8447"):
        pipe.check_audio(torch.zeros(2, 2, 23280), 44100)         # one sample short of the STFT's clip
    with pytest.raises(ValueError, match="float32 or int16"):
        pipe.check_audio(torch.zeros(2, 2, 23285, dtype=torch.int32), 44100)
    assert pipe.check_audio(torch.zeros(3, 2, 23285, dtype=torch.int16), 44100).shape == (3, 2, 23285)
    assert pipe.check_audio(torch.zeros(3, 23285), 44100).shape == (3, 1, 23285)


def test_refusals_of_the_enhancer():
    import maavss_amd
    n, s, a, fft, side = 8, 3, 8, 256, 128
    hop = maavss_amd.calc_hop_size(n, a, 30, 16000)[0]
    stft = maavss_amd.STFT(fft, hop, device="cpu")
    nb = stft.n_bins()
    model = maavss_amd.AV_Fusion_Model_Frames([2, 2, a * n, nb], [2, 1, n, side, side], a).eval()
    with pytest.raises(ValueError, match="audio_transform resamples to 22050"):
        maavss_amd.Enhancer(model, stft, n, s, a, audio_transform=maavss_amd.AudioTransform(22050))
    plain = maavss_amd.Enhancer(model, stft, n, s, a)
    clip = plain.clip_samples
    attn = torch.zeros(40, 1, side, side)
    with pytest.raises(ValueError, match="audio_transform="):
        plain._check(torch.zeros(2, 3 * clip), None, attn, audio_sr=44100)
    enh = maavss_amd.Enhancer(model, stft, n, s, a, audio_transform=maavss_amd.AudioTransform(16000))
    with pytest.raises(ValueError, match=r"\[L0\] or \[C, L0\]"):
        enh._check(torch.zeros(1, 2, 3 * clip), None, attn, audio_sr=44100)
    with pytest.raises(ValueError, match="float32 or int16"):
        enh._check(torch.zeros(2, 3 * clip, dtype=torch.float64), None, attn, audio_sr=44100)
    with pytest.raises(ValueError, match="shorter than one clip"):
        enh._check(torch.zeros(2, clip, dtype=torch.int16), None, attn, audio_sr=44100)       # `clip` samples at 44.1 kHz: 0.36 clips
    with pytest.raises(ValueError, match="1-D float32"):
        enh._check(torch.zeros(2, 3 * clip), None, attn)                                        # without audio_sr: today's contract
    raw_len = enh.audio_transform.input_length(3 * clip, 44100)
    n_clips, starts, raw = enh._check(torch.zeros(2, raw_len, dtype=torch.int16), None, attn, audio_sr=44100)
    assert raw.shape == (1, 2, raw_len) and (n_clips, starts) == enh.tiling(3 * clip, 40) and n_clips >= 1
