"""maavss_amd.Mixer on the GPU against its float64 twin (tests/mix_twin.py).

Gate of x and y (test 1): the project's own STFT gate (tests/test_stft_gpu.py: 5e-6 at |y| <= 0.5, i.e. 1e-5 of the largest coefficient;
2e-5 with normalize_output_fft), scaled by the twin's largest |x|, plus per element eps_g |g c I| for the error of the gain.
tests/test_mixer_cpu.py checks that the same chain in torch float32 stays inside it on these inputs.

Bound of the gain (test 2), from float32 arithmetic alone, u = 2^-24.  g = f sqrt(Sc / Si), Sc = sum a^2, Si = sum s^2 (the 1/L of the mean
powers cancels); the twin evaluates the same in float64 from the float32 snr_db.
  * a sum of squares: thread i runs over samples i, i + 256, ...: n_seq = ceil(L / 256) fused multiply-adds (one rounding each), then a
    binary tree over 256 partials, log2(256) = 8 additions deep.  All terms are >= 0, so the relative error of the sum is at most the
    number of roundings on the longest path: (n_seq + 8) u <= (n_seq + log2(threads) + 1) u =: e_p;
  * s itself is a float32 sum of K_b rows: |ds[n]| <= (K_b - 1) u A[n], A = sum_k |pool_k|, so Si moves by at most
    2 (K_b - 1) u sum |s| A, relative 2 e_f with e_f = (K_b - 1) u sum_n |s| A / sum_n s^2 (0 for a single partner);
  * Sc / Si: e_p + (e_p + 2 e_f) + u; the square root halves that and rounds once: e_p + e_f + 1.5 u; the product with f rounds once more
    and f itself is 10^(-snr/20) rounded to float32: + 2 u.
  eps_g = (n_seq + log2(threads) + 1 + 3.5) u + e_f, taken as (n_seq + 9 + 4) u + e_f so that the half u absorbs the second-order terms
  (they are below (20 u)^2).  For L = 594 that is 16 u + e_f, for L = 8448 46 u + e_f; the any-order bound (L + 4) u is asserted to be larger.

Mixture waveform (test 5): a + g s with s the float32 sum of K rows ((K - 1) roundings), the product and the sum (one fused
multiply-add): within (K + 2) u (|a| + |g| sum_k |pool_k|) of the float64 mixture built with the device's own gain.
"""
import pytest
import torch

import maavss_amd
import mix_twin as tw
from oracle import stft_ref_cpu as sref

pytestmark = pytest.mark.gpu

U = tw.U


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _stft(fft_len=512, hop=tw.HOP, **kw):
    kw.setdefault("noise_std", tw.SIGMA)
    return maavss_amd.STFT(fft_len, hop, device="cuda", **kw)


def _cuda(t):
    return None if t is None else t.cuda()


@pytest.mark.parametrize("fft_len,trim,norm,k,own_pool", tw.CASES)
def test_x_and_y_against_the_twin_every_element(fft_len, trim, norm, k, own_pool):
    audio, pool, partners, snr = tw.inputs(k, own_pool)
    src = audio if pool is None else pool
    st = _stft(fft_len, trim_stft_end=trim, normalize_output_fft=norm)
    noise = tw.noise_for(tw.BATCH, tw.LENGTH, tw.HOP, st.n_bins())
    x, y, gain = maavss_amd.Mixer(st, k)(audio.cuda(), partners, snr, pool=_cuda(pool), noise=noise.cuda(), return_gain=True)
    assert x.shape == y.shape == (tw.BATCH, 2, tw.LENGTH // tw.HOP, st.n_bins())
    g64 = tw.gain(audio, src, partners, snr)
    x64, y64, term = tw.example(audio, src, partners, g64, fft_len, tw.HOP, tw.SIGMA, noise, trim=trim, normalize_output=norm)
    eps_g = tw.gain_bound(audio, src, partners)
    tol_x = tw.gate(norm) * float(x64.abs().max()) + eps_g[:, None, None, None] * term.abs()
    ex, ey = (x.cpu().double() - x64).abs(), (y.cpu().double() - y64).abs()
    print(f"[mixer] n_fft {fft_len} trim {trim} norm {norm} K {k} own pool {own_pool}: worst x error / tolerance {float((ex / tol_x).max()):.3f}, "
          f"y {float(ey.max()) / (tw.gate(norm) * float(y64.abs().max())):.3f}; largest |term| / |y| {float(term.abs().max() / y64.abs().max()):.2f}")
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all())
    assert bool((ex <= tol_x).all())
    assert float(ey.max()) <= tw.gate(norm) * float(y64.abs().max())
    assert float(term.abs().max()) > 0.05 * float(y64.abs().max())          # the mix is not hiding under the gate


def test_benched_clip_against_the_twin():
    b, length, k = 32, 8448, 4
    audio = sref.synthetic_audio(b, length, 21)
    st = _stft(512)
    mixer = maavss_amd.Mixer(st, k, (-5.0, 30.0))
    partners, snr = mixer.sample(b, torch.Generator().manual_seed(2))
    partners[3, 1:] = -1
    partners[7] = -1
    noise = tw.noise_for(b, length, tw.HOP, 257)
    x, y, mix, gain = mixer(audio.cuda(), partners, snr, noise=noise.cuda(), return_mixture=True, return_gain=True)
    g64 = tw.gain(audio, audio, partners, snr)
    x64, y64, term = tw.example(audio, audio, partners, g64, 512, tw.HOP, tw.SIGMA, noise)
    eps_g = tw.gain_bound(audio, audio, partners)
    assert bool((eps_g <= (length + 4) * U).all())
    live = g64 > 0
    rel = ((gain.cpu().double() - g64).abs() / g64.clamp_min(1e-300))[live]
    print(f"[mixer] B = 32, L = 8448: worst gain error / bound {float((rel / eps_g[live]).max()):.3f}")
    assert bool((rel <= eps_g[live]).all()) and float(gain[7]) == 0.0
    tol_x = tw.gate(False) * float(x64.abs().max()) + eps_g[:, None, None, None] * term.abs()
    assert bool(((x.cpu().double() - x64).abs() <= tol_x).all())
    assert float((y.cpu().double() - y64).abs().max()) <= tw.gate(False) * float(y64.abs().max())
    _check_mixture(audio, audio, partners, snr, gain, mix, eps_g)


@pytest.mark.parametrize("own_pool,k", sorted(tw.PARTNERS))
def test_gain_within_the_f32_bound(own_pool, k):
    audio, pool, partners, snr = tw.inputs(k, own_pool)
    src = audio if pool is None else pool
    _, _, gain = maavss_amd.Mixer(_stft(), k)(audio.cuda(), partners, snr, pool=_cuda(pool), return_gain=True)
    g64 = tw.gain(audio, src, partners, snr)
    eps_g = tw.gain_bound(audio, src, partners)
    assert bool((eps_g <= (tw.LENGTH + 4) * U).all()), eps_g / U                      # never looser than the any-order bound
    got = gain.cpu().double()
    live = g64 > 0
    assert bool((got[~live] == 0).all()) and bool(torch.isfinite(got).all())
    rel = (got - g64).abs()[live] / g64[live]
    print(f"[mixer] gain, K {k} own pool {own_pool}: bound {[round(float(e / U), 1) for e in eps_g]} u, worst error / bound "
          f"{float((rel / eps_g[live]).max()):.3f}")
    assert bool((rel <= eps_g[live]).all())


def test_degenerate_clips_have_zero_gain_and_leave_x_equal_to_y():
    audio = sref.synthetic_audio(tw.BATCH, tw.LENGTH, 11)
    audio[1] = 0                                                    # a silent target, and clip 0's only interferer
    partners = torch.tensor([[1, -1], [2, 3], [0, 4], [-1, -1], [3, -1]], dtype=torch.int32)
    snr = torch.tensor(tw.SNRS)
    for norm in (False, True):
        for pool in (None, torch.zeros(5, tw.LENGTH)):              # the batch as pool / an all-zero pool
            st0 = _stft(noise_std=0.0, normalize_output_fft=norm)
            x, y, mix, gain = maavss_amd.Mixer(st0, 2)(audio.cuda(), partners, snr, pool=_cuda(pool), return_mixture=True, return_gain=True)
            dead = [0, 1, 3] if pool is None else [0, 1, 2, 3, 4]
            for t in (x, y, mix, gain):
                assert bool(torch.isfinite(t).all())
            for b in range(tw.BATCH):
                if b in dead:
                    assert float(gain[b]) == 0.0 and _same_bits(x[b], y[b]) and _same_bits(mix[b].cpu(), audio[b]), (norm, b)
                else:
                    assert float(gain[b]) > 0.0 and not torch.equal(x[b], y[b]), (norm, b)
            # with noise on, the dead clips are exactly the plain call's
            st = _stft(normalize_output_fft=norm)
            xn, yn = maavss_amd.Mixer(st, 2)(audio.cuda(), partners, snr, pool=_cuda(pool), seed=4)
            xp, yp = st(audio.cuda(), seed=4)
            assert bool(torch.isfinite(xn).all()) and _same_bits(yn, yp)
            assert bool(((xn[dead].double() - xp[dead].double()).abs() <= 4 * U * torch.maximum(xp[dead].abs(), yp[dead].abs()).double()).all())
            if not norm:                                            # same expression on the same operands
                assert torch.equal(xn[dead], xp[dead])


@pytest.mark.parametrize("norm", [False, True])
def test_a_near_silent_interferer_leaves_the_clip_unmixed(norm):
    """Interferers at 1e-20 of the clips' level: their squares are float32 denormals (or flush to 0), Sc / Si is past float's range, and
    the gain the definition asks for (some 1e20) times such a signal is nothing a float32 front end can form.  The clip then stays
    unmixed: g = 0 exactly, x = y bit for bit at sigma = 0, the mixture is the clip, and no inf or NaN reaches an output."""
    audio = sref.synthetic_audio(tw.BATCH, tw.LENGTH, 11)
    pool = sref.synthetic_audio(tw.POOL, tw.LENGTH, 12) * 1e-20
    assert float(pool.abs().max()) > 0 and float(pool.double().pow(2).sum(1).min()) < 1e-36
    partners = torch.tensor([[0, -1], [1, 2], [2, 0], [1, -1], [-1, -1]], dtype=torch.int32)
    snr = torch.tensor(tw.SNRS)
    st0 = _stft(noise_std=0.0, normalize_output_fft=norm)
    x, y, mix, gain = maavss_amd.Mixer(st0, 2)(audio.cuda(), partners, snr, pool=pool.cuda(), return_mixture=True, return_gain=True)
    for t in (x, y, mix, gain):
        assert bool(torch.isfinite(t).all())
    assert bool((gain == 0).all()) and _same_bits(x, y) and _same_bits(mix.cpu(), audio)
    # the batch as pool, one clip near-silent: it cannot be mixed INTO the others, but the others are mixed into it (a small finite gain)
    audio[1] *= 1e-20
    partners = torch.tensor([[1, -1], [0, 2], [1, -1], [2, 4], [-1, -1]], dtype=torch.int32)
    x, y, mix, gain = maavss_amd.Mixer(st0, 2)(audio.cuda(), partners, snr, return_mixture=True, return_gain=True)
    for t in (x, y, mix, gain):
        assert bool(torch.isfinite(t).all())
    assert gain.cpu().tolist()[0] == 0.0 and gain.cpu().tolist()[2] == 0.0 and float(gain[3]) > 0.0 and float(gain[4]) == 0.0
    assert 0.0 <= float(gain[1]) < 1e-15
    assert _same_bits(x[0], y[0]) and _same_bits(x[2], y[2]) and not torch.equal(x[3], y[3])


def test_the_call_does_not_wait_for_its_stream():
    """Mixer.__call__ queues its work and returns: partners and SNR factors go to the device through pinned memory, not with a blocking
    copy.  On ClipPipeline's side stream a blocking copy would hold the host until the extraction queued in front of it had finished,
    and the two streams would run one after the other.  Here a device-side spin (tens of milliseconds, no host wait) stands for that
    extraction: when the call returns, the event recorded behind the spin must still be pending."""
    audio = sref.synthetic_audio(tw.BATCH, tw.LENGTH, 11).cuda()
    mixer = maavss_amd.Mixer(_stft(normalize_output_fft=False), 2)
    want = mixer(audio, seed=1, return_mixture=True, return_gain=True)      # warm: the library, the allocators' blocks
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(50_000_000)
        busy = torch.cuda.Event()
        busy.record()
        got = mixer(audio, seed=1, return_mixture=True, return_gain=True)
        returned_early = not busy.query()
    side.synchronize()
    assert returned_early, "Mixer.__call__ synchronised with its stream"
    for u, v in zip(want, got):
        assert _same_bits(u, v)


@pytest.mark.parametrize("norm", [False, True])
def test_y_is_the_plain_call_s_and_calls_repeat_bit_for_bit(norm):
    for fft_len in (256, 512, 1024):
        for trim in (False, True):
            audio, _, partners, snr = tw.inputs(2, True)
            st = _stft(fft_len, trim_stft_end=trim, normalize_output_fft=norm)
            mixer = maavss_amd.Mixer(st, 2)
            a = mixer(audio.cuda(), partners, snr, seed=3, return_mixture=True, return_gain=True)
            b = mixer(audio.cuda(), partners, snr, seed=3, return_mixture=True, return_gain=True)
            _, y_plain = st(audio.cuda(), want_x=False)
            assert _same_bits(a[1], y_plain), (fft_len, trim)
            for u, v in zip(a, b):
                assert _same_bits(u, v), (fft_len, trim)
            # rows of a longer buffer (a row stride above L) against their contiguous copy
            wide = torch.zeros(tw.BATCH, tw.LENGTH + 37)
            wide[:, :tw.LENGTH] = audio
            wide[:, tw.LENGTH:] = 7.0                                # must never be read
            c = mixer(wide.cuda()[:, :tw.LENGTH], partners, snr, seed=3, return_mixture=True, return_gain=True)
            for u, v in zip(a, c):
                assert _same_bits(u, v), (fft_len, trim, "strided")


@pytest.mark.parametrize("length", [tw.LENGTH, 660])
@pytest.mark.parametrize("norm", [False, True])
def test_grid_independence(norm, length):
    """The first 5 clips of a 264-clip launch equal the 5-clip launch, for gain, x and y (the partners of the first 5 are among them).

    One exception, which is the plain STFT's and not the mixer's: maavss_stft_fwd packs the frames of a launch two by two into one complex
    FFT, across clip borders.  With 9 frames per clip frame 44 (clip 4, frame 8) shares its FFT with frame 45 in the 264-clip launch and
    with nothing in the 5-clip launch, and its y moves in the last bits (measured on the MI355X: stft(audio)[1] itself differs there and
    only there).  y has to be bit for bit what stft(audio, want_x=False) returns for the same batch, so it cannot be both; at that frame the
    test asks for that identity in both launches instead, and for x within the gate of test 1.  With normalize_output_fft the clip's
    maximum may sit in that frame, so there the whole of clip 4 falls under the exception.  Everything else, and every frame at the even
    frame count (660 samples, 10 frames), is held to bit equality; the mixer's own kernels pair frames inside a clip."""
    frames = length // tw.HOP
    big = sref.synthetic_audio(264, length, 11)
    partners5 = torch.tensor(tw.PARTNERS[(True, 2)], dtype=torch.int32)
    snr5 = torch.tensor(tw.SNRS)
    rest = 5 + torch.arange(259 * 2, dtype=torch.int32).view(259, 2) % 259
    rest[rest == torch.arange(5, 264, dtype=torch.int32)[:, None]] = -1
    partners = torch.cat([partners5, rest])
    snr = torch.cat([snr5, torch.full((259,), 3.0)])
    for fft_len in (256, 512, 1024):
        st = _stft(fft_len, normalize_output_fft=norm)
        mixer = maavss_amd.Mixer(st, 2)
        xb, yb, gb = mixer(big.cuda(), partners, snr, seed=5, return_gain=True)
        xs, ys, gs = mixer(big[:5].cuda(), partners5, snr5, seed=5, return_gain=True)
        assert _same_bits(gb[:5], gs), fft_len
        assert _same_bits(yb, st(big.cuda(), want_x=False)[1]) and _same_bits(ys, st(big[:5].cuda(), want_x=False)[1]), fft_len
        same = torch.ones(5, frames, dtype=torch.bool)
        if frames % 2:
            same[4, -1] = False                                       # the frame the plain launch pairs differently
            if norm:
                same[4] = False                                       # ... and whose coefficients may be the clip's maximum
        keep = same[:, None, :, None].expand_as(ys).cuda()
        assert torch.equal(_bits(yb[:5])[keep], _bits(ys)[keep]), fft_len
        assert torch.equal(_bits(xb[:5])[keep], _bits(xs)[keep]), fft_len
        tol = tw.gate(norm) * float(xs.abs().max())
        assert float((xb[:5] - xs).abs().max()) <= tol and float((yb[:5] - ys).abs().max()) <= tol, fft_len


@pytest.mark.parametrize("norm", [False, True])
def test_noise_stream_is_the_plain_call_s(norm):
    """(x_mix(seed) - x_mix(sigma = 0)) against (x_plain(seed) - y), differences taken in float64, element-wise within
    4 u max(|x_mix|, |x_plain|); clip 4 has no partner, bin n_fft / 2 is the last one of every row."""
    audio, _, partners, snr = tw.inputs(1, True)
    assert partners[4].tolist() == [-1]
    a = audio.cuda()
    for fft_len in (256, 512, 1024):
        st, st0 = _stft(fft_len, normalize_output_fft=norm), _stft(fft_len, noise_std=0.0, normalize_output_fft=norm)
        x_mix, y_mix = maavss_amd.Mixer(st, 1)(a, partners, snr, seed=7)
        x_mix0, _ = maavss_amd.Mixer(st0, 1)(a, partners, snr, seed=7)
        x_plain, y = st(a, seed=7)
        assert _same_bits(y_mix, y)
        d_mix, d_plain = x_mix.double() - x_mix0.double(), x_plain.double() - y.double()
        tol = 4 * U * torch.maximum(x_mix.abs(), x_plain.abs()).double()
        err = (d_mix - d_plain).abs()
        print(f"[mixer] noise stream, n_fft {fft_len} norm {norm}: worst error / tolerance {float((err / tol.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= tol).all()), fft_len
        assert abs(float(d_mix.std()) / tw.SIGMA - 1) < 0.05                        # and it is noise
        if not norm:
            assert torch.equal(x_mix[4], x_plain[4])                                  # no partner: the plain call's x, same expression
        assert not torch.equal(x_mix[0], x_plain[0])


def _check_mixture(audio, src, partners, snr, gain, mix, eps_g):
    k = partners.shape[1]
    g = gain.cpu().double()
    want = tw.mixture(audio, src, partners, g)
    bound = (k + 2) * U * (audio.double().abs() + g[:, None] * tw.abs_sum(src, partners))
    err = (mix.cpu().double() - want).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    live = g > 0
    got = tw.realised_snr_db(audio, mix.cpu())[live]
    tol_db = -20.0 * torch.log10(1.0 - eps_g[live])
    miss = (got - snr.double()[live]).abs()
    print(f"[mixer] mixture K {k}: worst sample error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, "
          f"realised SNR off by at most {float(miss.max()):.2e} dB, worst / tolerance {float((miss / tol_db).max()):.3f}")
    assert bool((miss <= tol_db).all())


@pytest.mark.parametrize("own_pool,k", sorted(tw.PARTNERS))
def test_mixture_waveform(own_pool, k):
    audio, pool, partners, snr = tw.inputs(k, own_pool)
    src = audio if pool is None else pool
    x, y, mix, gain = maavss_amd.Mixer(_stft(), k)(audio.cuda(), partners, snr, pool=_cuda(pool), return_mixture=True, return_gain=True)
    assert mix.shape == audio.shape
    _check_mixture(audio, src, partners, snr, gain, mix, tw.gain_bound(audio, src, partners))


def test_sampled_call_draws_what_sample_draws():
    audio = sref.synthetic_audio(tw.BATCH, tw.LENGTH, 11).cuda()
    mixer = maavss_amd.Mixer(_stft(), 2, (-5.0, 30.0))
    partners, snr = mixer.sample(tw.BATCH, torch.Generator().manual_seed(9))
    a = mixer(audio, seed=9, return_gain=True)
    b = mixer(audio, partners, snr, seed=9, return_gain=True)
    for u, v in zip(a, b):
        assert _same_bits(u, v)
    pool = sref.synthetic_audio(tw.POOL, tw.LENGTH, 12).cuda()
    partners, snr = mixer.sample(tw.BATCH, torch.Generator().manual_seed(9), pool_size=tw.POOL)
    for u, v in zip(mixer(audio, pool=pool, seed=9), mixer(audio, partners, snr, pool=pool, seed=9)):
        assert _same_bits(u, v)


# ---- ClipPipeline(mixer=): as tests/test_pipeline_gpu.py builds its extractor
T, W, FFT, HPF = 8, 128, 256, 8


def _pipeline_parts():
    from oracle import vit_ref_cpu as vref
    hop, length, _ = maavss_amd.calc_hop_size(T, HPF, 30, 16000)
    va = maavss_amd.VideoAttention(path_to_weights="/nonexistent.pth")
    va.load_state_dict(vref.seeded_vit_state(3))
    st = maavss_amd.STFT(FFT, hop, noise_std=0.1, device="cuda")
    frames = [vref.synthetic_frames(2 * T, W, 100 + i).cuda() for i in range(2)]
    return va, st, frames, length


@pytest.mark.parametrize("with_audio_transform", [False, True])
def test_pipeline_with_a_mixer_equals_the_serial_calls(with_audio_transform):
    va, st, frames, length = _pipeline_parts()
    mixer = maavss_amd.Mixer(st, 1, (0.0, 10.0))
    if with_audio_transform:
        at = maavss_amd.AudioTransform(16000)
        sr = 44100
        raw = [sref.synthetic_audio(2, at.input_length(length, sr) + 8, 200 + i, sr=sr).cuda() for i in range(2)]
        kw = dict(audio_transform=at, audio_length=length)
    else:
        raw = [sref.synthetic_audio(2, length, 200 + i).cuda() for i in range(2)]
        kw = {}
    serial = []
    for i in range(2):
        attn = va.attention_frames(frames[i], clip_frames=T).view(2, 1, T, W, W)
        clips = at(raw[i], sr, length=length, batched=True) if with_audio_transform else raw[i]
        x, y = mixer(clips, seed=i)
        serial.append((attn.clone(), x.clone(), y.clone()))
        assert not torch.equal(x, st(clips, seed=i)[0])                              # the mixer did mix
    pipe = maavss_amd.ClipPipeline(va, st, T, mixer=mixer, **kw)
    for i in range(2):                                                               # both batches in flight: depth-2 slots
        pipe.submit(frames[i], raw[i], seed=i, **(dict(audio_sr=sr) if with_audio_transform else {}))
    for i in range(2):
        x_v, x, y = pipe.get()
        assert torch.equal(x_v, serial[i][0]) and _same_bits(x, serial[i][1]) and _same_bits(y, serial[i][2]), i
        pipe.release()
    pipe.drain()
    # explicit partners / snr_db reach the mixer
    p, s = torch.tensor([[-1], [0]], dtype=torch.int32), torch.tensor([0.0, 20.0])
    pipe.submit(frames[0], raw[0], seed=0, partners=p, snr_db=s, **(dict(audio_sr=sr) if with_audio_transform else {}))
    _, x, y = pipe.get()
    clips = at(raw[0], sr, length=length, batched=True) if with_audio_transform else raw[0]
    xs, ys = mixer(clips, p, s, seed=0)
    assert _same_bits(x, xs) and _same_bits(y, ys)
    pipe.release()
    pipe.drain()


def test_pipeline_without_a_mixer_is_unchanged():
    va, st, frames, length = _pipeline_parts()
    audio = sref.synthetic_audio(2, length, 200).cuda()
    pipe = maavss_amd.ClipPipeline(va, st, T)
    pipe.submit(frames[0], audio, seed=3)
    _, x, y = pipe.get()
    xs, ys = st(audio, seed=3)
    assert _same_bits(x, xs) and _same_bits(y, ys)
    pipe.release()
    pipe.drain()
    with pytest.raises(ValueError, match="built with mixer="):
        pipe.submit(frames[0], audio, seed=3, partners=torch.tensor([[1], [0]], dtype=torch.int32))
