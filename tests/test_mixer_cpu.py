"""maavss_amd.Mixer without a device: every refusal of check(), the seeded sampler, the float64 twin's own consistency, the float32
chain against the gate the GPU tests use, and ClipPipeline's refusal of mixing arguments without a mixer."""
import math

import pytest
import torch

import maavss_amd
import mix_twin as tw
from maavss_amd import Mixer          # every test here, the twin's self-checks included, is about this class: none runs without it
from oracle import stft_ref_cpu as sref


def _mixer(k=2, snr=(0.0, 10.0), **kw):
    return Mixer(maavss_amd.STFT(512, tw.HOP, device="cpu", **kw), k, snr)


def test_exported_and_constructor_refusals():
    assert maavss_amd.Mixer is maavss_amd.mixer.Mixer is Mixer
    for k in (0, 5, -1, 2.0, True):
        with pytest.raises(ValueError, match="interferers"):
            _mixer(k)
    for rng in ((1.0, 0.0), (0.0, math.inf), (math.nan, 1.0)):
        with pytest.raises(ValueError, match="snr_db"):
            _mixer(1, rng)


def test_check_refusals():
    m = _mixer()
    audio = torch.zeros(3, tw.LENGTH)
    ok = torch.tensor([[1, 2], [0, -1], [-1, -1]], dtype=torch.int32)
    snr = torch.zeros(3)
    p, s = m.check(audio, ok, snr)
    assert p.dtype == torch.int32 and torch.equal(p, ok) and s.dtype == torch.float64 and tuple(s.shape) == (3,)
    assert torch.equal(m.check((3, tw.LENGTH), ok, 3.0)[1], torch.full((3,), 3.0, dtype=torch.float64))      # shape pair, scalar SNR
    with pytest.raises(ValueError, match="K must be in"):
        m.check(audio, torch.full((3, 5), -1, dtype=torch.int32), snr)
    with pytest.raises(ValueError, match="K must be in"):
        m.check(audio, torch.zeros(3, 0, dtype=torch.int32), snr)
    with pytest.raises(ValueError, match="int32"):
        m.check(audio, ok.long(), snr)
    with pytest.raises(ValueError, match="int32"):
        m.check(audio, ok[:2], snr)                                   # [2, K] for three clips
    with pytest.raises(ValueError, match="int32"):
        m.check(audio, ok[:, 0], snr)                                 # not 2-D
    with pytest.raises(ValueError, match=r"entries must be in \[-1, 3\)"):
        m.check(audio, torch.tensor([[1, 3], [0, -1], [-1, -1]], dtype=torch.int32), snr)
    with pytest.raises(ValueError, match=r"entries must be in \[-1, 3\)"):
        m.check(audio, torch.tensor([[1, 2], [0, -2], [-1, -1]], dtype=torch.int32), snr)
    with pytest.raises(ValueError, match="its own partner"):
        m.check(audio, torch.tensor([[1, 2], [0, 1], [-1, -1]], dtype=torch.int32), snr)
    pool = torch.zeros(2, tw.LENGTH)
    m.check(audio, torch.tensor([[0, 1], [1, -1], [-1, 0]], dtype=torch.int32), snr, pool)     # own pool: index b is another clip
    with pytest.raises(ValueError, match=r"entries must be in \[-1, 2\)"):
        m.check(audio, ok, snr, pool)
    with pytest.raises(ValueError, match="pool clips have 593 samples"):
        m.check(audio, ok, snr, torch.zeros(2, tw.LENGTH - 1))
    with pytest.raises(ValueError, match="pool must be float32"):
        m.check(audio, ok, snr, torch.zeros(2, tw.LENGTH, dtype=torch.float64))
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="finite"):
            m.check(audio, ok, torch.tensor([0.0, bad, 1.0]))
    with pytest.raises(ValueError, match="float32 can hold"):
        m.check(audio, ok, torch.tensor([0.0, -2000.0, 1.0]))
    with pytest.raises(ValueError, match=r"number or a \[3\]"):
        m.check(audio, ok, torch.zeros(2))
    with pytest.raises(ValueError, match="audio must be float32"):
        m.check(audio.double(), ok, snr)
    with pytest.raises(ValueError, match="audio must be float32"):
        m.check(torch.zeros(3, tw.LENGTH, 2)[:, :, 0], ok, snr)      # last stride 2
    with pytest.raises(ValueError, match="noise must be"):
        m.check(audio, ok, snr, noise=torch.zeros(3, 2, 9, 256))


def test_cpu_tensors_are_refused_like_every_other_op():
    with pytest.raises(maavss_amd._lib.MaavssError, match="no CPU fallback"):
        _mixer()(torch.zeros(3, tw.LENGTH))


@pytest.mark.parametrize("k", [1, 2, 4])
def test_sample(k):
    m = _mixer(k, (-5.0, 30.0))
    a = m.sample(16, torch.Generator().manual_seed(3))
    b = m.sample(16, torch.Generator().manual_seed(3))
    c = m.sample(16, torch.Generator().manual_seed(4))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    partners, snr = a
    assert partners.dtype == torch.int32 and tuple(partners.shape) == (16, k) and snr.dtype == torch.float32 and tuple(snr.shape) == (16,)
    assert bool(((snr.double() >= -5.0) & (snr.double() <= 30.0)).all())
    for b_ in range(16):
        row = partners[b_].tolist()
        assert b_ not in row and -1 not in row and len(set(row)) == k and all(0 <= p < 16 for p in row)
    m.check((16, tw.LENGTH), partners, snr)
    # candidates run out: -1 exactly in the slots past them
    p1, _ = m.sample(1, torch.Generator().manual_seed(0))
    assert p1.tolist() == [[-1] * k]
    p3, _ = m.sample(3, torch.Generator().manual_seed(0))
    for b_ in range(3):
        row = p3[b_].tolist()
        live = row[:min(k, 2)]
        assert sorted(live) == sorted(set(live)) and b_ not in live and all(0 <= p < 3 for p in live) and row[min(k, 2):] == [-1] * (k - min(k, 2))
    # an own pool: every row is a candidate, the clip's own index included
    pp, _ = m.sample(64, torch.Generator().manual_seed(1), pool_size=2)
    n = min(k, 2)
    assert all(set(r[:n]) <= {0, 1} and len(set(r[:n])) == n and r[n:] == [-1] * (k - n) for r in pp.tolist())
    if k == 1:
        assert {r[0] for r in pp.tolist()} == {0, 1}
    # a degenerate range draws the one value
    assert _mixer(k, (3.0, 3.0)).sample(4, torch.Generator().manual_seed(0))[1].tolist() == [3.0] * 4


def test_sample_is_uniform_over_the_other_clips():
    m = _mixer(1)
    g = torch.Generator().manual_seed(5)
    counts = torch.zeros(4, 4)
    for _ in range(600):
        p, _ = m.sample(4, g)
        for b in range(4):
            counts[b, int(p[b, 0])] += 1
    assert bool((counts.diagonal() == 0).all())
    off = counts[~torch.eye(4, dtype=torch.bool)]
    assert bool(((off - 200).abs() < 5 * math.sqrt(600 * (1 / 3) * (2 / 3))).all()), counts      # 5 sigma of Binomial(600, 1/3)


@pytest.mark.parametrize("own_pool,k", sorted(tw.PARTNERS))
def test_twin_realises_the_requested_snr(own_pool, k):
    audio, pool, partners, snr = tw.inputs(k, own_pool)
    src = audio if pool is None else pool
    g = tw.gain(audio, src, partners, snr)
    mix = tw.mixture(audio, src, partners, g)
    got = tw.realised_snr_db(audio, mix)
    live = (partners >= 0).any(1)
    assert bool((g[~live] == 0).all()) and bool((g[live] > 0).all())
    assert bool((mix[~live] == audio[~live].double()).all())
    assert float((got[live] - snr.double()[live]).abs().max()) < 1e-12
    # degenerate clips: zero target, zero interferer -> g == 0 exactly, nothing non-finite
    audio[1] = 0
    g = tw.gain(audio, src, partners, snr)
    pc, pi = tw.powers(audio, src, partners)
    assert bool(torch.isfinite(g).all()) and float(g[1]) == 0.0 and bool((g[(pi == 0) | (pc == 0)] == 0).all())


@pytest.mark.parametrize("fft_len,trim,norm,k,own_pool", tw.CASES)
def test_float32_chain_stays_inside_the_gpu_gate(fft_len, trim, norm, k, own_pool):
    """What tests/test_mixer_gpu.py holds the kernels to, applied to the same definition evaluated in torch float32 (torch.stft, f32 gain,
    f32 mix): the gate must leave room for float32 arithmetic on the chosen inputs before it is used to judge a kernel."""
    audio, pool, partners, snr = tw.inputs(k, own_pool)
    src = audio if pool is None else pool
    f = fft_len // 2 + (0 if trim else 1)
    noise = tw.noise_for(tw.BATCH, tw.LENGTH, tw.HOP, f)
    g64 = tw.gain(audio, src, partners, snr)
    x64, y64, term = tw.example(audio, src, partners, g64, fft_len, tw.HOP, tw.SIGMA, noise, trim=trim, normalize_output=norm)
    assert bool(torch.isfinite(x64).all())
    # float32 chain
    s32 = torch.zeros_like(audio)
    for kk in range(k):
        idx = partners[:, kk].long()
        s32 = s32 + torch.where((idx >= 0)[:, None], src[idx.clamp_min(0)], torch.zeros_like(audio))
    pc, pi = audio.pow(2).sum(1), s32.pow(2).sum(1)
    live = (partners >= 0).any(1) & (pc > 0) & (pi > 0)
    g32 = torch.where(live, torch.pow(10.0, -snr.double() / 20.0).float() * torch.sqrt(pc / pi.clamp_min(1e-30)), torch.zeros_like(pc))
    y32 = sref.stft_ref(audio, fft_len, tw.HOP, trim_stft_end=trim)
    i32 = sref.stft_ref(s32, fft_len, tw.HOP, trim_stft_end=trim)
    c32 = torch.ones(tw.BATCH)
    if norm:
        c32 = 1.0 / (y32.abs().flatten(1).max(1).values + 1e-7)
        y32 = y32 * c32[:, None, None, None]
    x32 = y32 + (g32 * c32)[:, None, None, None] * i32 + tw.SIGMA * noise
    tol = tw.gate(norm) * float(x64.abs().max()) + tw.gain_bound(audio, src, partners)[:, None, None, None] * term.abs()
    assert bool(((x32.double() - x64).abs() <= tol).all()), float(((x32.double() - x64).abs() / tol).max())
    assert float((y32.double() - y64).abs().max()) <= tw.gate(norm) * float(y64.abs().max())


def test_pipeline_without_a_mixer_refuses_mixing_arguments():
    """A ClipPipeline without its side stream (the constructor opens one on the device): the host-side checks only."""
    pipe = object.__new__(maavss_amd.ClipPipeline)
    pipe.mixer = None
    audio = torch.zeros(2, tw.LENGTH)
    assert pipe.check_mix(audio, None, 0, None, None) == (None, None)
    with pytest.raises(ValueError, match="built with mixer="):
        pipe.check_mix(audio, None, 0, torch.tensor([[1], [0]], dtype=torch.int32), None)
    with pytest.raises(ValueError, match="built with mixer="):
        pipe.check_mix(audio, None, 0, None, torch.zeros(2))
    # with one: the seeded draw is the one Mixer.__call__ makes, and explicit arguments go through check()
    pipe.mixer = _mixer(1)
    p, s = pipe.check_mix(audio, None, 7, None, None)
    want = pipe.mixer.sample(2, torch.Generator().manual_seed(7))
    assert torch.equal(p, want[0]) and torch.equal(s, want[1].double())
    with pytest.raises(ValueError, match="its own partner"):
        pipe.check_mix(audio, None, 7, torch.tensor([[0], [0]], dtype=torch.int32), None)
    st = maavss_amd.STFT(512, tw.HOP, device="cpu")
    with pytest.raises(ValueError, match="same STFT|STFT object"):
        maavss_amd.ClipPipeline(None, st, 8, mixer=_mixer(1))


def test_entry_points_refuse_an_output_that_overlaps_an_input():
    """maavss_mix_wave and maavss_stft_mix_fwd read rows that other workgroups write if an output overlaps an input: refused from the
    addresses alone, before any launch (the addresses here are never dereferenced)."""
    from maavss_amd import _lib
    b, length = 4, 100
    rows = 4 * b * length                                                              # bytes of [4, 100] float32
    wave = dict(audio=0x10000, batch=b, length=length, audio_stride=length, pool=0x20000, n_pool=b, pool_stride=length, partners=0x30000,
                k_slots=2, gain=0x40000, mixture=0x50000, mixture_stride=length, stream=None)
    for kw in (dict(mixture=0x10000), dict(mixture=0x10000 + rows - 4), dict(mixture=0x10000 - rows + 4), dict(mixture=0x20000),
               dict(pool=0x10000, mixture=0x10000 + 4 * length), dict(mixture=0x20000 + 4, mixture_stride=2 * length)):
        with pytest.raises(_lib.MaavssError, match="mixture overlaps audio or pool"):
            _lib.call("maavss_mix_wave", *{**wave, **kw}.values())
    frames, bins = tw.LENGTH // tw.HOP, 129
    spec = 4 * b * 2 * frames * bins
    mix = dict(pool=0x10000, n_pool=b, length=tw.LENGTH, pool_stride=tw.LENGTH, partners=0x30000, k_slots=2, batch=b, window=0x40000, n_fft=256,
               hop=tw.HOP, n_frames=frames, n_bins_out=bins, y=0x100000, x=0x200000, noise=None, sigma=0.0, seed=0, gain=0x50000,
               clip_absmax=None, stream=None)
    for kw in (dict(x=0x100000), dict(x=0x100000 + spec - 4), dict(x=0x100000 - spec + 4), dict(x=0x10000 + 4 * tw.LENGTH),
               dict(noise=0x200000 + spec - 4)):
        with pytest.raises(_lib.MaavssError, match="x overlaps y, noise or pool"):
            _lib.call("maavss_stft_mix_fwd", *{**mix, **kw}.values())
