"""Torch CPU restatement of AV_Dataset.audio_transforms (av_dataset.py:203-215) for the AudioTransform tests: channel downmix,
the `normalize` line, torchaudio's sinc_interp_hann resampling in torchaudio's own formulation (a DENSE [new, 2 width + orig] kernel,
zero padding, conv1d with stride orig, transpose / reshape, crop) and contrast.  Every step runs in f32 or, with dtype=torch.float64,
in float64 on the same f32 taps and the same f32 input samples: that is the exact result the device kernel's f32 arithmetic is held to.
Test infrastructure, not a test module."""
import math

import torch
import torch.nn.functional as F


def to_float(x):
    """int16 PCM -> f32 in [-1, 1) as torchaudio.load(normalize=True) scales it (exact); f32 passes."""
    return x.to(torch.float32) / 32768 if x.dtype == torch.int16 else x


def downmix(x, dtype=torch.float32):
    """x [..., C, L] -> [..., L]: the reference's `audio /= C; audio.sum(dim=0)`; one channel passes unchanged."""
    x = to_float(x).to(dtype)
    c = x.shape[-2]
    return x[..., 0, :] if c == 1 else (x / c).sum(dim=-2)


def normalize(x):
    """av_dataset.py:209 as written: the clip TIMES its own max |x| (per clip = per row)."""
    return x * x.abs().amax(dim=-1, keepdim=True)


def sinc_kernel(orig, new, lowpass_filter_width=6, rolloff=0.99, rounded=True):
    """-> (dense kernel [new, 2 width + orig], width); orig, new already divided by their gcd.  float64, rounded to f32 unless
    rounded=False."""
    lpw = lowpass_filter_width
    base = min(orig, new) * rolloff
    width = math.ceil(lpw * orig / base)
    i = torch.arange(2 * width + orig, dtype=torch.float64)[None, :]
    p = torch.arange(new, dtype=torch.float64)[:, None]
    t = ((-p / new + (i - width) / orig) * base).clamp(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    tp = t * math.pi
    sinc = torch.where(tp == 0, torch.ones_like(tp), torch.sin(tp) / tp)
    k = sinc * (window * (base / orig))
    return (k.to(torch.float32) if rounded else k), width


def resample(x, orig, new, kernel, width, dtype=torch.float32):
    """x [B, L] -> [B, ceil(new L / orig)]: pad (width, width + orig), conv1d(stride=orig) with one output channel per phase,
    interleave the phases, crop."""
    b, length = x.shape
    xp = F.pad(x.to(dtype), (width, width + orig))
    y = F.conv1d(xp[:, None], kernel.to(dtype)[:, None, :], stride=orig)       # [B, new, J]
    y = y.transpose(1, 2).reshape(b, -1)
    return y[:, :-(-new * length // orig)]


def contrast(x):
    """torchaudio.functional.contrast(x, enhancement_amount=75)."""
    t = x * (math.pi / 2)
    return torch.sin(t + 0.1 * torch.sin(t * 4))


def chain(x, sr, samplerate=16000, compress_audio=False, normalize_clip=False, lowpass_filter_width=6, rolloff=0.99, length=None,
          dtype=torch.float32):
    """x [B, C, L0] f32 or int16 -> [B, L] in `dtype`, the four steps in the reference's order."""
    y = downmix(x, dtype)
    if normalize_clip:
        y = normalize(y)
    g = math.gcd(sr, samplerate)
    orig, new = sr // g, samplerate // g
    if orig != new:
        kernel, width = sinc_kernel(orig, new, lowpass_filter_width, rolloff)
        y = resample(y, orig, new, kernel, width, dtype)
    if compress_audio:
        y = contrast(y)
    return y if length is None else y[:, :length]


def signal(b, c, length, seed, dtype=torch.float32):
    """Seeded noise plus sinusoids, |x| <= 1, [B, C, L]; int16: the same, quantised."""
    g = torch.Generator().manual_seed(seed)
    n = torch.arange(length, dtype=torch.float64)
    x = 0.25 * torch.randn(b, c, length, generator=g, dtype=torch.float64)
    for k in range(3):
        f = torch.rand(b, c, 1, generator=g, dtype=torch.float64) * 0.2 + 0.003 * (k + 1)
        ph = torch.rand(b, c, 1, generator=g, dtype=torch.float64) * 2 * math.pi
        x = x + 0.2 * torch.sin(2 * math.pi * f * n + ph)
    x = x.clamp(-1, 1)
    if dtype == torch.int16:
        return (x * 32767).round().to(torch.int16)
    return x.to(torch.float32)
