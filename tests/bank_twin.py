"""TEST INFRASTRUCTURE ONLY -- restatement of maavss_amd.ClipBank's definitions (maavss_amd/clip_bank.py, include/maavss.h).

    pack     q = rint(min(max(v, 0), 1) * 65535)     one float32 product, rounded half to even; NaN -> 0
    unpack   v = q / 65535                            the correctly rounded float32 quotient
    index    clip k of a recording: frames [k*frame_hop, k*frame_hop + T), samples [s_k, s_k + n), s_k = round(k*frame_hop*sr/fps)
             on the exact fraction; a recording holds the longest prefix of clips that fit both its frames and its samples
    batch    clip = maps of the clip's frames (unpacked), with attn_diff the zero-padded temporal difference; each value x8 in both
             directions, zero outside the patch grid; times 1 / clip.max()

numpy float32 follows IEEE-754 in every operation used here (product, quotient, rint), so the first two are exact statements.
"""
from fractions import Fraction

import numpy as np
import torch

CRAFTED = [0.0, 1.0, 1.0 - 2.0 ** -24, 0.5 / 65535, 1.5 / 65535, 1e-8, -0.1, 1.1]
# What the rule gives for six of them, by hand.  1 - 2^-24 is a float32; its exact product with 65535 is 65535 - 0.00390619, the
# float32 grid there has step 2^-8 = 0.00390625, so the product rounds to 65535 - 2^-8 and rint gives 65535.  1e-8 * 65535 = 6.6e-4
# -> 0; -0.1 clamps to 0 and 1.1 to 1.  The two half-way values depend on how 0.5 / 65535 and 1.5 / 65535 round to float32:
# pack_exact decides them in rational arithmetic.
CRAFTED_BY_HAND = {0.0: 0, 1.0: 65535, 1.0 - 2.0 ** -24: 65535, 1e-8: 0, -0.1: 0, 1.1: 65535}


def pack(v):
    """float32 array -> uint16 array."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(v), np.float32(0), np.minimum(np.maximum(v, np.float32(0)), np.float32(1))).astype(np.float32)
    p = c * np.float32(65535)
    assert p.dtype == np.float32
    return np.rint(p).astype(np.uint16)


def unpack(q):
    """uint16 array -> float32 array."""
    out = np.asarray(q, dtype=np.uint16).astype(np.float32) / np.float32(65535)
    assert out.dtype == np.float32
    return out


def pack_exact(v):
    """The same rule in exact rational arithmetic on one float32 value: the float32 product is the exact product rounded to nearest
    even, which Fraction arithmetic and one numpy conversion from a float64 that holds it exactly give."""
    v = float(np.float32(v))
    c = min(max(v, 0.0), 1.0)
    exact = Fraction(c) * 65535                    # at most 24 + 16 significant bits: a float64 holds it exactly
    prod = np.float32(float(exact))                # one rounding to float32, half to even
    f = Fraction(float(prod))
    lo = f.numerator // f.denominator
    rest = f - lo
    return lo + (1 if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2) else 0)


def sample_start(k, frame_hop, fps, sr):
    return round(Fraction(k * frame_hop * sr, 1) / Fraction(fps))


def clips_brute_force(n_frames, n_samples, clip_frames, frame_hop, clip_samples, fps=30, sr=16000):
    """[(first frame, first sample)] of a recording's clips, by trying every k in turn."""
    out = []
    for k in range(n_frames + 1):
        v, s = k * frame_hop, sample_start(k, frame_hop, fps, sr)
        if v + clip_frames > n_frames or s + clip_samples > n_samples:
            break
        out.append((v, s))
    return out


def expected_attn(maps, size, attn_diff):
    """maps [T, (size//8)^2] float32 (a clip's unpacked maps, any device) -> [1, T, size, size]: the batch definition in torch ops."""
    t, hp = maps.shape[0], size // 8
    clip = maps.view(t, hp, hp)
    if attn_diff:
        clip = torch.cat([torch.zeros_like(clip[:1]), clip[1:] - clip[:-1]])
    up = clip.repeat_interleave(8, 1).repeat_interleave(8, 2)
    up = torch.nn.functional.pad(up, (0, size - 8 * hp, 0, size - 8 * hp))
    return (up * (1.0 / up.max()))[None]
