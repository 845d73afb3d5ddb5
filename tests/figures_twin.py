"""Float64 restatement of csrc/figures.hip (numpy only): the contract of maavss_amd.figures.  Written from the definitions in
include/maavss.h, not from matplotlib's source; tests/test_figures_cpu.py holds it to matplotlib itself (the colour mapping byte for
byte, the spectrogram planes to 1e-12), tests/test_figures_gpu.py holds the kernels to it.

The list of spectrogram cases of the GPU tests is here, with fixed seeds.  The seeds were CHOSEN (scripts/figures_parity.py --seeds
searches them on the CPU) so that no case has an unwrap decision or more than a handful of pixels within M = 1e-5 of a boundary:
test_figures_cpu.py checks that, and the GPU gate (1e-6 and below) then decides nothing differently from the twin."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUT_HEADER = os.path.join(ROOT, "maavss_amd", "csrc", "viridis_lut.h")
M = 1e-5                                   # decision margin: radians for an unwrap decision, LUT-index units for a pixel


def read_lut(path=LUT_HEADER):
    """The 256 x 3 table of csrc/viridis_lut.h."""
    text = open(path).read()
    text = text[text.index("viridis_lut[VIRIDIS_N][3]"):]
    rows = re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\}", text)
    lut = np.array(rows, dtype=np.int64)
    assert lut.shape == (256, 3) and lut.max() <= 255, lut.shape
    return lut.astype(np.uint8)


_LUT = None


def lut():
    global _LUT
    if _LUT is None:
        _LUT = read_lut()
    return _LUT


# ---- colour mapping -------------------------------------------------------------------------------------------------------------------

def finite_range(x):
    """(min, max) over the finite elements; (+inf, -inf) when there is none."""
    x = np.asarray(x, dtype=np.float64)
    f = x[np.isfinite(x)]
    return (float(f.min()), float(f.max())) if f.size else (np.inf, -np.inf)


def scaled_index(x, vmin=None, vmax=None):
    """256 u of every element (float64; whatever for a non-finite one) and the range used."""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = finite_range(x)
    lo = lo if vmin is None else float(vmin)
    hi = hi if vmax is None else float(vmax)
    with np.errstate(all="ignore"):
        u = np.zeros_like(x) if hi == lo else (x - lo) / (hi - lo)
        return u * 256.0, lo, hi


def viridis_image(x, vmin=None, vmax=None, transpose=False, flip_rows=False, scale=(1, 1)):
    """One image [H, W] (any float dtype) -> uint8 [H sy, W sx, 4]."""
    x = np.asarray(x)
    assert x.ndim == 2
    x = x.astype(np.float64)
    if transpose:
        x = x.T
    if flip_rows:
        x = x[::-1]
    s, _, _ = scaled_index(x, vmin, vmax)
    ok = np.isfinite(x)
    with np.errstate(all="ignore"):
        idx = np.clip(np.trunc(np.where(ok, s, 0.0)), 0, 255).astype(np.int64)
    out = np.zeros(x.shape + (4,), dtype=np.uint8)
    out[..., :3] = lut()[idx]
    out[..., 3] = 255
    out[~ok] = 0
    return np.repeat(np.repeat(out, scale[0], axis=0), scale[1], axis=1)


def boundary_margin(x, vmin=None, vmax=None):
    """Distance of every finite pixel's 256 u from the nearest integer (a colour boundary), float64 [H, W]; +inf for the pixels that are
    decided whatever the rounding: non-finite ones, those equal to the image's own minimum or maximum (u is exactly 0 or 1), and those
    clamped from outside [0, 256] by at least 1."""
    x = np.asarray(x, dtype=np.float64)
    s, lo, hi = scaled_index(x, vmin, vmax)
    with np.errstate(all="ignore"):
        d = np.abs(s - np.rint(s))
    d[~np.isfinite(x)] = np.inf
    if vmin is None:
        d[x == lo] = np.inf
    if vmax is None:
        d[x == hi] = np.inf
    with np.errstate(all="ignore"):
        d[(s < -1.0) | (s > 257.0)] = np.inf
    return d


# ---- spectrogram planes ---------------------------------------------------------------------------------------------------------------

def segments(length, nfft, noverlap):
    return (max(length, nfft) - noverlap) // (nfft - noverlap)


def hann(nfft):
    """The symmetric Hann window, 0.5 - 0.5 cos(2 pi k / (nfft - 1)), in the form numpy evaluates: 0.5 + 0.5 cos(pi n / (nfft - 1)),
    n = 2 k + 1 - nfft."""
    n = np.arange(1 - nfft, nfft, 2, dtype=np.float64)
    return 0.5 + 0.5 * np.cos(np.pi * n / (nfft - 1))


def _columns(x, nfft, noverlap):
    """One-sided transforms of the windowed segments: complex128 [nfft / 2 + 1, n], and sum(w)."""
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim == 1
    if x.size < nfft:
        x = np.concatenate([x, np.zeros(nfft - x.size)])
    step, n = nfft - noverlap, segments(x.size, nfft, noverlap)
    w = hann(nfft)
    seg = np.stack([x[i * step:i * step + nfft] for i in range(n)], axis=1)          # [nfft, n]
    with np.errstate(all="ignore"):
        spec = np.fft.fft(seg * w[:, None], axis=0)[:nfft // 2 + 1]
    return spec, w.sum()


def unwrap_terms(p):
    """p [bins, n] -> (dd, correction) of the unwrap along axis 0, both [bins - 1, n]."""
    with np.errstate(all="ignore"):
        dd = np.diff(p, axis=0)
        m = np.mod(dd + np.pi, 2 * np.pi) - np.pi
        m[(m == -np.pi) & (dd > 0)] = np.pi
        c = m - dd
        c[np.abs(dd) < np.pi] = 0.0
    return dd, c


def specgram_planes(x, nfft=256, noverlap=128):
    """One row x [L] -> (mag_db, phase), float64 [nfft / 2 + 1, n], row 0 the Nyquist bin."""
    spec, wsum = _columns(x, nfft, noverlap)
    with np.errstate(all="ignore"):
        mag = 20.0 * np.log10(np.abs(spec) / wsum)
        p = np.angle(spec)
        _, c = unwrap_terms(p)
        phase = p.copy()
        phase[1:] = p[1:] + np.cumsum(c, axis=0)
    return mag[::-1].copy(), phase[::-1].copy()


def unwrap_margin(x, nfft=256, noverlap=128):
    """The smallest | |dd| - pi | over the unwrap decisions of a row's finite columns (+inf when there is none)."""
    spec, _ = _columns(x, nfft, noverlap)
    with np.errstate(all="ignore"):
        dd, _ = unwrap_terms(np.angle(spec))
    dd = dd[np.isfinite(dd)]
    return float(np.abs(np.abs(dd) - np.pi).min()) if dd.size else np.inf


def specgram_images(x, nfft=256, noverlap=128, scale=(1, 1)):
    mag, phase = specgram_planes(x, nfft, noverlap)
    return viridis_image(mag, scale=scale), viridis_image(phase, scale=scale)


def undecided_cap(pixels):
    return max(2, pixels / 32768)


# ---- the reference's composites -------------------------------------------------------------------------------------------------------

def stft_panels(y_stft, yh_stft):
    """[2, T_a, F] x 2 -> uint8 [4, F, T_a, 4]."""
    return np.stack([viridis_image(p, transpose=True) for p in (y_stft[0], y_stft[1], yh_stft[0], yh_stft[1])])


def scale_clip(t):
    """The reference's scale and clip in float32: s = 1 / (max + 1e-7), v s, clipped to [0, 1]."""
    t = np.asarray(t, dtype=np.float32)
    s = np.float32(1.0) / (np.float32(t.max()) + np.float32(1e-7))
    return np.clip(t * s, np.float32(0.0), np.float32(1.0)).astype(np.float32)


def _strip(frames):
    """[T, H, W] -> [H, T W]: the frames side by side."""
    return np.concatenate(list(frames), axis=1)


def filmstrip_image(y_attn, yh_attn, video=None):
    """[1, T, H, W] x 2 and [3, T, H, W] or None -> uint8 [R H, T W, 4]; the inputs are not modified."""
    rows = []
    if video is not None:
        v = scale_clip(video)
        rgb = np.stack([_strip(v[c]) for c in range(3)], axis=-1)                       # [H, T W, 3] float32
        img = np.full(rgb.shape[:2] + (4,), 255, dtype=np.uint8)
        img[..., :3] = np.trunc(rgb * np.float32(255.0)).astype(np.uint8)
        rows.append(img)
    for a in (y_attn, yh_attn):
        rows.append(viridis_image(_strip(scale_clip(a)[0]), vmin=-1.0, vmax=1.0))
    return np.concatenate(rows, axis=0)


# ---- the spectrogram cases of the GPU tests ---------------------------------------------------------------------------------------------

LENGTHS = (100, 256, 383, 384, 1000, 8448)
PARAMS = ((64, 0), (64, 63), (256, 128), (512, 128), (1024, 512))
# seed of the noise of case (length, nfft, noverlap); chosen by scripts/figures_parity.py --seeds, see the module docstring
SEEDS = {(length, nfft, noverlap): 0 for length in LENGTHS for nfft, noverlap in PARAMS}
SEEDS.update({(8448, 64, 63): 68, (8448, 256, 128): 1})      # seeds 0 .. 67 (0) put a decision or too many pixels within M of a boundary


def tone_noise(length, seed):
    """0.3 sin(2 pi 440 t) + 0.1 randn at 16 kHz, float32."""
    g = np.random.default_rng(seed)
    t = np.arange(length, dtype=np.float64) / 16000.0
    return (0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.1 * g.standard_normal(length)).astype(np.float32)


def gpu_cases():
    """-> [(name, x float32 [L], nfft, noverlap)]: every length with every (nfft, noverlap), and the special rows."""
    out = []
    for length in LENGTHS:
        for nfft, noverlap in PARAMS:
            out.append((f"L{length}_n{nfft}_o{noverlap}", tone_noise(length, SEEDS[(length, nfft, noverlap)]), nfft, noverlap))
    for name, x in special_rows().items():
        out.append((name, x, 256, 128))
    return out


SPECIAL_SEEDS = {"silent": 0, "nan": 0, "overlap": 0}


def special_row(name):
    """Rows of 2000 samples at (256, 128): a silent stretch that covers whole segments (-inf dB, phase 0), or a NaN sample."""
    x = tone_noise(2000, SPECIAL_SEEDS[name])
    if name == "silent":
        x[500:1100] = 0.0                        # segments 4 .. 6 (samples 512 .. 1023) are silent, their neighbours partly
    else:
        x[700] = np.nan                          # segments 4 and 5
    return x


def special_rows():
    return {name: special_row(name) for name in ("silent", "nan")}


# overlapping rows and a row at an odd 4-byte offset: rows of one signal, ROWS x N from OFF with stride STRIDE < N
OVERLAP = dict(rows=3, n=1000, stride=333, off=3, length=3 + 2 * 333 + 1000, nfft=256, noverlap=128)


def overlap_signal():
    return tone_noise(OVERLAP["length"], SPECIAL_SEEDS["overlap"])


def overlap_rows():
    o, sig = OVERLAP, overlap_signal()
    return np.stack([sig[o["off"] + r * o["stride"]:o["off"] + r * o["stride"] + o["n"]] for r in range(o["rows"])])


def case_margins(x, nfft, noverlap):
    """-> dict(unwrap=smallest unwrap margin, mag=(undecided pixels, pixels), phase=(...)) of one row."""
    mag, phase = specgram_planes(x, nfft, noverlap)
    res = dict(unwrap=unwrap_margin(x, nfft, noverlap))
    for key, plane in (("mag", mag), ("phase", phase)):
        res[key] = (int((boundary_margin(plane) < M).sum()), plane.size)
    return res


def case_ok(x, nfft, noverlap):
    m = case_margins(x, nfft, noverlap)
    return m["unwrap"] >= M and all(m[k][0] <= undecided_cap(m[k][1]) for k in ("mag", "phase"))
