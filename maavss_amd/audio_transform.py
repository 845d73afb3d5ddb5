"""AV_Dataset.audio_transforms on the GPU (av_dataset.py:203-215, called at :294 and :299): the demuxer's PCM -- any rate, any channel
count, f32 or int16 -- -> channel downmix [-> normalize] -> torchaudio's sinc_interp_hann Resample to `samplerate` [-> contrast], as
the mono f32 [B, L] clips STFT reads.  The rate change the reference leaves to `ffmpeg -ar 16000` (utilities.py:69-71) is the same
stage.  The kernels are maavss_audio_transform (include/maavss.h); the polyphase tap table is built on the host, in float64 rounded to
f32 as torchaudio.transforms.Resample does, and kept compressed: only the taps inside the window's support are stored."""
import math

import torch

from . import _lib

MAX_TABLE = 1 << 22          # taps of a compressed table (16 MiB)
_RUN = 256                   # outputs per workgroup of maavss_audio_transform (AT_RUN)
_MAX_SPAN = 16384            # input samples a workgroup can stage (AT_MAX_LDS / 4)


def _pos_int(name, v):
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"{name} must be a positive integer, got {v!r}")
    return v


def sinc_table(orig, new, lowpass_filter_width=6, rolloff=0.99):
    """Compressed sinc_interp_hann table for orig -> new (already divided by their gcd) -> (taps f32 [new, S], first int32 [new], S,
    width), all on the CPU: tap k of phase p is dense tap first[p] + k of torchaudio's kernel, whose row has 2 * width + orig taps.
    The dense tap is sinc(pi t) cos^2(pi t / (2 lpw)) base / orig at t = clamp((-p / new + (i - width) / orig) base, -lpw, lpw) in
    float64, rounded to f32; at |t| = lpw that is exactly 0.0 in f32, so only the at most S = ceil(2 lpw orig / base) taps with
    |t| < lpw are kept.  The dense table is never formed."""
    lpw = lowpass_filter_width
    base = min(orig, new) * rolloff
    width = math.ceil(lpw * orig / base)
    s = math.ceil(2 * lpw * orig / base)
    if new * s > MAX_TABLE:
        raise ValueError(f"resampling {orig} -> {new} (rates divided by their gcd) needs a table of {new} x {s} taps, more than 2^22")
    p = torch.arange(new, dtype=torch.float64)[:, None]
    # first tap of the support: the smallest i with t > -lpw.  A float64 guess one below it, then the exact test on the same t the
    # taps are made of.
    guess = torch.floor(width + orig * p / new - lpw * orig / base) - 1
    cand = guess + torch.arange(4, dtype=torch.float64)[None, :]
    inside = ((-p / new + (cand - width) / orig) * base).abs() < lpw
    if not bool((inside.any(dim=1) & ~inside[:, 0]).all()):
        raise ValueError(f"resampling {orig} -> {new}: could not place the window support")
    first = guess[:, 0] + inside.to(torch.int64).argmax(dim=1)
    i = first[:, None] + torch.arange(s, dtype=torch.float64)[None, :]
    t_raw = (-p / new + (i - width) / orig) * base
    t = t_raw.clamp(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    tp = t * math.pi
    sinc = torch.where(tp == 0, torch.ones_like(tp), torch.sin(tp) / tp)
    taps = (sinc * (window * (base / orig))).to(torch.float32)
    # a tap past the dense row's end (i >= 2 width + orig) would read beyond torchaudio's right padding: it must be a dead one
    if bool((taps[(i >= 2 * width + orig) | (i < 0)] != 0).any()):
        raise ValueError(f"resampling {orig} -> {new}: live tap outside the dense row")
    first = first.to(torch.int32)
    # what the kernel's staging relies on: the first taps of outputs n and n + RUN - 1 are at most ceil((RUN - 1) orig / new) + 1 apart
    n = torch.arange(new + _RUN, dtype=torch.int64)
    start = (n // new) * orig + first.to(torch.int64)[n % new]
    if bool((start[1:] < start[:-1]).any()) or int((start[_RUN - 1:] - start[:new + 1]).max()) > -(-(_RUN - 1) * orig // new) + 1:
        raise ValueError(f"resampling {orig} -> {new}: tap support is not monotone")
    return taps.contiguous(), first.contiguous(), s, width


class AudioTransform:
    """`t = AudioTransform(samplerate=16000)`; `clips = t(audio, sr, length=L)` -> f32 [B, L] on the device.

    In the reference's order (av_dataset.py:204-214): (1) C > 1 channels: every channel divided by C, then summed; (2) normalize=True:
    the clip is MULTIPLIED by its own max |x| -- this is the reference's line 209 as written (`audio *= audio.abs().max()`), kept for
    parity; it is not a peak normalisation, and the reference never switches it on; (3) sr != samplerate: torchaudio's
    sinc_interp_hann Resample(sr, samplerate, lowpass_filter_width, rolloff), otherwise the samples pass through bit-unchanged;
    (4) compress_audio=True: torchaudio.functional.contrast(x, 75) = sin(x pi/2 + 0.1 sin(4 x pi/2)).  int16 input is scaled by 2^-15
    first, as torchaudio.load(normalize=True) does."""

    def __init__(self, samplerate=16000, compress_audio=False, normalize=False, lowpass_filter_width=6, rolloff=0.99, device="cuda"):
        self.samplerate = _pos_int("samplerate", samplerate)
        self.lowpass_filter_width = _pos_int("lowpass_filter_width", lowpass_filter_width)
        if isinstance(rolloff, bool) or not isinstance(rolloff, (int, float)) or not 0 < rolloff <= 1:
            raise ValueError(f"rolloff must be in (0, 1], got {rolloff!r}")
        self.rolloff = float(rolloff)
        self.compress_audio, self.normalize = bool(compress_audio), bool(normalize)
        self.device = torch.device(device)
        self._tables = {}            # (orig, new) -> CPU table; (orig, new, device) -> device copies

    def _ratio(self, sr):
        g = math.gcd(_pos_int("sr", sr), self.samplerate)
        return sr // g, self.samplerate // g

    def output_length(self, n_in, sr):
        orig, new = self._ratio(sr)
        return -(-int(n_in) * new // orig)

    def input_length(self, n_out, sr):
        """ceil(n_out orig / new): enough input for n_out samples (output_length(input_length(n), sr) >= n)."""
        orig, new = self._ratio(sr)
        return -(-int(n_out) * orig // new)

    def table(self, sr):
        """-> (taps f32 [new, S], first int32 [new], S, width) on the CPU for sr -> samplerate (sinc_table), built once per rate pair."""
        orig, new = self._ratio(sr)
        if orig == new:
            raise ValueError(f"sr = {sr} equals the output rate: no table")
        key = (orig, new)
        if key not in self._tables:
            tab = sinc_table(orig, new, self.lowpass_filter_width, self.rolloff)
            span = -(-(_RUN - 1) * orig // new) + 2 + tab[2]
            if span > _MAX_SPAN:
                raise ValueError(f"resampling sr = {sr} -> {self.samplerate}: the rate ratio is too large for the kernel "
                                 f"({span} staged samples per workgroup, at most {_MAX_SPAN})")
            self._tables[key] = tab
        return self._tables[key]

    def _device_table(self, sr, dev):
        orig, new = self._ratio(sr)
        key = (orig, new, dev)
        if key not in self._tables:
            taps, first, s, width = self.table(sr)
            # tap-major on the device: the lanes of a wave (consecutive phases) read consecutive floats
            self._tables[key] = (taps.t().contiguous().to(dev), first.to(dev), s, width)
        return self._tables[key]

    def check(self, audio, sr, length=None, out=None, batched=False):
        """Host-side validation (no device work) -> (audio as a [B, C, L0] view, L).  batched=True reads a 2-D input as [B, L0] mono
        clips (ClipPipeline) instead of [C, L0]."""
        self._ratio(sr)
        if not isinstance(audio, torch.Tensor) or audio.dtype not in (torch.float32, torch.int16):
            raise ValueError(f"audio must be a float32 or int16 tensor, got {getattr(audio, 'dtype', type(audio))}")
        if audio.dim() not in (1, 2, 3):
            raise ValueError(f"audio must be [L0], [C, L0] or [B, C, L0], got {tuple(audio.shape)}")
        if audio.dim() == 1:
            audio = audio[None, None]
        elif audio.dim() == 2:
            audio = audio[:, None] if batched else audio[None]
        b, c, l0 = audio.shape
        if b < 1 or c < 1 or l0 < 1:
            raise ValueError(f"audio needs at least one clip, one channel and one sample, got [B, C, L0] = {tuple(audio.shape)}")
        if audio.stride(2) != 1 or audio.stride(0) < 0 or audio.stride(1) < 0:
            raise ValueError(f"audio layout: the last stride must be 1 and none negative, got strides {audio.stride()}")
        full = self.output_length(l0, sr)
        if length is None:
            length = full
        elif isinstance(length, bool) or not isinstance(length, int) or length < 1:
            raise ValueError(f"length must be a positive integer, got {length!r}")
        elif length > full:
            raise ValueError(f"length = {length} exceeds the {full} samples that {l0} samples at {sr} Hz resample to")
        if sr != self.samplerate:
            self.table(sr)               # refuses rate pairs the kernel cannot serve
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (b, length):
                raise ValueError(f"out must be a float32 [{b}, {length}] tensor, got {getattr(out, 'dtype', type(out))} "
                                 f"{tuple(getattr(out, 'shape', ()))}")
            if out.stride(1) != 1 or (b > 1 and out.stride(0) < length):
                raise ValueError(f"out layout: rows of stride 1 that do not overlap, got strides {out.stride()}")
            if out.device != audio.device:
                raise ValueError(f"out is on {out.device}, audio on {audio.device}")
        return audio, length

    def __call__(self, audio, sr, length=None, out=None, batched=False):
        """audio: [L0], [C, L0] (torchaudio.load's layout) or [B, C, L0], float32 or int16, on the device, last stride 1; sr: its rate.
        -> f32 [B, length] (default length: output_length(L0, sr)), into `out` when given (returned as is).  Everything is checked
        before any device work; all work goes to the current stream, at most two kernel launches."""
        audio, length = self.check(audio, sr, length, out, batched)
        _lib.require_cuda(audio, out)
        dev = audio.device
        if self.device.index is not None and dev != self.device:
            raise ValueError(f"audio is on {dev}, the transform was built for {self.device}")
        b, c, l0 = audio.shape
        orig, new = self._ratio(sr)
        taps = first = None
        s = width = 0
        if orig != new:
            taps, first, s, width = self._device_table(sr, dev)
        if out is None:
            out = torch.empty(b, length, device=dev, dtype=torch.float32)
        nbytes = _lib.query("maavss_audio_transform_ws_bytes", b, c, l0, int(self.normalize))
        if nbytes < 0:
            raise ValueError(f"unsupported audio shape [B, C, L0] = {(b, c, l0)}")
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
        _lib.call("maavss_audio_transform", _lib.ptr(audio), int(audio.dtype == torch.int16), b, c, l0, audio.stride(0), audio.stride(1),
                  _lib.ptr(taps), _lib.ptr(first), orig, new, s, width, int(self.normalize), int(self.compress_audio), _lib.ptr(out),
                  length, out.stride(0) if b > 1 else length, _lib.ptr(ws), nbytes, _lib.stream_ptr())
        return out
