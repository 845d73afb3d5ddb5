"""Whole-recording inference: video frames (or per-frame attention maps) and noisy audio -> enhanced waveform.

The reference turns a trained `AV_Fusion_Model_Frames` into audio only inside its training callbacks
(train_avse_frames.py:139-176,196-200: the `num_seq` window outputs stitched into `output_stft`, then `dataset.istft`;
train_av_net.py:147-186: `model.eval()` + `torch.no_grad()` over held-out clips).  `Enhancer` does the same over a whole
recording, every step a HIP kernel.  Definition (the contract tests/test_enhance_*.py check), with a = hops_per_frame,
h = stft.hop, n = num_frames, s = num_seq:

1. Training clip: T_c = n + s frames (train_avse_frames.py:31) and a*h*T_c samples (calc_hop_size).
2. Audio-clocked tiling: clip c takes samples [c*s*a*h, c*s*a*h + a*h*T_c) and the T_c video frames from
   v_c = round(c*s*a*h * fps / sr) (Python's round, exact rational arithmetic: the inverse of the pairing at
   av_dataset.py:285-289).  C = the largest clip count for which both audio and frames suffice.  Clip c's STFT frame k is
   centred at sample (c*s*a + k)*h, so all clips lie on one global hop grid, the stitched STFT has no gap and a single inverse
   gives a seamless waveform; when sr / fps == a*h exactly, v_c = c*s.  Audio and not video sets the clock because the hop
   grid lives in samples: with the reference's 16 kHz / 30 fps / a = 8, a*h = 528 samples is not the 533.3 of one video frame,
   so clips starting on video frames would leave gaps in the audio.
3. Per clip, exactly the training example: the attention frames that
   `VideoAttention.attention_frames(frames[v_c : v_c + T_c], clip_frames=T_c, attn_diff=attn_diff)` gives (av_dataset.py:
   321-328), and Y_c = STFT of the clip's samples divided by g_c = max|Y_c| + 1e-7 when `stft.normalize_output_fft`
   (av_dataset.py:337-340), else g_c = 1.  No noise is added (`stft.noise_std` is ignored).
4. Windows: window j < s of clip c takes the clip's frames [j, j+n) and STFT frames [a*j, a*(j+n)) (train_avse_frames.py:
   150-163); the model's audio output [2, a, F], times g_c, becomes stitched STFT frames a*(c*s + j) .. a*(c*s + j + 1) - 1.
5. Output: wave = stft.inverse(stitched), h*(C*s*a - 1) samples; start = target_offset*a*h is the sample of `audio` that
   wave[0] corresponds to (window j predicts clip frame j + target_offset).

The ViT runs once per recording frame (clips overlap by n frames; per-clip extraction would repeat its work T_c / s times):
maavss_vit_attn_maps_pass1 keeps each frame's map at patch resolution, and maavss_av_attn_windows cuts, normalises and upsamples
the window batch from those.  One maavss_stft_fwd launch covers all clips as overlapping rows of `audio`; maavss_av_stft_windows
gathers the model's audio input, and maavss_av_stitch writes its output times g_c where STFT.inverse reads it.
"""
from fractions import Fraction

import torch

from . import _lib
from .avse import AV_Fusion_Model_Frames
from ._lib import call, ptr, stream_ptr


def clip_tiling(n_samples, n_frames, num_frames, num_seq, hops_per_frame, hop, fps=30, sr=16000):
    """Step 2 of the module docstring on the host -> (C, [v_0 .. v_{C-1}]).  C = 0 when the recording holds no whole clip."""
    clip_frames = num_frames + num_seq
    clip_len = hops_per_frame * hop * clip_frames
    step = num_seq * hops_per_frame * hop
    rate = Fraction(fps) / Fraction(sr)
    starts = []
    c = 0
    while c * step + clip_len <= n_samples:
        v = round(c * step * rate)
        if v + clip_frames > n_frames:
            break
        starts.append(v)
        c += 1
    return len(starts), starts


class Enhancer:
    """`enh = Enhancer(model, stft, num_frames, num_seq, hops_per_frame, video_attention=..)`; `wave, start = enh(audio, frames=..)`
    or `enh(audio, attn=..)`.  See the module docstring for what is computed.

    model: a trained AV_Fusion_Model_Frames in eval mode; stft: the STFT it was trained with; num_frames, num_seq, hops_per_frame:
    as in the reference's run_config.py.  target_offset: the clip frame window j predicts is j + target_offset (default the
    reference's idx_middle_frame = (num_seq - 1) // 2, train_avse_frames.py:105).  windows_per_launch: windows per model forward
    (default the model's constructed batch, frame_shape[0]); the window buffers are allocated once per call and reused."""

    def __init__(self, model, stft, num_frames, num_seq, hops_per_frame, *, video_attention=None, fps=30, sr=16000, attn_diff=False,
                 target_offset=None, windows_per_launch=None, audio_transform=None):
        if not isinstance(model, AV_Fusion_Model_Frames):
            raise ValueError(f"model must be an AV_Fusion_Model_Frames, got {type(model).__name__}")
        n, s, a = int(num_frames), int(num_seq), int(hops_per_frame)
        if n < 1 or s < 1 or a < 1:
            raise ValueError("num_frames, num_seq and hops_per_frame must be positive")
        if model.t_v != n:
            raise ValueError(f"the model was built for windows of {model.t_v} frames, not num_frames={n}")
        if model.output_stft_frames != a or model.t_a != a * n:
            raise ValueError(f"the model was built for {model.t_a} STFT frames in and {model.output_stft_frames} out per window, not "
                             f"hops_per_frame={a} x num_frames={n}")
        if model.n_bins != stft.n_bins():
            raise ValueError(f"the model was built for {model.n_bins} frequency bins, the STFT gives {stft.n_bins()}")
        if not (fps > 0 and sr > 0):
            raise ValueError("fps and sr must be positive")
        self.target_offset = (s - 1) // 2 if target_offset is None else int(target_offset)
        if not 0 <= self.target_offset <= n:
            raise ValueError(f"target_offset={self.target_offset}: window j must predict a frame j + target_offset of its clip "
                             f"(0 <= target_offset <= num_frames={n})")
        wpl = model.frame_shape[0] if windows_per_launch is None else int(windows_per_launch)
        if wpl < 1:
            raise ValueError("windows_per_launch must be positive")
        if audio_transform is not None and audio_transform.samplerate != sr:
            raise ValueError(f"audio_transform resamples to {audio_transform.samplerate} Hz, the Enhancer runs at sr={sr}")
        self.audio_transform = audio_transform
        self.model, self.stft, self.video_attention = model, stft, video_attention
        self.num_frames, self.num_seq, self.hops_per_frame = n, s, a
        self.fps, self.sr, self.attn_diff, self.windows_per_launch = fps, sr, bool(attn_diff), wpl
        self.clip_frames = n + s
        self.clip_samples = a * stft.hop * self.clip_frames
        self._marks = None          # list -> (stage, CUDA event) at stage boundaries (scripts/enhance_bench.py)

    def tiling(self, n_samples, n_frames):
        return clip_tiling(n_samples, n_frames, self.num_frames, self.num_seq, self.hops_per_frame, self.stft.hop, self.fps, self.sr)

    def output_length(self, n_clips):
        return self.stft.hop * (n_clips * self.num_seq * self.hops_per_frame - 1)

    def _mark(self, stage):
        if self._marks is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self._marks.append((stage, e))

    def _check(self, audio, frames, attn, audio_sr=None):
        """Every refusal, on shapes and flags only: nothing here touches the device.  -> (n_clips, starts, raw): raw = the [1, C, L0]
        view the audio_transform takes when audio_sr is given, else None."""
        if self.model.training:
            raise ValueError("the model is in training mode: call model.eval() first (train_av_net.py:147); an inference pass must "
                             "not update the BatchNorm running statistics")
        if (frames is None) == (attn is None):
            raise ValueError("pass exactly one of frames= (ViT input frames) and attn= (per-frame attention maps)")
        if frames is not None and self.video_attention is None:
            raise ValueError("frames= needs the Enhancer to be built with video_attention=")
        raw = None
        if audio_sr is not None:
            if self.audio_transform is None:
                raise ValueError("audio_sr= needs the Enhancer to be built with audio_transform=")
            if not isinstance(audio, torch.Tensor) or audio.dim() not in (1, 2):
                raise ValueError(f"audio must be [L0] or [C, L0] with audio_sr=, got {tuple(getattr(audio, 'shape', ()))}")
            raw, n_samples = self.audio_transform.check(audio, audio_sr)
        elif not isinstance(audio, torch.Tensor) or audio.dim() != 1 or audio.dtype != torch.float32:
            raise ValueError(f"audio must be a 1-D float32 tensor, got {getattr(audio, 'shape', type(audio))}")
        else:
            n_samples = audio.shape[0]
        vid = frames if frames is not None else attn
        ch = 3 if frames is not None else 1
        w = self.model.width
        if not isinstance(vid, torch.Tensor) or vid.dim() != 4 or tuple(vid.shape[1:]) != (ch, w, w) or vid.dtype != torch.float32:
            raise ValueError(f"{'frames' if frames is not None else 'attn'} must be float32 [N, {ch}, {w}, {w}] for this model, got "
                             f"{tuple(getattr(vid, 'shape', ()))} {getattr(vid, 'dtype', '')}")
        n_clips, starts = self.tiling(n_samples, vid.shape[0])
        if n_clips == 0:
            raise ValueError(f"the recording ({n_samples} samples at {self.sr} Hz, {vid.shape[0]} frames) is shorter than one clip of "
                             f"{self.clip_samples} samples and {self.clip_frames} frames")
        return n_clips, starts, raw

    def _prepare(self, audio, frames, attn, audio_sr=None):
        """Steps 2-3 for the whole recording: per-frame maps, clip scales, all clip STFTs.  -> dict of device buffers."""
        n_clips, starts, raw = self._check(audio, frames, attn, audio_sr)
        _lib.require_cuda(audio, frames, attn)
        if raw is not None:
            audio = self.audio_transform(raw, audio_sr)[0]          # the recording once: av_dataset.py:203-215, then the tiling at self.sr
        s, a, tc, stft = self.num_seq, self.hops_per_frame, self.clip_frames, self.stft
        dev, st, side = audio.device, stream_ptr(), self.model.width
        used = starts[-1] + tc                          # recording frames the clips use
        self._mark("start")
        # per-frame maps: the ViT once per frame, pass 1 of the map post-process
        flag = fmax = None
        if frames is not None:
            va = self.video_attention
            hp = wp = side // 8
            maps = torch.empty(used, hp * wp, device=dev, dtype=torch.float32)
            fmax = torch.empty(used, device=dev, dtype=torch.float32)
            flag = torch.zeros(1, device=dev, dtype=torch.int32)
            for f0 in range(0, used, va.frames_per_launch):
                f1 = min(used, f0 + va.frames_per_launch)
                att = va.cls_attention(frames[f0:f1])
                call("maavss_vit_attn_maps_pass1", ptr(att), ptr(maps[f0:f1]), ptr(fmax[f0:f1]), f1 - f0, va.spec.heads, hp * wp,
                     ptr(flag), st)
            frame_elems, upsample = hp * wp, 1
        else:
            maps = attn[:used].contiguous()
            if maps.data_ptr() % 16:
                maps = maps.clone()
            frame_elems, upsample = side * side, 0
        table = torch.tensor(starts, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        rcp = torch.empty(n_clips, device=dev, dtype=torch.float32)
        call("maavss_av_clip_scale", ptr(maps), ptr(fmax), ptr(table), n_clips, used, tc, frame_elems, int(self.attn_diff), ptr(rcp), st)
        if flag is not None and int(flag.item()) != 0:          # checked before any map reaches the model
            raise _lib.MaavssError(
                "Enhancer: non-finite attention maps -- an activation of the ViT left the range of its 16-bit storage format "
                f"(act_dtype={self.video_attention.act_dtype!r}) or the input frames / weights hold inf or NaN")
        self._mark("vit")
        # all clip STFTs in one launch, over overlapping rows of the recording
        audio = audio.contiguous()
        rows = audio.as_strided((n_clips, self.clip_samples), (s * a * stft.hop, 1))
        _, y, amax = stft(rows, want_x=False, return_scale=True)
        self._mark("stft")
        return dict(n_clips=n_clips, used=used, maps=maps, upsample=upsample, table=table, rcp=rcp, y=y, amax=amax)

    def _gather(self, p, w0, k, x_a, x_v):
        """Step 4's inputs of windows w0 .. w0 + k - 1 into x_a [>= k, 2, a*n, F] and x_v [>= k, 1, n, S, S]."""
        n, s, a, tc, side, st = self.num_frames, self.num_seq, self.hops_per_frame, self.clip_frames, self.model.width, stream_ptr()
        call("maavss_av_attn_windows", ptr(p["maps"]), ptr(p["rcp"]), ptr(p["table"]), p["n_clips"], p["used"], tc, s, n, w0, k, side,
             side, p["upsample"], int(self.attn_diff), ptr(x_v), st)
        call("maavss_av_stft_windows", ptr(p["y"]), p["n_clips"], a * tc, self.stft.n_bins(), a, s, n, w0, k, ptr(x_a), st)

    def window_inputs(self, audio, frames=None, attn=None, audio_sr=None):
        """All windows' model inputs at once (inspection; a whole recording's windows take n * S^2 * 4 B each):
        -> (x_a [C*s, 2, a*n, F], x_v [C*s, 1, n, S, S], amax [C]), window c*s + j = window j of clip c."""
        p = self._prepare(audio, frames, attn, audio_sr)
        w = p["n_clips"] * self.num_seq
        x_a = torch.empty(w, 2, self.hops_per_frame * self.num_frames, self.stft.n_bins(), device=audio.device, dtype=torch.float32)
        x_v = torch.empty(w, 1, self.num_frames, self.model.width, self.model.width, device=audio.device, dtype=torch.float32)
        self._gather(p, 0, w, x_a, x_v)
        return x_a, x_v, p["amax"]

    def enhance_stft(self, audio, frames=None, attn=None, audio_sr=None):
        """Steps 1-4: -> (stitched [1, 2, a*C*s, F], start)."""
        p = self._prepare(audio, frames, attn, audio_sr)
        n_win, nb, dev = p["n_clips"] * self.num_seq, self.stft.n_bins(), audio.device
        a, n, side, wpl = self.hops_per_frame, self.num_frames, self.model.width, min(self.windows_per_launch, n_win)
        # window buffers once per call, reused by every chunk: memory is bounded by one chunk
        x_v = torch.empty(wpl, 1, n, side, side, device=dev, dtype=torch.float32)
        x_a = torch.empty(wpl, 2, a * n, nb, device=dev, dtype=torch.float32)
        stitched = torch.empty(1, 2, a * n_win, nb, device=dev, dtype=torch.float32)
        gain = p["amax"] if self.stft.normalize_output_fft else None
        with torch.no_grad():
            for w0 in range(0, n_win, wpl):
                k = min(wpl, n_win - w0)
                self._gather(p, w0, k, x_a, x_v)
                self._mark("gather")
                pred = self.model(x_a[:k], x_v[:k])[0]
                self._mark("forward")
                stitch_windows(pred, gain, p["n_clips"], self.num_seq, w0, stitched)
                self._mark("stitch")
        return stitched, self.target_offset * a * self.stft.hop

    def __call__(self, audio, frames=None, attn=None, audio_sr=None):
        """audio [L] f32 cuda (with audio_sr=, on an Enhancer built with audio_transform=: the raw recording [L0] or [C, L0], f32 or int16,
        at audio_sr Hz, transformed once to self.sr before the tiling); frames [N,3,S,S] f32 cuda (the ViT input, needs video_attention) or attn [N,1,S,S] (per-frame maps,
        each divided by its own max as VideoAttention._inference / the attention-frame cache give them) -> (wave, start)."""
        stitched, start = self.enhance_stft(audio, frames, attn, audio_sr)
        wave = self.stft.inverse(stitched)[0]
        self._mark("inverse")
        return wave, start


def stitch_windows(pred, clip_absmax, n_clips, num_seq, w0=0, out=None):
    """Step 4's output half: pred [k, 2, a, F] of windows w0 .. w0 + k - 1 -> rows a*w .. a*w + a - 1 of out [1, 2, a*n_clips*num_seq, F],
    times g_c = clip_absmax[c] + 1e-7 (clip_absmax None: g_c = 1), c = w // num_seq."""
    _lib.require_cuda(pred, clip_absmax, out)
    k, two, a, nb = pred.shape
    if out is None:
        out = torch.empty(1, 2, a * n_clips * num_seq, nb, device=pred.device, dtype=torch.float32)
    assert two == 2 and pred.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (1, 2, a * n_clips * num_seq, nb)
    call("maavss_av_stitch", ptr(pred.contiguous()), ptr(clip_absmax), n_clips, num_seq, a, nb, w0, k, ptr(out), stream_ptr())
    return out
