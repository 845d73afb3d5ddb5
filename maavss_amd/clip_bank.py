"""A dataset's attention maps and audio resident in HBM, indexed in clips as the reference's dataset is.

The reference trains from cached attention frames (train_avse_frames.py:50, `attn_frames_path`; av_dataset.py:251-268) and cuts the
audio out of one memmap of the whole dataset (av_dataset.py:136-147, 285-294, `use_audio_memmap`): the frozen ViT runs once per
frame, not once per epoch.  `ClipBank` is that cache on the device.  Per frame it keeps the map at patch resolution, (S/8)^2 values
as maavss_vit_attn_maps_pass1 writes them (the frame divided by its own maximum), as f32 or as 16-bit integers; per recording the
samples at `sr`.  `batch(indices)` cuts a training batch from both without the ViT, the host or a synchronisation
(maavss_bank_attn_clips, maavss_bank_audio_clips; csrc/clip_bank.hip).

Clip index (utilities.extract_clips -> VideoClips, av_dataset.py:285-289): clip k of a recording takes its frames
[k*frame_hop, k*frame_hop + clip_frames) and its samples [s_k, s_k + hops_per_frame*hop*clip_frames) with
s_k = round(k*frame_hop*sr/fps) (Python's round on the exact fraction, as enhance.clip_tiling rounds).  A recording holds the longest
prefix of clips for which both its frames and its samples suffice, and the bank keeps the frames and samples those clips use.
Clips are numbered through the recordings in the order these were added.

Contract.  storage="f32": attn[b] is bit-identical to video_attention.attention_frames(frames[v:v+T], clip_frames=T,
attn_diff=attn_diff) of the clip's frames, audio[b] to the clip's samples.  storage="u16": a map value v is kept as
q = rint(min(max(v, 0), 1) * 65535) (one f32 product, half to even) and read back as the correctly rounded f32 quotient q / 65535;
the batch is the f32 contract applied to those values (clip maximum over them, or over their zero-padded difference, then
value * (1 / m)).  Against f32 storage the maps differ by at most 1/131070 (half a step; plus 2^-23 for the f32 roundings of the product
and the quotient) before the clip normalisation, in half the bytes.
A clip never reads a map or a sample of a neighbouring recording, with attn_diff too (clip frame 0 is 0 * (1 / m)).
tests/bank_twin.py restates the pack and the index on the host.

`batch(indices, boxes=, flip=)` crops and mirrors the stored maps per clip on the way out (maavss_bank_warp_maps, csrc/bank_warp.hip;
tests/bank_warp_twin.py restates it): the bank path's stand-in for the frames-fed path's RandomResizedCrop, drawn by `BankCrop`.

`activity()` is one pass over the bank that says which clips are silent, still or cut (csrc/clip_select.hip; tests/select_twin.py);
maavss_amd.ClipSampler turns it into the clips an epoch trains on.
"""
from bisect import bisect_right
from fractions import Fraction
from itertools import accumulate

import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .video_transform import VideoTransform

FORMAT = "maavss_amd.ClipBank"
FORMAT_VERSION = 1
_STORAGE = {"f32": (0, torch.float32), "u16": (1, torch.int16)}      # the u16 payload lives in int16 tensors (bit patterns)


def clip_sample_start(k, frame_hop, fps=30, sr=16000):
    """s_k: the first sample of a recording's clip k."""
    return round(k * frame_hop * Fraction(sr) / Fraction(fps))


def count_clips(n_frames, n_samples, clip_frames, frame_hop, clip_samples, fps=30, sr=16000):
    """The longest prefix of clips that n_frames frames and n_samples samples hold."""
    k = 0
    while k * frame_hop + clip_frames <= n_frames and clip_sample_start(k, frame_hop, fps, sr) + clip_samples <= n_samples:
        k += 1
    return k


def _positive_int(name, v):
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"{name} must be a positive integer, got {v!r}")
    return v


class ClipBank:
    """`bank = ClipBank(frame_size, clip_frames, frame_hop, hops_per_frame, hop, capacity_frames=.., capacity_samples=..)`;
    `bank.add_recording(audio, frames=.., video_attention=va)` once per recording; `attn, audio = bank.batch(indices)` per step.

    frame_size S: frames are S x S, S % 4 == 0, S >= 8, patch grid S // 8 squared.  The map buffer [capacity_frames][(S//8)^2] and the
    audio buffer [capacity_samples] are allocated here, once: nothing is reallocated or copied later, and a recording that does not fit
    raises ValueError and leaves the bank as it was.  See the module docstring for the clip index and the contract."""

    def __init__(self, frame_size, clip_frames, frame_hop, hops_per_frame, hop, *, fps=30, sr=16000, capacity_frames, capacity_samples,
                 storage="f32", device="cuda"):
        s = _positive_int("frame_size", frame_size)
        if s < 8 or s % 4:
            raise ValueError(f"frame_size must be at least 8 and a multiple of 4, got {s}")
        for name, v in (("clip_frames", clip_frames), ("frame_hop", frame_hop), ("hops_per_frame", hops_per_frame), ("hop", hop),
                        ("capacity_frames", capacity_frames), ("capacity_samples", capacity_samples)):
            _positive_int(name, v)
        if not (fps > 0 and sr > 0):
            raise ValueError("fps and sr must be positive")
        if storage not in _STORAGE:
            raise ValueError(f"storage must be 'f32' or 'u16', got {storage!r}")
        self.frame_size, self.clip_frames, self.frame_hop, self.hops_per_frame, self.hop = s, clip_frames, frame_hop, hops_per_frame, hop
        self.fps, self.sr, self.storage = fps, sr, storage
        self.capacity_frames, self.capacity_samples = capacity_frames, capacity_samples
        self.clip_samples = hops_per_frame * hop * clip_frames
        self.frame_elems = (s // 8) ** 2
        self.device = torch.device(device)
        self.maps = torch.empty(capacity_frames, self.frame_elems, device=self.device, dtype=_STORAGE[storage][1])
        self.audio = torch.empty(capacity_samples, device=self.device, dtype=torch.float32)
        self.n_frames = self.n_samples = 0            # used part of the two buffers
        self.recordings = []                          # per recording (first frame, first sample, frames, samples, clips)
        self._clip_ends = []                          # running total of clips after each recording
        self._tables = None                           # the same as CPU tensors, for batch()
        self._activity = None                         # (range_db, activity()'s result), until the next add_recording

    # ---- the clip index: pure host arithmetic ---------------------------------------------------------
    def __len__(self):
        return self._clip_ends[-1] if self._clip_ends else 0

    def locate(self, idx):
        """Clip number -> (recording, k): clip k of the recording-th recording added."""
        if isinstance(idx, bool) or not isinstance(idx, int) or not 0 <= idx < len(self):
            raise IndexError(f"clip index {idx!r} is outside [0, {len(self)})")
        r = bisect_right(self._clip_ends, idx)
        return r, idx - (self._clip_ends[r - 1] if r else 0)

    def clip_start(self, idx):
        """Clip number -> (frame, sample): where the clip starts in the bank's two buffers."""
        r, k = self.locate(idx)
        f0, s0 = self.recordings[r][:2]
        return f0 + k * self.frame_hop, s0 + clip_sample_start(k, self.frame_hop, self.fps, self.sr)

    def count_clips(self, n_frames, n_samples):
        return count_clips(n_frames, n_samples, self.clip_frames, self.frame_hop, self.clip_samples, self.fps, self.sr)

    def _append(self, n_frames, n_samples, n_clips):
        self.recordings.append((self.n_frames, self.n_samples, n_frames, n_samples, n_clips))
        self._clip_ends.append(len(self) + n_clips)
        self.n_frames += n_frames
        self.n_samples += n_samples
        self._tables = self._activity = None

    def _check_recording(self, audio, frames, maps, video_attention):
        """Every refusal of add_recording, on shapes and the bank's fill alone -> (clips, frames used, samples used)."""
        if (frames is None) == (maps is None):
            raise ValueError("pass exactly one of frames= (ViT input frames) and maps= (per-frame maps at patch resolution)")
        if not isinstance(audio, torch.Tensor) or audio.dim() != 1 or audio.dtype != torch.float32:
            raise ValueError(f"audio must be a 1-D float32 tensor, got {getattr(audio, 'dtype', type(audio))} {tuple(getattr(audio, 'shape', ()))}")
        s = self.frame_size
        if frames is not None:
            if video_attention is None:
                raise ValueError("frames= needs video_attention=, the extractor that turns them into maps")
            if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or tuple(frames.shape[1:]) != (3, s, s) or frames.dtype != torch.float32:
                raise ValueError(f"frames must be float32 [N, 3, {s}, {s}], got {getattr(frames, 'dtype', type(frames))} "
                                 f"{tuple(getattr(frames, 'shape', ()))}")
            n = frames.shape[0]
        else:
            if video_attention is not None:
                raise ValueError("video_attention= goes with frames=; maps= are stored as given")
            if not isinstance(maps, torch.Tensor) or maps.dim() != 2 or maps.shape[1] != self.frame_elems or maps.dtype != torch.float32:
                raise ValueError(f"maps must be float32 [N, {self.frame_elems}] (the {s // 8} x {s // 8} patch grid of {s} x {s} frames), got "
                                 f"{getattr(maps, 'dtype', type(maps))} {tuple(getattr(maps, 'shape', ()))}")
            n = maps.shape[0]
        n_clips = self.count_clips(n, audio.shape[0])
        if n_clips == 0:
            raise ValueError(f"the recording ({n} frames, {audio.shape[0]} samples) holds no whole clip of {self.clip_frames} frames and "
                             f"{self.clip_samples} samples")
        used_f = (n_clips - 1) * self.frame_hop + self.clip_frames
        used_s = clip_sample_start(n_clips - 1, self.frame_hop, self.fps, self.sr) + self.clip_samples
        if self.n_frames + used_f > self.capacity_frames:
            raise ValueError(f"capacity_frames={self.capacity_frames} exceeded: {self.n_frames} frames banked, the recording's clips use {used_f}")
        if self.n_samples + used_s > self.capacity_samples:
            raise ValueError(f"capacity_samples={self.capacity_samples} exceeded: {self.n_samples} samples banked, the recording's clips use {used_s}")
        return n_clips, used_f, used_s

    def add_recording(self, audio, *, frames=None, maps=None, video_attention=None):
        """Bank one recording -> the number of clips it adds.  audio [L] f32, mono at `sr`, on the bank's device (a raw recording goes
        through AudioTransform first).  Exactly one of
          frames [N,3,S,S] f32, the ViT input after the frame transform, with video_attention=: the frames go through cls_attention and
            maavss_vit_attn_maps_pass1, frames_per_launch at a time, straight into the map buffer.  The extractor's non-finite flag is
            read once at the end (this call may synchronise); a non-finite map raises MaavssError and the recording is not added.
          maps [N,(S//8)^2] f32 as pass 1 writes them: for callers with maps of their own.  They are stored as given, unchecked.
        The crop is whatever the frames were given with: one crop per recording, fixed when it is banked, as in the reference's
        attention-frame cache; batch(boxes=, flip=) crops and mirrors the stored maps per clip and step instead (the map, not the frame:
        see there).  Frames and samples behind the recording's last whole clip are not kept."""
        n_clips, used_f, used_s = self._check_recording(audio, frames, maps, video_attention)
        u16 = self.storage == "u16"
        if u16 or frames is not None:
            _lib.require_cuda(audio, frames, maps, self.maps)
        dst, st = self.maps[self.n_frames:self.n_frames + used_f], None
        if frames is not None:
            va, st = video_attention, stream_ptr()
            flag = torch.zeros(1, device=self.device, dtype=torch.int32)
            step = va.frames_per_launch
            fmax = torch.empty(min(step, used_f), device=self.device, dtype=torch.float32)
            tmp = torch.empty(min(step, used_f), self.frame_elems, device=self.device, dtype=torch.float32) if u16 else None
            for f0 in range(0, used_f, step):
                f1 = min(used_f, f0 + step)
                att = va.cls_attention(frames[f0:f1])
                small = tmp[:f1 - f0] if u16 else dst[f0:f1]
                call("maavss_vit_attn_maps_pass1", ptr(att), ptr(small), ptr(fmax), f1 - f0, va.spec.heads, self.frame_elems, ptr(flag), st)
                if u16:
                    call("maavss_bank_pack_u16", ptr(small), ptr(dst[f0:f1]), small.numel(), st)
            if int(flag.item()) != 0:
                raise _lib.MaavssError(
                    "ClipBank: non-finite attention maps -- an activation of the ViT left the range of its 16-bit storage format "
                    f"(act_dtype={va.act_dtype!r}) or the input frames / weights hold inf or NaN; the recording was not added")
        elif u16:
            src = maps[:used_f].contiguous()
            call("maavss_bank_pack_u16", ptr(src), ptr(dst), src.numel(), stream_ptr())
        else:
            dst.copy_(maps[:used_f])
        self.audio[self.n_samples:self.n_samples + used_s].copy_(audio[:used_s])
        self._append(used_f, used_s, n_clips)
        return n_clips

    def unpacked_maps(self, recording=None):
        """The banked maps as f32 [frames, (S//8)^2] (a copy), of one recording or of all: what batch() normalises and upsamples."""
        f0, n = (0, self.n_frames) if recording is None else (self.recordings[recording][0], self.recordings[recording][2])
        part = self.maps[f0:f0 + n]
        if self.storage == "f32" or n == 0:
            return part.clone()
        _lib.require_cuda(part)
        out = torch.empty(n, self.frame_elems, device=self.device, dtype=torch.float32)
        call("maavss_bank_unpack_u16", ptr(part), ptr(out), out.numel(), stream_ptr())
        return out

    # ---- batches ----------------------------------------------------------------------------------------
    def check_indices(self, indices):
        """Host-side validation of batch()'s indices (no device work) -> (frame starts int32 [B], sample starts int64 [B]), CPU tensors
        in bank coordinates."""
        if isinstance(indices, torch.Tensor):
            if indices.is_cuda:
                raise ValueError("indices must be a CPU sequence or tensor (they are checked on the host, like crop boxes)")
            if indices.dim() != 1 or indices.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8):
                raise ValueError(f"indices must be a 1-D integer tensor, got {indices.dtype} {tuple(indices.shape)}")
            idx = indices.to(torch.int64)
        else:
            idx = list(indices)
            if any(isinstance(i, bool) or not isinstance(i, int) for i in idx):
                raise ValueError("indices must be integers")
            idx = torch.tensor(idx, dtype=torch.int64)
        if idx.numel() == 0:
            raise ValueError("indices is empty")
        if bool(((idx < 0) | (idx >= len(self))).any()):
            raise IndexError(f"clip indices must be in [0, {len(self)}), got [{int(idx.min())}, {int(idx.max())}]")
        if self._tables is None:
            rec = torch.tensor(self.recordings, dtype=torch.int64)
            ends = torch.tensor(self._clip_ends, dtype=torch.int64)
            s_k = torch.tensor([clip_sample_start(k, self.frame_hop, self.fps, self.sr) for k in range(int(rec[:, 4].max()))], dtype=torch.int64)
            self._tables = (ends, ends - rec[:, 4], rec[:, 0], rec[:, 1], s_k)
        ends, firsts, frame0, sample0, s_k = self._tables
        r = torch.bucketize(idx, ends, right=True)
        k = idx - firsts[r]
        return (frame0[r] + k * self.frame_hop).to(torch.int32), sample0[r] + s_k[k]

    def check_warp(self, b, boxes, flip, frame_norm=True):
        """Host-side validation of batch()'s crop arguments (no device work) -> None without boxes and flip, else (boxes CPU int32
        [b, 4], flip CPU uint8 [b]): a missing box is the whole frame, a missing flip none."""
        if boxes is None and flip is None:
            if frame_norm is not True:
                raise ValueError("frame_norm= belongs to the warped path: it needs boxes= or flip=")
            return None
        s = self.frame_size
        if s % 8:
            raise ValueError(f"boxes= / flip= resample the {s // 8} x {s // 8} patch grid and need frame_size % 8 == 0, got {s}")
        if boxes is None:
            boxes = torch.tensor([0, 0, s, s], dtype=torch.int32).repeat(b, 1)
        else:
            if not isinstance(boxes, torch.Tensor) or boxes.device.type != "cpu" or boxes.dtype != torch.int32 or tuple(boxes.shape) != (b, 4):
                raise ValueError(f"boxes must be a CPU int32 tensor [{b}, 4] of (top, left, height, width), one per clip, got "
                                 f"{getattr(boxes, 'dtype', type(boxes))} {tuple(getattr(boxes, 'shape', ()))}"
                                 f"{' on ' + str(boxes.device) if isinstance(boxes, torch.Tensor) and boxes.device.type != 'cpu' else ''}")
            top, left, h, w = boxes.to(torch.int64).unbind(1)
            bad = (h < 1) | (w < 1) | (top < 0) | (left < 0) | (top + h > s) | (left + w > s)
            if bool(bad.any()):
                k = int(bad.nonzero()[0, 0])
                raise ValueError(f"box {k} = {tuple(boxes[k].tolist())} (top, left, height, width) is empty or not inside the {s}x{s} frame")
            boxes = boxes.contiguous()
        if flip is None:
            flip = torch.zeros(b, dtype=torch.uint8)
        else:
            if (not isinstance(flip, torch.Tensor) or flip.device.type != "cpu" or flip.dtype not in (torch.bool, torch.uint8)
                    or tuple(flip.shape) != (b,)):
                raise ValueError(f"flip must be a CPU bool or uint8 tensor [{b}], one flag per clip, got "
                                 f"{getattr(flip, 'dtype', type(flip))} {tuple(getattr(flip, 'shape', ()))}")
            flip = flip.ne(0).to(torch.uint8)
        return boxes, flip

    def batch(self, indices, *, attn_diff=False, out=None, boxes=None, flip=None, frame_norm=True):
        """The clips `indices` (a CPU sequence or integer tensor; duplicates allowed; anything outside [0, len) raises before any device
        work) -> (attn [B,1,clip_frames,S,S] f32, audio [B, clip_samples] f32) on the current stream.  out=(attn, audio): buffers of
        those shapes to fill (attn contiguous; audio with unit last stride, its rows may be longer than a clip).  The start tables
        reach the device in one copy from pinned memory: no synchronisation.

        boxes= (CPU int32 [B, 4] of (top, left, height, width) in pixels of the S x S frame, as VideoTransform.sample_boxes and
        BankCrop.sample give them) and / or flip= (CPU bool or uint8 [B]): every clip's stored maps are resampled from its box to the
        whole patch grid and mirrored where flagged (maavss_bank_warp_maps; the definition is in include/maavss.h), each frame divided
        by its own maximum again (frame_norm=True, as the extractor leaves it) or not, and the clip maximum, attn_diff and the x8
        upsampling follow on the warped maps as they do on the stored ones.  Needs S % 8 == 0.  This crops the attention MAP: it is a
        geometric augmentation of the tensor the fusion network reads, not the attention of the cropped frame (the ViT would attend
        differently).  A frame whose box holds only zeros becomes NaN under frame_norm, as an all-zero map does in the extractor.
        Every refusal is raised before any device work; boxes and flags travel in the same pinned copy as the start tables.  Without
        boxes= and flip= the launches, buffers and bytes are those of the plain cut."""
        starts = self.check_indices(indices)
        return self.cut(*starts, attn_diff=attn_diff, out=out, boxes=boxes, flip=flip, frame_norm=frame_norm)

    def _stage(self, frame_start, sample_start, warp):
        """Every table of one batch in one non-blocking copy through pinned memory -> device int32: the int64 sample starts (8-byte
        aligned) [0, 2b), the frame starts [2b, 3b) and, with a warp, the warped workspace's clip starts b * clip_frames [3b, 4b),
        the boxes [4b, 8b) and the flip bytes [8b, ...)."""
        b = frame_start.numel()
        parts = [sample_start.view(torch.int32), frame_start]
        if warp is not None:
            flips = torch.zeros((b + 3) // 4 * 4, dtype=torch.uint8)
            flips[:b] = warp[1]
            parts += [torch.arange(b, dtype=torch.int32) * self.clip_frames, warp[0].reshape(-1), flips.view(torch.int32)]
        host = torch.cat(parts)
        staged = torch.empty(host.numel(), device=self.device, dtype=torch.int32)
        staged.copy_(host.pin_memory(), non_blocking=True)
        return staged

    def _warp(self, staged, b, frame_norm):
        """maavss_bank_warp_maps on the staged tables -> the workspace [b * clip_frames, frame_elems] f32."""
        ws = torch.empty(b * self.clip_frames, self.frame_elems, device=self.device, dtype=torch.float32)
        call("maavss_bank_warp_maps", ptr(self.maps), _STORAGE[self.storage][0], ptr(staged[2 * b:]), ptr(staged[4 * b:]), ptr(staged[8 * b:]),
             b, self.n_frames, self.clip_frames, self.frame_size, int(bool(frame_norm)), ptr(ws), stream_ptr())
        return ws

    def warp_maps(self, indices, boxes, flip=None, frame_norm=True):
        """The cropped / flipped maps batch(indices, boxes=, flip=, frame_norm=) upsamples, at patch resolution -> f32
        [B, clip_frames, S // 8, S // 8] on the current stream; one launch, no synchronisation."""
        frame_start, sample_start = self.check_indices(indices)
        b = frame_start.numel()
        if boxes is None:
            raise ValueError("warp_maps needs boxes=")
        warp = self.check_warp(b, boxes, flip, frame_norm)
        _lib.require_cuda(self.maps)
        ws = self._warp(self._stage(frame_start, sample_start, warp), b, frame_norm)
        return ws.view(b, self.clip_frames, self.frame_size // 8, self.frame_size // 8)

    def cut(self, frame_start, sample_start, *, attn_diff=False, out=None, boxes=None, flip=None, frame_norm=True):
        """batch() behind its index check: the two CPU tables check_indices returned -> (attn, audio)."""
        b, t, s, n =frame_start.numel(), self.clip_frames, self.frame_size, self.clip_samples
        warp = self.check_warp(b, boxes, flip, frame_norm)
        if out is None:
            _lib.require_cuda(self.maps)
            attn = torch.empty(b, 1, t, s, s, device=self.device, dtype=torch.float32)
            audio = torch.empty(b, n, device=self.device, dtype=torch.float32)
        else:
            attn, audio = out
            if (not isinstance(attn, torch.Tensor) or tuple(attn.shape) != (b, 1, t, s, s) or attn.dtype != torch.float32
                    or not attn.is_contiguous()):
                raise ValueError(f"out[0] must be a contiguous float32 {[b, 1, t, s, s]} tensor, got {getattr(attn, 'dtype', type(attn))} "
                                 f"{tuple(getattr(attn, 'shape', ()))}")
            if (not isinstance(audio, torch.Tensor) or tuple(audio.shape) != (b, n) or audio.dtype != torch.float32 or audio.stride(1) != 1
                    or (b > 1 and audio.stride(0) < n)):
                raise ValueError(f"out[1] must be a float32 {[b, n]} tensor with unit last stride and rows that do not overlap, got "
                                 f"{getattr(audio, 'dtype', type(audio))} {tuple(getattr(audio, 'shape', ()))}")
            _lib.require_cuda(self.maps, attn, audio)
        # every table in one copy through pinned memory, as Mixer stages its partners: a blocking copy on ClipPipeline's side stream would
        # hold the host until the work queued in front of it had finished
        staged = self._stage(frame_start, sample_start, warp)
        rcp = torch.empty(b, device=self.device, dtype=torch.float32)
        st = stream_ptr()
        if warp is None:
            call("maavss_bank_attn_clips", ptr(self.maps), _STORAGE[self.storage][0], ptr(staged[2 * b:]), b, self.n_frames, t, s, s,
                 int(bool(attn_diff)), ptr(rcp), ptr(attn), st)
        else:
            # the warped maps are an f32 bank of b clips laid end to end: the clip maximum and the x8 stores are the plain cut's
            ws = self._warp(staged, b, frame_norm)
            call("maavss_bank_attn_clips", ptr(ws), 0, ptr(staged[3 * b:]), b, b * t, t, s, s, int(bool(attn_diff)), ptr(rcp), ptr(attn), st)
        call("maavss_bank_audio_clips", ptr(self.audio), self.n_samples, ptr(staged), b, n, ptr(audio), audio.stride(0) if b > 1 else n, st)
        return attn, audio

    # ---- which clips are worth a step ---------------------------------------------------------------------
    def clip_recordings(self):
        """The recording every clip belongs to: CPU int32 [len(bank)], pure host arithmetic."""
        ends = torch.tensor(self._clip_ends, dtype=torch.int64)
        return torch.bucketize(torch.arange(len(self), dtype=torch.int64), ends, right=True).to(torch.int32)

    def activity(self, range_db=40.0):
        """Per-clip activity statistics of every banked clip, computed on the device next to the data (csrc/clip_select.hip; the
        definitions and the order of every sum are in include/maavss.h, restated by tests/select_twin.py) -> a dict of device tensors
        of length len(bank):
          f64  energy (sum of squares), rms_db = 10 log10(energy / clip_samples) (-inf for silence), rel_db (the same against the mean
               power of the clip's recording), motion_mean and motion_peak (mean / largest mean absolute difference of consecutive
               stored maps inside the clip; 0 for clips of one frame)
          f32  peak (max |x|)
          i32  n_bad (inf or NaN samples), n_active (segments of `hop` samples whose mean power is at least the recording's mean power
               less range_db decibels -- the dynamic-range rule STOI uses for silent frames), recording
        The clip tables are uploaded once from pinned memory and four launches follow on the current stream: no synchronisation.  The
        result is cached until the next add_recording (save / load do not store it: the pass is cheaper than a format change).
        `ClipSampler` turns the table into the clips to train on."""
        if not isinstance(range_db, (int, float)) or isinstance(range_db, bool) or not 0.0 <= range_db <= 3000.0:
            raise ValueError(f"range_db must be a number in [0, 3000], got {range_db!r}")
        range_db = float(range_db)
        if self._activity is not None and self._activity[0] == range_db:
            return self._activity[1]
        c, r = len(self), len(self.recordings)
        if c == 0:
            raise ValueError("the bank holds no clip")
        j = self.hops_per_frame * self.clip_frames
        if j > _lib.query("maavss_bank_max_segments"):
            raise ValueError(f"hops_per_frame * clip_frames = {j} segments per clip, the activity kernel holds {_lib.query('maavss_bank_max_segments')}")
        _lib.require_cuda(self.maps, self.audio)
        frame_start, sample_start = self.check_indices(torch.arange(c, dtype=torch.int64))
        rec = self.clip_recordings()
        chunks = [_lib.query("maavss_bank_level_chunks", q[3]) for q in self.recordings]
        first = [0] + list(accumulate(chunks))[:-1]          # a recording's first chunk partial: the running chunk count
        rec_tab = torch.tensor([[q[1] for q in self.recordings], [q[3] for q in self.recordings], first], dtype=torch.int64)
        # one copy through pinned memory, as cut() stages its tables: the int64 tables first (8-byte aligned), then the int32 ones
        host = torch.cat([sample_start.view(torch.int32), rec_tab.reshape(-1).view(torch.int32), frame_start, rec]).pin_memory()
        staged = torch.empty(host.numel(), device=self.device, dtype=torch.int32)
        staged.copy_(host, non_blocking=True)
        o_rec, o_frame, o_clip_rec = 2 * c, 2 * c + 6 * r, 3 * c + 6 * r
        f64 = {k: torch.empty(c, device=self.device, dtype=torch.float64) for k in ("energy", "rms_db", "rel_db", "motion_mean", "motion_peak")}
        peak = torch.empty(c, device=self.device, dtype=torch.float32)
        n_bad, n_active = (torch.empty(c, device=self.device, dtype=torch.int32) for _ in range(2))
        partials = torch.empty(sum(chunks), device=self.device, dtype=torch.float64)
        level = torch.empty(r, device=self.device, dtype=torch.float64)
        st = stream_ptr()
        call("maavss_bank_recording_level", ptr(self.audio), self.n_samples, ptr(staged[o_rec:]), ptr(host[o_rec:]), r, ptr(partials),
             partials.numel(), ptr(level), st)
        motion = None
        if self.clip_frames > 1:
            motion = torch.empty(self.n_frames - 1, device=self.device, dtype=torch.float64)
            call("maavss_bank_frame_motion", ptr(self.maps), _STORAGE[self.storage][0], self.n_frames, self.frame_elems, ptr(motion), st)
        call("maavss_bank_clip_activity", ptr(self.audio), self.n_samples, ptr(motion), self.n_frames, ptr(level), ptr(staged[o_rec:]), r,
             ptr(staged), ptr(staged[o_frame:]), ptr(staged[o_clip_rec:]), ptr(host), ptr(host[o_frame:]), ptr(host[o_clip_rec:]), c,
             self.clip_frames, self.hops_per_frame, self.hop, 10.0 ** (-range_db / 10.0), ptr(f64["energy"]), ptr(f64["rms_db"]),
             ptr(f64["rel_db"]), ptr(f64["motion_mean"]), ptr(f64["motion_peak"]), ptr(peak), ptr(n_bad), ptr(n_active), st)
        out = dict(f64, peak=peak, n_bad=n_bad, n_active=n_active, recording=staged[o_clip_rec:o_clip_rec + c])
        self._activity = (range_db, out)
        return out

    # ---- one file -----------------------------------------------------------------------------------------
    def save(self, path):
        """The used part of both buffers (CPU tensors), the per-recording lengths and every constructor argument, in one file."""
        torch.save({"format": FORMAT, "version": FORMAT_VERSION, "frame_size": self.frame_size, "clip_frames": self.clip_frames,
                    "frame_hop": self.frame_hop, "hops_per_frame": self.hops_per_frame, "hop": self.hop, "fps": self.fps, "sr": self.sr,
                    "storage": self.storage, "capacity_frames": self.capacity_frames, "capacity_samples": self.capacity_samples,
                    "recordings": torch.tensor([r[2:4] for r in self.recordings], dtype=torch.int64).reshape(-1, 2),
                    "maps": self.maps[:self.n_frames].cpu(), "audio": self.audio[:self.n_samples].cpu()}, path)

    @classmethod
    def load(cls, path, device="cuda", *, frame_size=None, storage=None, capacity_frames=None, capacity_samples=None):
        """A bank as save() wrote it (read with torch.load(weights_only=True)).  frame_size / storage: what the caller expects; a file
        that says otherwise is refused.  capacity_*: default the stored fill, may be given larger."""
        d = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(d, dict) or d.get("format") != FORMAT:
            raise ValueError(f"{path}: not a ClipBank file (format {d.get('format') if isinstance(d, dict) else type(d).__name__!r})")
        if d.get("version") != FORMAT_VERSION:
            raise ValueError(f"{path}: version {d.get('version')!r} of the ClipBank format, this build reads version {FORMAT_VERSION}")
        if frame_size is not None and frame_size != d["frame_size"]:
            raise ValueError(f"{path}: frame_size {d['frame_size']} in the file, frame_size={frame_size} expected")
        if storage is not None and storage != d["storage"]:
            raise ValueError(f"{path}: storage {d['storage']!r} in the file, storage={storage!r} expected")
        maps, audio = d["maps"], d["audio"]
        cap_f = maps.shape[0] if capacity_frames is None else capacity_frames
        cap_s = audio.shape[0] if capacity_samples is None else capacity_samples
        if cap_f < maps.shape[0] or cap_s < audio.shape[0]:
            raise ValueError(f"{path}: holds {maps.shape[0]} frames and {audio.shape[0]} samples, more than capacity_frames={cap_f} / "
                             f"capacity_samples={cap_s}")
        bank = cls(d["frame_size"], d["clip_frames"], d["frame_hop"], d["hops_per_frame"], d["hop"], fps=d["fps"], sr=d["sr"],
                   capacity_frames=max(cap_f, 1), capacity_samples=max(cap_s, 1), storage=d["storage"], device=device)
        if maps.dtype != bank.maps.dtype or maps.dim() != 2 or maps.shape[1] != bank.frame_elems or audio.dtype != torch.float32 or audio.dim() != 1:
            raise ValueError(f"{path}: buffers {maps.dtype} {tuple(maps.shape)} / {audio.dtype} {tuple(audio.shape)} do not fit "
                             f"storage {d['storage']!r} at frame_size {d['frame_size']}")
        for n_f, n_s in d["recordings"].tolist():
            n_clips = bank.count_clips(n_f, n_s)
            if n_clips == 0 or bank.n_frames + n_f > maps.shape[0] or bank.n_samples + n_s > audio.shape[0]:
                raise ValueError(f"{path}: the recording table does not fit the stored buffers")
            bank._append(n_f, n_s, n_clips)
        bank.maps[:bank.n_frames].copy_(maps[:bank.n_frames])
        bank.audio[:bank.n_samples].copy_(audio[:bank.n_samples])
        return bank


class BankCrop:
    """The random boxes and flips of ClipBank.batch(boxes=, flip=): `boxes, flip = BankCrop(scale, ratio, flip=p).sample(B, S, generator)`.

    Host code.  Draw order: first the B boxes, exactly VideoTransform(S, scale, ratio).sample_boxes(B, S, S, generator) -- the
    frames-fed path's RandomResizedCrop boxes on the S x S frame -- then, only when flip > 0, one torch.rand(B, dtype=float64,
    generator=generator) < flip.  With flip == 0 the generator is left where the boxes left it and no clip is flipped."""

    def __init__(self, scale=(0.6, 1.0), ratio=(3 / 4, 4 / 3), flip=0.0):
        if not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]):
            raise ValueError(f"bad scale {scale} or ratio {ratio}")
        if isinstance(flip, bool) or not isinstance(flip, (int, float)) or not 0.0 <= flip <= 1.0:
            raise ValueError(f"flip must be a probability in [0, 1], got {flip!r}")
        self.scale, self.ratio, self.flip = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1])), float(flip)

    def sample(self, batch, frame_size, generator=None):
        """-> (boxes CPU int32 [batch, 4] of (top, left, height, width), flip CPU bool [batch])."""
        _positive_int("batch", batch)
        s = _positive_int("frame_size", frame_size)
        boxes = VideoTransform(s, self.scale, self.ratio).sample_boxes(batch, s, s, generator)
        if self.flip > 0:
            flip = torch.rand(batch, dtype=torch.float64, generator=generator) < self.flip
        else:
            flip = torch.zeros(batch, dtype=torch.bool)
        return boxes, flip
