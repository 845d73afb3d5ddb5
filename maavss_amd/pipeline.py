"""Two-stream clip pipeline: attention-frame extraction + STFT of batch i+1 on a side HIP stream while the training step of
batch i runs on the main stream.

In the reference the ViT and the STFT run in the DATA path (`AV_Dataset.__getitem__`, av_dataset.py:321 and :335-342, called
by the DataLoader at train_avse_frames.py:122) and have no dependency on the optimizer step (:150-181) -- only the order
"extract batch i before training on batch i".  This module keeps exactly that dependency and nothing more: extraction of the
next batch is enqueued on its own stream and joins the training stream through HIP events, so the latency-bound parts of the
fusion network's step (16 sequential LSTM launches per direction, the M = batch Linear layers, the small STFT-encoder
convolutions) run next to the extractor's full-chip GEMMs instead of in front of them.  Slots are double-buffered; a slot
is reused only after the training step that read it has been enqueued and has signalled its `consumed` event.

With `transform` (a VideoTransform) the pipeline starts one stage earlier, at the decoder's uint8 clips: the frame transform of
av_dataset.py:315-319 runs on the side stream in front of the extractor, into a per-slot frame buffer.  With `audio_transform` (an
AudioTransform) and `audio_length` (the samples per clip the STFT is to see) the audio side does the same: the demuxer's PCM clips
at their own rate go through av_dataset.py:203-215 on the side stream in front of the STFT, into a per-slot clip buffer.
With `mixer` (a Mixer built on the same STFT) the bare STFT call becomes the mixer's: x is the clip mixed with other clips of the batch
(the interferers are the clips after the audio transform), y stays the clip's own STFT.
With `bank` (a ClipBank) the batches come from attention maps and audio already resident on the device: `submit_clips(indices, seed)`
cuts them on the side stream (no ViT, no frame or audio transform) in front of the same STFT / mixer call; `video_attention` may
then be None.  With `bank_crop` (a BankCrop) every clip of such a batch gets a random box and flip, and the bank cuts the batch through
them (ClipBank.batch(boxes=, flip=): the stored maps cropped and mirrored, no ViT).
With `reverb` (a Reverb holding a table of room responses) every clip is convolved with a room on the side stream in front of that
call: from zero state in submit(), from its recording's past in the bank in submit_clips().  reverb_target="wet": the wet clips take
the place of the audio, so y is reverberant too and every interferer of a mixture carries its own room; "dry": x is the STFT of the
wet clips (with its noise), y the STFT of the dry ones -- the network learns to dereverberate.  "dry" with a mixer is not built.
"""
import torch

from .reverb import bank_floor


class ClipPipeline:
    def __init__(self, video_attention, stft, clip_frames, depth=2, finite_check="deferred", *, transform=None, audio_transform=None,
                 audio_length=None, mixer=None, bank=None, reverb=None, reverb_target="wet", bank_crop=None):
        self.va, self.stft, self.t = video_attention, stft, clip_frames
        if bank is not None:
            if transform is not None or audio_transform is not None:
                raise ValueError("transform= / audio_transform= do not go with bank=: a bank holds maps and audio that are already transformed")
            if bank.clip_frames != clip_frames:
                raise ValueError(f"the bank cuts clips of {bank.clip_frames} frames, the pipeline was given clip_frames={clip_frames}")
        if bank_crop is not None:
            if bank is None:
                raise ValueError("bank_crop= draws the crops of a bank's batches: it needs bank=")
            if bank.frame_size % 8:
                raise ValueError(f"bank_crop= needs a bank with frame_size % 8 == 0, got {bank.frame_size}")
        self.bank, self.bank_crop = bank, bank_crop
        self.transform = transform
        if audio_transform is None and audio_length is not None:
            raise ValueError("audio_length needs a ClipPipeline built with audio_transform=")
        if audio_transform is not None and (isinstance(audio_length, bool) or not isinstance(audio_length, int) or audio_length < 1):
            raise ValueError(f"audio_transform= needs audio_length=, the samples per clip after the transform, got {audio_length!r}")
        self.audio_transform, self.audio_length = audio_transform, audio_length
        if mixer is not None and mixer.stft is not stft:
            raise ValueError("mixer= must be built on the STFT object the pipeline is given")
        self.mixer = mixer
        if reverb_target not in ("wet", "dry"):
            raise ValueError(f"reverb_target must be 'wet' or 'dry', got {reverb_target!r}")
        if reverb is not None and reverb_target == "dry" and mixer is not None:
            raise ValueError("reverb_target='dry' together with mixer= is not built: the target of a reverberant mixture is left open")
        self.reverb, self.reverb_target = reverb, reverb_target
        self.depth = depth
        self.finite_check = finite_check
        self.side = torch.cuda.Stream()
        self.slots = [dict(attn=None, x=None, y=None, ready=torch.cuda.Event(), consumed=None) for _ in range(depth)]
        if transform is not None:
            for slot in self.slots:
                slot["frames"] = None
        if audio_transform is not None:
            for slot in self.slots:
                slot["audio"] = None
        self.head = self.tail = 0            # next slot to submit into / next slot to hand out

    def check_audio(self, audio, audio_sr):
        """Host-side validation of submit()'s audio arguments (no device work) -> the raw clips as [B, C, L0], None without an
        audio_transform."""
        if self.audio_transform is None:
            if audio_sr is not None:
                raise ValueError("audio_sr needs a ClipPipeline built with audio_transform=")
            return None
        if audio_sr is None:
            raise ValueError("a ClipPipeline built with audio_transform= needs audio_sr=, the rate of the submitted clips")
        if not isinstance(audio, torch.Tensor) or audio.dim() not in (2, 3):
            raise ValueError(f"audio must be [B, C, L0] or [B, L0], got {tuple(getattr(audio, 'shape', ()))}")
        return self.audio_transform.check(audio, audio_sr, self.audio_length, batched=True)[0]

    def check_mix(self, audio, raw_audio, seed, partners, snr_db):
        """Host-side validation / seeded draw of submit()'s mixing arguments (no device work) -> (partners, snr_db) for the mixer, (None,
        None) without one."""
        if self.mixer is None:
            if partners is not None or snr_db is not None:
                raise ValueError("partners / snr_db need a ClipPipeline built with mixer=")
            return None, None
        # the clips the mixer will see: `audio` itself (or its shape (B, L): submit_clips), or the [B, audio_length] buffer the audio
        # transform is about to fill
        clips = audio if raw_audio is None else (raw_audio.shape[0], self.audio_length)
        if partners is None or snr_db is None:
            drawn = self.mixer.sample(clips.shape[0] if isinstance(clips, torch.Tensor) else clips[0], torch.Generator().manual_seed(seed))
            partners = drawn[0] if partners is None else partners
            snr_db = drawn[1] if snr_db is None else snr_db
        return self.mixer.check(clips, partners, snr_db)

    def check_reverb(self, clips, seed, rir_index):
        """Host-side validation / seeded draw of the rooms (no device work) -> rir_index for the reverb, None without one.  `clips` is
        the [B, L] tensor the reverb will see or, when it does not exist yet, the pair (B, L)."""
        if self.reverb is None:
            if rir_index is not None:
                raise ValueError("rir_index needs a ClipPipeline built with reverb=")
            return None
        return self.reverb.check(clips, rir_index, seed)

    def _encode(self, slot, audio, wet, partners, snr_db, seed):
        """The STFT / mixer call of one batch on the current (side) stream: `wet` is None without a reverb."""
        if wet is not None and self.reverb_target == "dry":
            slot["x"] = self.stft(wet, seed=seed)[0]
            slot["y"] = self.stft(audio, want_x=False)[1]
            return
        audio = audio if wet is None else wet
        if self.mixer is not None:
            slot["x"], slot["y"] = self.mixer(audio, partners, snr_db, seed=seed)
        else:
            slot["x"], slot["y"] = self.stft(audio, seed=seed)    # replaces (frees) the tensors of two batches ago, after the wait on `consumed`

    def submit(self, frames, audio, seed, boxes=None, audio_sr=None, partners=None, snr_db=None, rir_index=None):
        """Enqueue the extraction of one batch: frames [B*T,3,H,W], audio [B,L] (both resident on the device).  The caller's
        stream must already hold the work that produced them (the side stream waits for it).
        With a transform, frames are the uint8 clips [B*T,H0,W0,3] or [B,T,H0,W0,3] and `boxes` the CPU crop boxes [B,4]; by default
        transform.sample_boxes(B, H0, W0, torch.Generator().manual_seed(seed)), so a pipelined and a serial run see the same crops.
        With an audio_transform, audio is the raw clips [B,C,L0] or [B,L0] (f32 or int16) at `audio_sr` Hz; they must resample to at
        least audio_length samples and are cropped to that.
        With a mixer, `partners` [B,K] int32 and `snr_db` [B] (CPU) choose the mixtures; by default
        mixer.sample(B, torch.Generator().manual_seed(seed)), which is also what mixer(audio, seed=seed) draws: a pipelined and a serial
        run see the same mixtures.
        With a reverb, `rir_index` [B] int32 (CPU) chooses each clip's room in reverb.rirs; by default
        reverb.sample_index(B, torch.Generator().manual_seed(seed)), which is also what reverb(audio, seed=seed) draws.  The clips
        (after the audio transform) are convolved from zero state."""
        if self.va is None:
            raise ValueError("submit() needs a ClipPipeline built with a video_attention (a bank-fed one takes submit_clips())")
        assert self.head - self.tail < self.depth, "pipeline full: get()/release() a batch first"
        slot = self.slots[self.head % self.depth]
        raw_audio = self.check_audio(audio, audio_sr)                        # everything is validated before any device work
        partners, snr_db = self.check_mix(audio, raw_audio, seed, partners, snr_db)
        rir_index = self.check_reverb(audio if raw_audio is None else (raw_audio.shape[0], self.audio_length), seed, rir_index)
        if self.transform is not None:
            raw, _, boxes = self.transform.check(frames, boxes, self.t)
            f, h0, w0, _ = raw.shape
            if boxes is None:
                boxes = self.transform.sample_boxes(f // self.t, h0, w0, torch.Generator().manual_seed(seed))
            h = w = self.transform.size
        elif boxes is not None:
            raise ValueError("boxes need a ClipPipeline built with transform=")
        else:
            f, _, h, w = frames.shape
        main = torch.cuda.current_stream()
        produced = torch.cuda.Event()
        produced.record(main)
        # the caller may drop its references right after this call: tell the caching allocator that the side stream still reads them
        frames.record_stream(self.side)
        audio.record_stream(self.side)
        with torch.cuda.stream(self.side):
            self.side.wait_event(produced)
            if slot["consumed"] is not None:
                self.side.wait_event(slot["consumed"])      # the training step that read this slot's buffers is past them
            if slot["attn"] is None or slot["attn"].shape != (f, 1, h, w):
                slot["attn"] = torch.empty(f, 1, h, w, device=frames.device, dtype=torch.float32)
            if self.transform is not None:
                if slot["frames"] is None or slot["frames"].shape != (f, 3, h, w):
                    slot["frames"] = torch.empty(f, 3, h, w, device=frames.device, dtype=torch.float32)
                frames = self.transform(raw, boxes=boxes, clip_frames=self.t, out=slot["frames"])
            self.va.attention_frames(frames, clip_frames=self.t, out=slot["attn"], finite_check=self.finite_check)
            if self.audio_transform is not None:
                nb = raw_audio.shape[0]
                if slot["audio"] is None or slot["audio"].shape != (nb, self.audio_length):
                    slot["audio"] = torch.empty(nb, self.audio_length, device=audio.device, dtype=torch.float32)
                audio = self.audio_transform(raw_audio, audio_sr, length=self.audio_length, out=slot["audio"])
            wet = None if self.reverb is None else self.reverb(audio, rir_index)
            self._encode(slot, audio, wet, partners, snr_db, seed)
            slot["ready"].record(self.side)
        self.head += 1

    def check_crop(self, b, seed, boxes, flip):
        """Host-side validation / seeded draw of submit_clips()'s crops (no device work) -> (boxes, flip) for bank.cut, (None, None)
        when there is nothing to warp."""
        if self.bank_crop is None:
            if boxes is not None or flip is not None:
                raise ValueError("boxes / flip need a ClipPipeline built with bank_crop=")
            return None, None
        if boxes is None or flip is None:
            drawn = self.bank_crop.sample(b, self.bank.frame_size, torch.Generator().manual_seed(seed))
            boxes = drawn[0] if boxes is None else boxes
            flip = drawn[1] if flip is None else flip
        return self.bank.check_warp(b, boxes, flip)

    def submit_clips(self, indices, seed, boxes=None, flip=None, *, attn_diff=False, partners=None, snr_db=None, rir_index=None):
        """Enqueue one batch cut from the bank: `indices` as ClipBank.batch takes them (CPU; checked before any device work), `seed`,
        `partners` and `snr_db` as in submit().  On the side stream bank.batch fills the slot's buffers, then the STFT / mixer call and
        the events are those of submit(); get() / release() do not change.  With a reverb the wet clips are reverb.bank_clips(bank, indices,
        rir_index): convolved from bank.audio, each clip with its recording's past.
        With a bank_crop, `boxes` [B,4] int32 and `flip` [B] bool (CPU) crop and mirror each clip's maps; by default
        bank_crop.sample(B, bank.frame_size, torch.Generator().manual_seed(seed)), which is what a serial
        bank.batch(indices, boxes=, flip=) with that draw sees: a pipelined and a serial run get the same crops."""
        if self.bank is None:
            raise ValueError("submit_clips needs a ClipPipeline built with bank=")
        assert self.head - self.tail < self.depth, "pipeline full: get()/release() a batch first"
        slot = self.slots[self.head % self.depth]
        bank = self.bank
        starts = bank.check_indices(indices)
        b = starts[0].numel()
        partners, snr_db = self.check_mix((b, bank.clip_samples), None, seed, partners, snr_db)
        rir_index = self.check_reverb((b, bank.clip_samples), seed, rir_index)
        if self.reverb is not None:
            self.reverb.check_bank(bank, b, rir_index, seed)
            floor = bank_floor(bank, indices)
        boxes, flip = self.check_crop(b, seed, boxes, flip)
        f, s = b * self.t, bank.frame_size
        main = torch.cuda.current_stream()
        produced = torch.cuda.Event()
        produced.record(main)                               # recordings banked on the caller's stream just before this call
        with torch.cuda.stream(self.side):
            self.side.wait_event(produced)
            if slot["consumed"] is not None:
                self.side.wait_event(slot["consumed"])
            if slot["attn"] is None or slot["attn"].shape != (f, 1, s, s):
                slot["attn"] = torch.empty(f, 1, s, s, device=bank.device, dtype=torch.float32)
            if slot.get("clips") is None or slot["clips"].shape != (b, bank.clip_samples):
                slot["clips"] = torch.empty(b, bank.clip_samples, device=bank.device, dtype=torch.float32)
            _, audio = bank.cut(*starts, attn_diff=attn_diff, out=(slot["attn"].view(b, 1, self.t, s, s), slot["clips"]), boxes=boxes, flip=flip)
            wet = None if self.reverb is None else self.reverb.cut(bank, starts[1], floor, rir_index)
            self._encode(slot, audio, wet, partners, snr_db, seed)
            slot["ready"].record(self.side)
        self.head += 1

    def get(self):
        """(attention frames [B,1,T,H,W], x_stft, y_stft) of the oldest submitted batch; the current stream waits for them."""
        assert self.tail < self.head, "nothing submitted"
        slot = self.slots[self.tail % self.depth]
        torch.cuda.current_stream().wait_event(slot["ready"])
        f, _, h, w = slot["attn"].shape
        return slot["attn"].view(f // self.t, 1, self.t, h, w), slot["x"], slot["y"]

    def release(self):
        """Call after the work that reads the batch handed out by get() has been enqueued on the current stream."""
        slot = self.slots[self.tail % self.depth]
        slot["consumed"] = torch.cuda.Event()
        slot["consumed"].record(torch.cuda.current_stream())
        self.tail += 1

    def drain(self):
        self.side.synchronize()
        if self.va is not None:                 # a bank-fed pipeline has no extractor: its maps were checked when they were banked
            self.va.check_finite()
