#!/usr/bin/env python
"""The reference's training loop (train_avse_frames.py:112-205) on the drop-in classes, with synthetic clips instead of the MUSICES
data loader (no datasets in this environment): frames -> VideoAttention (ViT-S/8, HIP) -> attention frames; audio -> STFT (+ noise);
sliding windows of `num_frames` frames through AV_Fusion_Model_Frames; loss / backward / Adam as the reference does them; a checkpoint
written and re-loaded through the reference's own file layout (utilities.py:162-204).  Extraction of the next batch runs on a second HIP
stream (ClipPipeline).

    python examples/train_synthetic.py [--steps 6] [--batch 4] [--num_frames 8] [--num_seq 3] [--framesize 256]
    python examples/train_synthetic.py --overfit --steps 300 --lr 1e-4 --log_every 20     # one fixed batch: the loss has to fall
    python examples/train_synthetic.py --raw_video 360x640 [--autocontrast]   # decoded uint8 clips through VideoTransform first
    python examples/train_synthetic.py --raw_audio [--compress_audio]         # 44.1 kHz stereo int16 clips through AudioTransform first
    python examples/train_synthetic.py --mix 2 --mix_snr 0 10                 # mix-and-separate: every clip + 2 others of the batch at 0..10 dB
    python examples/train_synthetic.py --reverb 16 [--reverb_target dry]      # every clip in one of 16 synthetic rooms, new rooms every epoch
                                                                              # (maavss_amd.Reverb; with --bank a clip hears its recording's
                                                                              # past); dry: the target stays the dry clip (dereverberation)
    python examples/train_synthetic.py --reverb 16 --rooms image --mix 1      # 16 shoebox rooms (image-source model) of 2 sources: a clip and
                                                                              # its partner are heard in the same room
    python examples/train_synthetic.py --reverb 16 --rooms image --calibrate t20   # the rooms' walls searched until the MEASURED T20 is the
                                                                              # requested time (Reverb.measure); prints requested against measured
    python examples/train_synthetic.py --clip 1.0 --watch 2                   # gradient-norm clipping; per-tensor histograms every 2 steps
    python examples/train_synthetic.py --val 2                                # every 2 steps: held-out loss and LSD, a checkpoint on improvement
    python examples/train_synthetic.py --val 2 --mix 1                        # also BSS-eval SDR / SIR / SAR of the held-out mixtures
    python examples/train_synthetic.py --bank 8 [--bank_storage u16]          # the ViT once per recording: maps and audio of 8 recordings in
                                                                              # HBM (ClipBank), every batch cut from them by clip index
    python examples/train_synthetic.py --bank 8 --bank_crop [--bank_flip 0.5] # a new random crop (and mirror image) of every clip's stored
                                                                              # maps in every step (maavss_amd.BankCrop): the map is cropped,
                                                                              # not the frame -- the ViT still runs once per recording
    python examples/train_synthetic.py --bank 8 --select [--val 2]            # every recording gets a silent and a frozen stretch; the bank's
                                                                              # activity pass finds them and maavss_amd.ClipSampler draws the
                                                                              # epochs from the clips that are left (held-out recordings: --val)
    python examples/train_synthetic.py --figures 2 [--figures-dir figures]    # every 2 steps the reference's callback images as PNGs
                                                                              # (maavss_amd.CallbackFigures: train_avse_frames.py:191-215)
    python examples/train_synthetic.py --audio_loss compressed [--compress 0.3 --loss_mix 0.3]    # the power-law compressed spectral loss
                                                                              # as the audio term (goes with --val, --mix and --overfit)
    python examples/train_synthetic.py --wave_loss si_sdr [--wave_weight 0.1]  # the clip-level SI-SDR (or snr) of the inverse STFT of the
                                                                              # joined windows, added to the objective (maavss_amd.WaveformLoss)
    python examples/train_synthetic.py --weight_decay 0.01 --ema 0.99 --skip_nonfinite --warmup 3 --schedule cosine [--val 2]
                                                                              # AdamW decay, averaged weights, the non-finite skip and a
                                                                              # warm-up + cosine rate (FusedAdam / maavss_amd.LRSchedule);
                                                                              # with --val both the raw and the averaged val_loss
"""
import argparse
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import maavss_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--num_frames", type=int, default=8)        # run_config.py: frames per window
    ap.add_argument("--num_seq", type=int, default=3)           # windows per optimizer step (train_avse_frames.py:143)
    ap.add_argument("--framesize", type=int, default=256)
    ap.add_argument("--fft_len", type=int, default=512)
    ap.add_argument("--hops_per_frame", type=int, default=8)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--overfit", action="store_true", help="train on ONE fixed batch (same clips, same noise draw) every step")
    ap.add_argument("--log_every", type=int, default=1)
    ap.add_argument("--precise", action="store_true", help="exact-f32 conv path instead of the 16-bit MFMA modes")
    ap.add_argument("--raw_video", default=None, metavar="HxW",
                    help="feed random uint8 HWC clips of this size through the GPU frame transform (RandomResizedCrop + Normalize)")
    ap.add_argument("--autocontrast", action="store_true", help="with --raw_video: the reference's --autocontrast (run_config.py)")
    ap.add_argument("--raw_audio", action="store_true",
                    help="feed 44.1 kHz stereo int16 clips through the GPU audio transform (downmix + resampling to 16 kHz)")
    ap.add_argument("--compress_audio", action="store_true", help="with --raw_audio: the reference's --compress_audio (run_config.py)")
    ap.add_argument("--mix", type=int, default=0, metavar="K",
                    help="mix-and-separate: add K other clips of the batch (1..4) to every clip's input; each clip is its own set of sinusoids")
    ap.add_argument("--mix_snr", type=float, nargs=2, default=(0.0, 10.0), metavar=("LO", "HI"), help="with --mix: signal-to-interferer range in dB")
    ap.add_argument("--reverb", type=int, default=0, metavar="N",
                    help="convolve every clip with one of N synthetic room responses of 0.5 s (maavss_amd.Reverb), N new rooms every epoch")
    ap.add_argument("--rooms", choices=("noise", "image"), default="noise",
                    help="with --reverb: decaying-noise responses (Reverb.make_rirs), or N shoebox rooms by the image-source model "
                         "(Reverb.sample_rooms + make_room_rirs); with --mix K every clip and its K partners are sources of one room")
    ap.add_argument("--room_sources", type=int, default=None, metavar="S",
                    help="with --rooms image: source positions per room (default: K + 1 with --mix K, else 1)")
    ap.add_argument("--calibrate", choices=("t20", "t30", "edt"), default=None,
                    help="with --rooms image: search every room's wall coefficient until this measured decay time is the requested one "
                         "(make_room_rirs(calibrate=)); prints requested against measured times of every epoch's rooms")
    ap.add_argument("--reverb_target", choices=("wet", "dry"), default="wet",
                    help="with --reverb: the target is the reverberant clip (wet) or the dry one (dry: not together with --mix)")
    ap.add_argument("--clip", type=float, default=None, metavar="MAX_NORM",
                    help="clip the global gradient norm (clip_grad_norm_'s rule, on the device: TrainStep(max_grad_norm=...))")
    ap.add_argument("--watch", type=int, default=0, metavar="N",
                    help="every N steps, the per-tensor gradient / parameter histograms wandb.watch would log (maavss_amd.ModelWatch)")
    ap.add_argument("--val", type=int, default=0, metavar="N",
                    help="every N steps, validate on one fixed seeded held-out batch (maavss_amd.Validator: train_av_net.py:147-181) and "
                         "save a checkpoint when the validation loss improves")
    ap.add_argument("--bank", type=int, default=0, metavar="R",
                    help="bank R synthetic recordings of 4 clips once (ViT + audio, maavss_amd.ClipBank: the reference's attn_frames_path / "
                         "use_audio_memmap), then draw every batch by clip index from a seeded permutation: no ViT in the step")
    ap.add_argument("--bank_storage", choices=("f32", "u16"), default="f32", help="with --bank: 4 or 2 bytes per map value")
    ap.add_argument("--bank_crop", action="store_true",
                    help="with --bank: cut every training clip through a fresh RandomResizedCrop box applied to its stored attention maps "
                         "(maavss_amd.BankCrop, ClipBank.batch(boxes=)); the held-out batch of --val keeps the whole frame")
    ap.add_argument("--bank_flip", type=float, default=0.0, metavar="P", help="with --bank_crop: mirror a clip's maps with probability P")
    ap.add_argument("--select", action="store_true",
                    help="with --bank: silence the first clip of every recording and freeze the frames of its last one, reject such clips by the "
                         "bank's activity statistics and iterate maavss_amd.ClipSampler's epochs instead of a hand-drawn permutation")
    ap.add_argument("--figures", type=int, default=0, metavar="N",
                    help="every N steps (the reference's cb_freq), run the step with collect=True and make the callback's images on the "
                         "device (maavss_amd.CallbackFigures), then write them as PNGs")
    ap.add_argument("--audio_loss", choices=("mse", "compressed"), default="mse",
                    help="the audio term of the loss: the reference's MSE of the STFT planes, or the power-law compressed spectral loss "
                         "(maavss_amd.SpectralLoss: TrainStep(audio_loss=...), and with --val Validator(audio_loss=...))")
    ap.add_argument("--compress", type=float, default=0.3, metavar="C", help="with --audio_loss compressed: the exponent, in (0, 1]")
    ap.add_argument("--loss_mix", type=float, default=0.3, metavar="L",
                    help="with --audio_loss compressed: the weight of the complex term, in [0, 1]; the magnitude term gets 1 - L")
    ap.add_argument("--wave_loss", choices=("si_sdr", "snr"), default=None,
                    help="add the clip-level waveform loss of the inverse STFT of the num_seq windows' joined outputs "
                         "(maavss_amd.WaveformLoss: TrainStep(wave_loss=...))")
    ap.add_argument("--wave_weight", type=float, default=1.0, metavar="W", help="with --wave_loss: its weight in the objective (dB per unit)")
    ap.add_argument("--figures-dir", default="figures", metavar="D", help="with --figures: where the PNGs go")
    ap.add_argument("--weight_decay", type=float, default=0.0, metavar="W", help="AdamW's decoupled decay on the tensors with two or more dimensions")
    ap.add_argument("--ema", type=float, default=None, metavar="D",
                    help="keep an exponential moving average of the weights with this decay (warmed up); with --val the averaged weights are "
                         "validated too, inside step.ema_weights()")
    ap.add_argument("--skip_nonfinite", action="store_true", help="skip an optimizer step whose gradient norm is NaN or infinite, on the device")
    ap.add_argument("--warmup", type=int, default=0, metavar="N", help="linear warm-up of the learning rate over N steps (maavss_amd.LRSchedule)")
    ap.add_argument("--schedule", choices=("constant", "linear", "cosine"), default="constant",
                    help="the rate after the warm-up: constant, or a linear / cosine decay to 0 at --steps")
    a = ap.parse_args()
    if a.select and not a.bank:
        ap.error("--select chooses among the clips of a bank: it goes with --bank")
    if a.bank_crop and not a.bank:
        ap.error("--bank_crop crops the maps of a bank: it goes with --bank")
    if a.bank_flip and not a.bank_crop:
        ap.error("--bank_flip is drawn with the crops: it goes with --bank_crop")
    if a.bank and (a.raw_video or a.raw_audio or a.overfit):
        ap.error("--bank holds transformed frames' maps and 16 kHz audio: it does not go with --raw_video, --raw_audio or --overfit")
    if a.reverb and a.reverb_target == "dry" and a.mix:
        ap.error("--reverb_target dry does not go with --mix: the target of a reverberant mixture is not built")
    if a.rooms == "image" and not a.reverb:
        ap.error("--rooms image chooses how --reverb N fills its table: it goes with --reverb")
    if a.calibrate and a.rooms != "image":
        ap.error("--calibrate searches the walls of image-source rooms: it goes with --reverb N --rooms image")
    room_sources = a.room_sources if a.room_sources is not None else a.mix + 1
    if a.rooms == "image" and a.mix and (room_sources < a.mix + 1 or a.batch % (a.mix + 1)):
        ap.error(f"--rooms image with --mix {a.mix}: groups of {a.mix + 1} clips share a room, so --room_sources must be at least {a.mix + 1} "
                 f"and --batch a multiple of it")
    dev = torch.device("cuda:0")
    b, nf, ns, w, hpf = a.batch, a.num_frames, a.num_seq, a.framesize, a.hops_per_frame
    t_total = nf + ns - 1                                      # frames per clip so that num_seq windows fit (av_dataset.py:251-278)
    hop, length, t_a = maavss_amd.calc_hop_size(t_total, hpf, 30, 16000)
    n_bins = a.fft_len // 2 + 1

    extractor = maavss_amd.VideoAttention(path_to_weights="dino_deitsmall8_pretrain.pth")      # random init when absent (no network)
    stft = maavss_amd.STFT(a.fft_len, hop, noise_std=0.1, device=dev)
    model = maavss_amd.AV_Fusion_Model_Frames([b, 2, hpf * nf, n_bins], [b, 1, nf, w, w], hpf, precise=a.precise).to(dev).train()
    audio_loss = maavss_amd.SpectralLoss(a.compress, a.loss_mix) if a.audio_loss == "compressed" else None
    schedule = None
    if a.warmup or a.schedule != "constant":
        schedule = maavss_amd.LRSchedule(a.lr, warmup_steps=a.warmup, total_steps=None if a.schedule == "constant" else max(a.steps, a.warmup + 1),
                                         kind=a.schedule)
    step = maavss_amd.TrainStep(model, lr=schedule if schedule is not None else a.lr, loss_coeff=0.001, num_seq=ns, max_grad_norm=a.clip,
                                audio_loss=audio_loss, weight_decay=a.weight_decay, ema_decay=a.ema, ema_warmup=a.ema is not None,
                                skip_nonfinite=a.skip_nonfinite,
                                wave_loss=maavss_amd.WaveformLoss(stft, kind=a.wave_loss) if a.wave_loss else None, wave_weight=a.wave_weight)
    watch = maavss_amd.ModelWatch(step, log_freq=a.watch) if a.watch else None
    figures = maavss_amd.CallbackFigures(stft) if a.figures else None
    transform = None
    if a.raw_video:
        h0, w0 = (int(v) for v in a.raw_video.lower().split("x"))
        transform = maavss_amd.VideoTransform(w, autocontrast=a.autocontrast)
    audio_transform, raw_sr = None, 44100
    if a.raw_audio:
        audio_transform = maavss_amd.AudioTransform(16000, compress_audio=a.compress_audio)
        raw_length = audio_transform.input_length(length, raw_sr)      # the fewest 44.1 kHz samples that give `length` at 16 kHz
    mixer = maavss_amd.Mixer(stft, a.mix, tuple(a.mix_snr)) if a.mix else None
    reverb = maavss_amd.Reverb(8000, rt60=(0.2, 0.5), device=dev) if a.reverb else None

    def make_rooms(seed):
        """The epoch's table: N decaying-noise responses, or N image-source rooms of room_sources sources each."""
        if a.rooms == "image":
            dims, mic, sources, rt60 = reverb.sample_rooms(a.reverb, torch.Generator().manual_seed(seed), sources=room_sources)
            reverb.make_room_rirs(dims, mic, sources, rt60=rt60, calibrate=a.calibrate)
            if a.calibrate:                                      # set-up, once an epoch: the calibration synchronises once a round
                pairs = ", ".join(f"{want:.3f}->{got:.3f}{'' if ok else '!'}" for want, got, ok in
                                  zip(rt60.tolist(), reverb.room_measured.tolist(), reverb.room_converged.tolist()))
                print(f"[rooms] seed {seed}: requested -> measured {a.calibrate} after {reverb.calibration_rounds} rounds (s): {pairs}", flush=True)
        else:
            reverb.make_rirs(a.reverb, seed=seed)

    def room_kw(seed):
        """--rooms image with --mix K: consecutive groups of K + 1 clips are the sources of one room and each other's partners."""
        if a.rooms != "image" or not a.mix:
            return {}
        group = a.mix + 1
        member = torch.arange(b, dtype=torch.int32).view(-1, group)
        partners = torch.stack([torch.cat([member[:, :j], member[:, j + 1:]], dim=1) for j in range(group)], dim=1).reshape(b, a.mix)
        return dict(partners=partners.contiguous(), rir_index=reverb.sample_room_index(b, torch.Generator().manual_seed(seed), group))

    if reverb is not None:
        make_rooms(0)                                            # epoch 0's rooms; submit() below makes the later ones
    if not a.bank:
        pipe = maavss_amd.ClipPipeline(extractor, stft, clip_frames=t_total, transform=transform, audio_transform=audio_transform,
                                       audio_length=length if a.raw_audio else None, mixer=mixer, reverb=reverb, reverb_target=a.reverb_target)

    g = torch.Generator().manual_seed(0)

    def batch(b=b, t_total=t_total, length=length):
        """b clips of t_total frames and `length` samples (--bank: one recording = one long clip)."""
        if transform is not None:
            frames = torch.randint(0, 256, (b, t_total, h0, w0, 3), generator=g, dtype=torch.uint8)
        else:
            frames = torch.rand(b * t_total, 3, w, w, generator=g)
        if mixer is not None:
            # "instruments": every clip its own three partials (a random fundamental in 110..880 Hz, harmonics 1-3) over a little noise,
            # so that the clips the mixer adds are other sources, not more of the same noise
            n, sr = (raw_length, raw_sr) if audio_transform is not None else (length, 16000)
            f0 = 110.0 * 2.0 ** (3.0 * torch.rand(b, 1, generator=g))
            t = torch.arange(n, dtype=torch.float32)[None, :] / sr
            audio = 0.02 * torch.randn(b, n, generator=g)
            for h in (1, 2, 3):
                audio = audio + (0.3 / h) * torch.sin(2 * torch.pi * h * f0 * t + 2 * torch.pi * torch.rand(b, 1, generator=g))
            if audio_transform is not None:
                audio = (32767 * audio[:, None, :].expand(b, 2, n)).to(torch.int16)
        elif audio_transform is not None:
            audio = (0.3 * 32767 * torch.randn(b, 2, raw_length, generator=g)).clamp(-32768, 32767).to(torch.int16)
        else:
            audio = (0.3 * torch.randn(b, length, generator=g)).clamp(-1, 1)
        return frames.to(dev), audio.to(dev)

    fixed = batch() if a.overfit else None
    sr_arg = dict(audio_sr=raw_sr) if a.raw_audio else {}

    if not a.bank:
        def submit(seed):
            pipe.submit(*(fixed or batch()), seed=seed, **sr_arg, **room_kw(seed))
    else:
        # the reference's cached attention frames and audio memmap (train_avse_frames.py:50, av_dataset.py:136-147), on the device: every
        # recording goes through the ViT once, here; clip k of a recording starts frame_hop frames after clip k - 1
        per_rec, frame_hop = 4, max(1, t_total // 2)
        n_f = (per_rec - 1) * frame_hop + t_total
        n_s = (per_rec - 1) * frame_hop * 16000 // 30 + 1 + length
        keep = per_rec - 2 if a.select else per_rec                  # --select: two clips of every recording are made to be rejected
        n_rec = a.bank + (-(-b // keep) if a.val else 0)             # --val: the last recordings are held out
        bank = maavss_amd.ClipBank(w, t_total, frame_hop, hpf, hop, capacity_frames=n_rec * n_f, capacity_samples=n_rec * n_s,
                                   storage=a.bank_storage, device=dev)
        for _ in range(n_rec):
            frames, audio = batch(1, n_f, n_s)
            if a.select:
                audio[0, :length] = 0.0                                  # clip 0: digital silence
                frames[-t_total:] = frames[-1].clone()                   # the last clip: one frame, repeated
            bank.add_recording(audio[0], frames=frames, video_attention=extractor)
        n_train = a.bank * per_rec
        if n_train < b:
            ap.error(f"--bank {a.bank} holds {n_train} clips, fewer than one batch of {b}")
        print(f"bank: {len(bank)} clips of {n_rec} recordings, {bank.maps.numel() * bank.maps.element_size() / 1e6:.2f} MB of maps "
              f"({a.bank_storage}), {bank.audio.numel() * 4 / 1e6:.2f} MB of audio", flush=True)
        bank_crop = maavss_amd.BankCrop(flip=a.bank_flip) if a.bank_crop else None
        pipe = maavss_amd.ClipPipeline(None, stft, clip_frames=t_total, bank=bank, mixer=mixer, reverb=reverb, reverb_target=a.reverb_target,
                                       bank_crop=bank_crop)
        # the held-out batch is not augmented: the whole frame, nobody mirrored (the extractor's maps come back as they are stored)
        uncropped = dict(boxes=torch.tensor([[0, 0, w, w]] * b, dtype=torch.int32), flip=torch.zeros(b, dtype=torch.bool)) if a.bank_crop else {}
        g_order, order = torch.Generator().manual_seed(0), []
        if a.select:
            # one pass over the bank on the device (ClipBank.activity), the thresholds there too, one copy of a byte per clip back
            limits = dict(min_rms_db=-50.0, min_motion=1e-4)
            sampler = maavss_amd.ClipSampler(bank, b, recordings=range(a.bank), seed=0, **limits)
            print(f"select: {sampler.accepted.numel()} of {sampler.n_considered} training clips accepted, {len(sampler)} steps an epoch; rejected "
                  + ", ".join(f"{k} {v}" for k, v in sampler.rejected.items() if v), flush=True)

            def batches():
                e = 0
                while True:
                    yield from sampler.epoch(e)
                    e += 1
            epochs = batches()

            def submit(seed):
                pipe.submit_clips(next(epochs), seed=seed, **room_kw(seed))
        else:
            def submit(seed):
                while len(order) < b:                                    # the next epoch's permutation of the training clips
                    order.extend(torch.randperm(n_train, generator=g_order).tolist())
                pipe.submit_clips([order.pop(0) for _ in range(b)], seed=seed, **room_kw(seed))

    if reverb is not None:
        # an epoch: the sampler's, or one pass over the bank's training clips, or (clips drawn on the fly) 8 steps
        epoch_steps = len(sampler) if a.select else (max(1, n_train // b) if a.bank else 8)
        submit_clips = submit

        def submit(seed):
            if seed and seed % epoch_steps == 0:
                # the side stream may still read the old table: keep its memory until that work is done.  The new one is written on
                # this stream in front of the submit, which the side stream waits for
                reverb.rirs.record_stream(pipe.side)
                make_rooms(seed // epoch_steps)
            submit_clips(seed)

    held_out = validator = val_dir = None
    if a.val:
        # one held-out batch from a generator of its own (the training stream's draws stay what they are without --val), extracted once
        if a.select:
            held = maavss_amd.ClipSampler(bank, b, recordings=range(a.bank, n_rec), shuffle=False, **limits)      # the split by file
            print(f"select: {held.accepted.numel()} of {held.n_considered} held-out clips accepted", flush=True)
            pipe.submit_clips(next(held.epoch(0)), seed=12345, **uncropped, **room_kw(12345))
        elif a.bank:
            pipe.submit_clips(list(range(n_train, n_train + b)), seed=12345, **uncropped, **room_kw(12345))
        else:
            g_train, g = g, torch.Generator().manual_seed(12345)
            frames_v, audio_v = batch()
            pipe.submit(frames_v, audio_v, seed=12345, **sr_arg, **room_kw(12345))
            g = g_train
            if mixer is not None and not a.raw_audio:
                # what kind of error the held-out mixtures hold before any separation (BSS-eval, maavss_amd.bss_eval_metrics): the same
                # seed draws the partners and ratios the pipeline's mixer call draws.  The Mixer has no output for the interferers'
                # waveform: `mixture - audio_v` is a torch subtraction.  The model's own output is scored the same way once it is a
                # waveform: Validator(bss_filter=...).add_recording(enhancer, mixture, clean, attn=..., others=...)
                mixture = mixer(audio_v, seed=12345, return_mixture=True)[2]
                bss = maavss_amd.Validator(model, bss_filter=512)
                bss.add_waves(mixture, audio_v, others=mixture - audio_v)
                r = bss.result()
                print(f"held-out mixtures, 512-tap BSS-eval over {r['sdr_db_n_finite']} clips: SDR {r['sdr_db']:.2f} dB  SIR {r['sir_db']:.2f} dB  "
                      f"SAR {r['sar_db']:.2f} dB", flush=True)
        held_out = tuple(t.clone() for t in pipe.get())
        pipe.release()
        validator = maavss_amd.Validator(model, loss_coeff=0.001, num_seq=ns, audio_loss=audio_loss)
        val_dir = tempfile.TemporaryDirectory()
    submit(0)
    for i in range(a.steps):
        submit(0 if a.overfit else i + 1)                                # extraction of the next batch: side stream
        attn, x_stft, y_stft = pipe.get()                        # [B,1,T,H,W], [B,2,T_a,F] x 2
        if figures is not None and i % a.figures == 0:
            # train_avse_frames.py:143-148, 173-177, 191-215: the stitched outputs, then the images of clip 0 -- launches only; the
            # copies happen in save_png.  (The synthetic clips keep no video next to their attention frames: two strips, not three.)
            losses, output_stft, output_attn = step.sliding_window_step(x_stft, y_stft, attn, attn, nf, hpf, collect=True)
            logs = figures(y_stft, output_stft, attn, output_attn)
            paths = maavss_amd.save_png(logs, a.figures_dir, i)
            print(f"step {i}: {len(paths)} images in {a.figures_dir}/ (" + ", ".join(f"{k} {tuple(logs[k].shape)}" for k in maavss_amd.figures.IMAGE_KEYS)
                  + f"); audio_input {tuple(logs['audio_input'].shape)}, audio_output {tuple(logs['audio_output'].shape)}", flush=True)
        else:
            losses = step.sliding_window_step(x_stft, y_stft, attn, attn, nf, hpf)
        pipe.release()
        logs = watch.after_step() if watch is not None else None
        if i % a.log_every == 0 or i == a.steps - 1:
            clip = "" if a.clip is None else f"  |g| {step.opt.grad_norm.item():.4g}  scale {step.opt.clip_scale.item():.4g}"
            parts = "" if audio_loss is None else "  (magnitude {:.5f}, complex {:.5f})".format(*step.loss_parts.tolist())
            rate = "" if schedule is None else f"  lr {step.opt.lr:.3g}"
            skips = "" if not a.skip_nonfinite else f"  skipped {step.opt.skipped_steps.item()}"
            wave = "" if not a.wave_loss else f"  {a.wave_loss} loss {step.wave['loss'].item():.3f} dB"
            print(f"step {i}: a_loss {losses[0].item():.5f}{parts}  v_loss {losses[1].item():.5f}  loss {losses[2].item():.5f}{wave}{clip}{rate}{skips}",
                  flush=True)
        if validator is not None and (i + 1) % a.val == 0:
            attn_v, x_v_stft, y_v_stft = held_out
            model.eval()
            validator.reset()
            validator.add_clips(x_v_stft, y_v_stft, attn_v, attn_v, nf, hpf)
            res = validator.result()
            if a.ema is not None:
                # the same held-out batch through the averaged weights (BatchNorm keeps its live running statistics)
                with step.ema_weights():
                    validator.reset()
                    validator.add_clips(x_v_stft, y_v_stft, attn_v, attn_v, nf, hpf)
                    res_ema = validator.result()
                print(f"step {i}: val_loss raw {res['val_loss']:.5f}  averaged {res_ema['val_loss']:.5f} ({step.opt.ema_updates} updates)", flush=True)
            model.train()
            print(f"step {i}: validation {res}", flush=True)
            key = "val_loss" if audio_loss is None else "val_objective"          # the loss the step trains on
            if validator.improved(res, key=key):
                maavss_amd.save_checkpoint(model.state_dict(), step.opt.state_dict(), i, res[key], "synthetic-best", val_dir.name,
                                           ema_dict=step.opt.ema_state_dict() if a.ema is not None else None,
                                           schedule_dict=schedule.state_dict() if schedule is not None else None)
                print(f"step {i}: {key} {res[key]:.5f} improved: checkpoint saved", flush=True)
        if logs is not None:
            # with wandb: wandb.log({k: wandb.Histogram(np_histogram=v) for k, v in logs.items() if not k.startswith("nonfinite/")})
            bad = [k for k in logs if k.startswith("nonfinite/")]
            counts, edges = logs["gradients/fc2.weight"]
            print(f"step {i}: {len(logs) - len(bad)} histograms; gradients/fc2.weight in [{edges[0]:.3g}, {edges[-1]:.3g}], fullest bin "
                  f"{int(counts.argmax())} of {len(counts)}; tensors with non-finite values: {len(bad)}", flush=True)
    pipe.drain()
    if val_dir is not None:
        val_dir.cleanup()

    with tempfile.TemporaryDirectory() as cp_dir:
        maavss_amd.save_checkpoint(model.state_dict(), step.opt.state_dict(), 0, losses[2].item(), "synthetic", cp_dir)
        fresh = maavss_amd.AV_Fusion_Model_Frames([b, 2, hpf * nf, n_bins], [b, 1, nf, w, w], hpf).to(dev)
        opt = maavss_amd.FusedAdam(fresh, lr=a.lr)
        maavss_amd.load_checkpoint(fresh, opt, cp_dir, auto=True, load_opt=True)
        assert opt.weight_decay == a.weight_decay
        same = all(torch.equal(p, q) for p, q in zip(model.state_dict().values(), fresh.state_dict().values()))
        print("checkpoint round trip:", "ok" if same else "MISMATCH")
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
