"""Validation on the device: held-out loss and per-clip quality metrics of waveforms and spectra.

The reference validates (train_avse_frames.py:55-65 splits off a validation set; train_av_net.py:147-181 runs `model.eval()` +
`torch.no_grad()` over `val_steps` batches, averages the loss and saves a checkpoint only when it improves).  `TrainStep` is
autograd-free and always trains; this module is the loss-only path next to it, and the measures an `Enhancer` output or a `Mixer`
example is judged by (csrc/quality_metrics.hip: f64 sums of the f32 data in a fixed order, no floating-point atomics).

* `plan_wave_chunks` -- the host-side chunk planner of the wave metrics (pure, no device)
* `wave_metrics`     -- per row of est [B, L] against ref [B, L]: Sxx, Syy, Sxy, See, Srr, SNR, SI-SDR, segmental SNR
* `spectrum_metrics` -- per row of pred [B, 2, T, F] against tgt: squared-error sum and log-spectral distance
* `Validator`        -- an additive device accumulator of both over batches, clips and recordings; `result()` makes the one copy;
                        with `intelligibility_sr=` also of STOI and ESTOI per clip (maavss_amd/stoi.py, csrc/stoi.hip), with
                        `bss_filter=` also of BSS-eval SDR, SIR and SAR against known other sources (maavss_amd/bss.py, csrc/bss_eval.hip)

Definitions (include/maavss.h states them next to the entry points; tests/quality_twin.py is their float64 restatement):
  snr_db = 10 log10(Sxx / See), si_sdr_db = 10 log10(alpha^2 Sxx / Srr) with alpha = Sxy / Sxx and Srr = sum (est - alpha ref)^2 summed
  directly, seg_snr_db = the mean over the complete frames of seg_len samples whose reference is not silent of the frame's SNR clamped
  to [-10, 35] dB.  No epsilon: est == ref gives +inf, a silent reference NaN, a non-finite sample makes its row NaN.
Nothing here synchronises with the host before `Validator.result()`.
"""
from collections import namedtuple

import torch

from ._lib import MaavssError, call, column_dict, ptr, query, require_cuda, require_same_shape, stream_ptr, wave_rows, workspace
from .bss import BSS_COLUMNS, BSS_DB, BSS_MAX_FILTER, bss_eval_metrics
from .spectral_loss import SpectralLoss
from .stoi import stoi_metrics
from .trainer import sliding_windows

WAVE_COLUMNS = ("sxx", "syy", "sxy", "see", "srr", "snr_db", "si_sdr_db", "seg_snr_db", "n_frames")
WAVE_DB = ("snr_db", "si_sdr_db", "seg_snr_db")            # columns 5..7 of a wave_metrics row
_DB0 = WAVE_COLUMNS.index("snr_db")


def wave_chunk():
    """CH: the most samples one workgroup of the wave metrics reduces (a constant of the library); seg_len may not exceed it."""
    return int(query("maavss_wave_metrics_chunk"))


def plan_wave_chunks(length, seg_len, ch):
    """[(start, n)]: one row of `length` samples cut into chunks of floor(ch / seg_len) * seg_len samples -- a whole number of frames of
    seg_len samples each, so that no frame of the segmental SNR is split; the last chunk takes what is left, the row's trailing partial
    frame included.  Every sample is in exactly one chunk.  The library cuts every row the same way (one workgroup per chunk)."""
    length, seg_len, ch = int(length), int(seg_len), int(ch)
    if length < 1:
        raise ValueError("length must be >= 1")
    if not 1 <= seg_len <= ch:
        raise ValueError(f"seg_len must be in 1..{ch} (the chunk length), got {seg_len}")
    cl = ch // seg_len * seg_len
    return [(a, min(cl, length - a)) for a in range(0, length, cl)]


def wave_metrics(est, ref, seg_len=256):
    """est, ref: f32 cuda [L] or [B, L], samples contiguous, any row stride >= 0 (rows may overlap) and any 4-byte-aligned offset -- a slice
    `clean[start:start + n]` is taken as it is.  -> dict of device f64 tensors [B]: sxx, syy, sxy, see, srr, snr_db, si_sdr_db, seg_snr_db,
    n_frames, and "raw" [B, 9], the one buffer they are columns of.  Only enqueues launches on the current stream."""
    est, ref = wave_rows(est, "est"), wave_rows(ref, "ref")
    require_same_shape(est, ref)
    ch = wave_chunk()
    if not 1 <= int(seg_len) <= ch:
        raise ValueError(f"seg_len must be in 1..{ch}, got {seg_len}")
    require_cuda(est, ref)
    b, n = est.shape
    out = torch.empty(b, len(WAVE_COLUMNS), dtype=torch.float64, device=est.device)
    nbytes = int(query("maavss_wave_metrics_ws_bytes", b, n, int(seg_len)))
    ws = workspace(nbytes, est.device)
    call("maavss_wave_metrics", ptr(est), est.stride(0), ptr(ref), ref.stride(0), b, n, int(seg_len), ptr(out), ptr(ws), nbytes, stream_ptr())
    return column_dict(out, WAVE_COLUMNS)


def spectrum_metrics(pred, tgt, lsd_floor=1e-10):
    """pred, tgt: f32 cuda [B, 2, T, F] (real and imaginary planes, as the model's audio output and its target) -> dict of device f64
    tensors [B]: sqerr (sum of the squared differences over the 2 T F elements: the numerator of the MSE) and lsd_db (log-spectral distance
    in dB over the powers re^2 + im^2, floored at `lsd_floor`), and "raw" [B, 2]."""
    for t, what in ((pred, "pred"), (tgt, "tgt")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 2 or t.numel() == 0:
            raise ValueError(f"{what} must be a non-empty float32 tensor [B, 2, T, F], got {tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))}")
    if pred.shape != tgt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and tgt {tuple(tgt.shape)} differ in shape")
    if not float(lsd_floor) > 0.0:
        raise ValueError("lsd_floor must be > 0 (a power)")
    require_cuda(pred, tgt)
    pred, tgt = pred.contiguous(), tgt.contiguous()
    b, _, t, f = pred.shape
    out = torch.empty(b, 2, dtype=torch.float64, device=pred.device)
    nbytes = int(query("maavss_spectrum_metrics_ws_bytes", b, t))
    ws = workspace(nbytes, pred.device)
    call("maavss_spectrum_metrics", ptr(pred), ptr(tgt), b, t, f, float(lsd_floor), ptr(out), ptr(ws), nbytes, stream_ptr())
    return {"sqerr": out[:, 0], "lsd_db": out[:, 1], "raw": out}


def sqerr_rows(pred, tgt):
    """pred, tgt: f32 cuda, same shape [B, ...] -> device f64 [B]: the sum of the squared differences per batch row (the attention term)."""
    if pred.shape != tgt.shape or pred.dtype != torch.float32 or tgt.dtype != torch.float32 or pred.dim() < 1 or pred.numel() == 0:
        raise ValueError(f"pred and tgt must be non-empty float32 tensors of one shape, got {tuple(pred.shape)} and {tuple(tgt.shape)}")
    require_cuda(pred, tgt)
    pred, tgt = pred.contiguous(), tgt.contiguous()
    b = pred.shape[0]
    n = pred.numel() // b
    out = torch.empty(b, dtype=torch.float64, device=pred.device)
    nbytes = int(query("maavss_sqerr_rows_ws_bytes", b, n))
    ws = workspace(nbytes, pred.device)
    call("maavss_sqerr_rows", ptr(pred), ptr(tgt), b, n, ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


# the accumulator: [stft sqerr, stft elements, lsd sum, windows, attn sqerr, attn elements], then five numbers {sum of the finite values,
# count finite, +inf, -inf, NaN} for each wave metric of the estimates, of the noisy inputs, and of estimate minus noisy per clip
_SUMS = ("stft", "lsd", "attn")
_GROUPS = ("est", "noisy", "gain")
_ACC_LEN = 2 * len(_SUMS) + 5 * len(WAVE_DB) * len(_GROUPS)
# the second accumulator, only with intelligibility_sr: the same five numbers for stoi and estoi of the same three groups
_INTEL = ("stoi", "estoi")
_INTEL_LEN = 5 * len(_INTEL) * len(_GROUPS)
# the third accumulator, only with bss_filter: the same five numbers for sdr_db, sir_db and sar_db of the same three groups
_BSS_LEN = 5 * len(BSS_DB) * len(_GROUPS)
_BSS0 = BSS_COLUMNS.index("sdr_db")
# the fourth accumulator, only with audio_loss: [S_mag, S_cplx, elements] of the spectral loss over the model's audio outputs
_SPEC_LEN = 3
_COUNTS = ("n_finite", "n_posinf", "n_neginf", "n_nan")

# What differs between the families of per-clip metrics (everything else add_waves, result() and the buffer's layout do once for all):
#   names    the columns accumulated, 15 numbers each (five per group)
#   attr     the Validator attribute that views the family's part of the buffer (the first family's is the tail of `.acc`)
#   metric   (validator, x, ref, others) -> the raw [B, cols] tensor of x against ref;  col0: its first accumulated column
#   counts   which of _COUNTS result() reports (a score that is a correlation is never infinite)
#   clips    the family that counts the clips: result() takes n_clips from its est group and leaves out a noisy_ / _improvement key
#            nothing was added to; the others always report all their keys
#   enabled  validator -> bool
_Family = namedtuple("_Family", "names attr metric col0 counts clips enabled")
_FAMILIES = (
    _Family(WAVE_DB, None, lambda v, x, ref, oth: wave_metrics(x, ref, v.seg_len), _DB0, _COUNTS, True, lambda v: True),
    _Family(_INTEL, "acc_intel", lambda v, x, ref, oth: stoi_metrics(x, ref, v.intelligibility_sr), 0, ("n_finite", "n_nan"), False,
            lambda v: v.intelligibility_sr is not None),
    _Family(BSS_DB, "acc_bss", lambda v, x, ref, oth: bss_eval_metrics(x, ref, oth, v.bss_filter), _BSS0, _COUNTS, False,
            lambda v: v.bss_filter is not None),
)


class Validator:
    """Held-out loss and quality metrics, accumulated on the device.

        val = maavss_amd.Validator(model, loss_coeff=0.001, num_seq=3)
        model.eval()
        val.reset()
        for x_stft, y_stft, attn in held_out:
            val.add_clips(x_stft, y_stft, attn, attn, num_frames, hops_per_frame)
        val.add_recording(enhancer, noisy, clean, attn=maps)
        res = val.result()                      # the one device-to-host copy
        if val.improved(res):
            save_checkpoint(...)                # train_av_net.py:174-181
        model.train()

    The accumulator is one small f64 device tensor (`.acc`) of sums and counts only, so it is additive: the element-wise sum of the
    accumulators of several ranks is the accumulator of their data.  `add_*` enqueue kernels on the current stream and never wait."""

    def __init__(self, model, loss_coeff=0.001, num_seq=1, seg_len=256, lsd_floor=1e-10, audio_loss=None, intelligibility_sr=None,
                 bss_filter=None):
        """audio_loss: a maavss_amd.SpectralLoss; with it add_windows also runs its forward-only form on the model's audio output and
        adds the two sums and the element count into a fourth accumulator (`.acc_spec`), and result() gains val_loss_spectral_mag,
        val_loss_spectral_cplx, val_loss_spectral and val_objective.  None (the default): nothing of that is launched or reported.
        intelligibility_sr: the sample rate of the waves given to add_waves / add_recording; with it they also add STOI and ESTOI
        (maavss_amd.stoi_metrics) of the estimate, of the noisy input and of estimate minus noisy per clip, into a second small
        accumulator (`.acc_intel`), and result() gains their keys.  None (the default): nothing of that is launched or reported.
        bss_filter: the length (1..512 taps) of the BSS-eval distortion filter; with it add_waves / add_recording also add sdr_db, sir_db
        and sar_db (maavss_amd.bss_eval_metrics, against the `others` they are given) of the same three groups into a third accumulator
        (`.acc_bss`), and result() gains their keys.  None (the default): nothing of that is launched or reported."""
        if bss_filter is not None and (isinstance(bss_filter, bool) or not isinstance(bss_filter, int) or not 1 <= bss_filter <= BSS_MAX_FILTER):
            raise ValueError(f"bss_filter must be None or an integer in 1..{BSS_MAX_FILTER} (taps), got {bss_filter!r}")
        if intelligibility_sr is not None and (isinstance(intelligibility_sr, bool) or not isinstance(intelligibility_sr, int)
                                               or intelligibility_sr < 1):
            raise ValueError(f"intelligibility_sr must be None or a positive integer (samples per second), got {intelligibility_sr!r}")
        if audio_loss is not None and not isinstance(audio_loss, SpectralLoss):
            raise ValueError(f"audio_loss must be None or a maavss_amd.SpectralLoss, got {audio_loss!r}")
        if int(num_seq) < 1:
            raise ValueError("num_seq must be >= 1")
        if int(seg_len) < 1:
            raise ValueError("seg_len must be >= 1")
        if not float(lsd_floor) > 0.0:
            raise ValueError("lsd_floor must be > 0 (a power)")
        self.model, self.loss_coeff, self.num_seq = model, float(loss_coeff), int(num_seq)
        self.seg_len, self.lsd_floor = int(seg_len), float(lsd_floor)
        self.intelligibility_sr = intelligibility_sr
        self.bss_filter = bss_filter
        self.audio_loss = audio_loss
        self.acc = None
        self.acc_intel = None        # with intelligibility_sr: the tail of the allocation `acc` heads, so that result() makes one copy
        self.acc_bss = None          # with bss_filter: the tail after that
        self.acc_spec = None         # with audio_loss: the last tail
        self._buf = None
        self.best = None

    def reset(self):
        """Clear the accumulator (the best val_loss `improved` keeps is not touched)."""
        if self._buf is not None:
            self._buf.zero_()

    def _layout(self):
        """([(family, its offset in _buf)] of the enabled families, the length of _buf): the sums, the families in table order, then
        the spectral tail"""
        o, fams = 2 * len(_SUMS), []
        for f in _FAMILIES:
            if f.enabled(self):
                fams.append((f, o))
                o += 5 * len(f.names) * len(_GROUPS)
        return fams, o + (0 if self.audio_loss is None else _SPEC_LEN)

    def _acc(self, dev):
        if self.acc is None:
            fams, n = self._layout()
            self._buf = torch.zeros(n, dtype=torch.float64, device=dev)
            self.acc = self._buf[:_ACC_LEN]
            for f, o in fams[1:]:
                setattr(self, f.attr, self._buf[o:o + 5 * len(f.names) * len(_GROUPS)])
            if self.audio_loss is not None:
                self.acc_spec = self._buf[n - _SPEC_LEN:]
        return self.acc

    def _buf_len(self):
        return self._layout()[1]

    def _slot(self, kind):
        o = 2 * _SUMS.index(kind)
        return self.acc[o:o + 2]

    def _check_eval(self):
        if self.model.training:
            raise ValueError("the model is in training mode: call model.eval() first (train_av_net.py:147); a validation pass must "
                             "not update the BatchNorm running statistics")

    def add_windows(self, x_a, x_v, y_a, y_v):
        """One batch of windows: x_a [B,2,T_a,F], x_v [B,1,T,H,W] and the targets y_a [B,2,a,F], y_v [B,1,H,W] as TrainStep takes them.
        Forward only (the public eval forward under no_grad: no gradient buffer is written, BatchNorm reads its running statistics)."""
        self._check_eval()
        require_cuda(x_a, x_v, y_a, y_v)
        with torch.no_grad():
            a, v, _ = self.model(x_a, x_v)
        if a.shape != y_a.shape or v.shape != y_v.shape:
            raise ValueError(f"targets {tuple(y_a.shape)}, {tuple(y_v.shape)} do not match the model's outputs {tuple(a.shape)}, {tuple(v.shape)}")
        self._acc(a.device)
        st = stream_ptr()
        spec = spectrum_metrics(a, y_a, self.lsd_floor)["raw"]
        b = spec.shape[0]
        call("maavss_metric_add_sum", ptr(spec), b, 2, float(a.numel() // b), ptr(self._slot("stft")), st)
        call("maavss_metric_add_sum", ptr(spec[:, 1]), b, 2, 1.0, ptr(self._slot("lsd")), st)
        attn = sqerr_rows(v, y_v)
        call("maavss_metric_add_sum", ptr(attn), b, 1, float(v.numel() // b), ptr(self._slot("attn")), st)
        if self.audio_loss is not None:
            rows = self.audio_loss(a, y_a)["rows"]
            # add_sum adds a sum to acc[0] and n * weight to acc[1]: S_cplx and the elements into [1:3], then S_mag into [0] (and 0 into [1])
            call("maavss_metric_add_sum", ptr(rows[:, 1]), b, 2, float(a.numel() // b), ptr(self.acc_spec[1:]), st)
            call("maavss_metric_add_sum", ptr(rows), b, 2, 0.0, ptr(self.acc_spec), st)

    def add_clips(self, x_stft, y_stft, x_attn, y_attn, num_frames, hops_per_frame):
        """One batch of clips, cut into the `num_seq` windows TrainStep.sliding_window_step trains on (the same slicing code)."""
        self._check_eval()
        for _, xa, xv, ya, yv in sliding_windows(x_stft, y_stft, x_attn, y_attn, num_frames, hops_per_frame, self.num_seq):
            self.add_windows(xa, xv, ya, yv)

    def add_waves(self, est, ref, noisy=None, others=None):
        """Per-row wave metrics of est against ref, each row one clip; with `noisy` (the unprocessed input of the same rows) also its own
        metrics against ref and, per clip, estimate minus noisy: the improvements (SNRi, SI-SDRi, segmental SNRi).  `others` ([B, L] or
        [B, K, L], the other sources of each row's mixture) is read only with bss_filter."""
        if others is not None and self.bss_filter is None:
            raise ValueError("others is given but this Validator was built without bss_filter")
        for f, o in self._layout()[0]:
            m = f.metric(self, est, ref, others)["raw"]
            self._acc(m.device)
            st = stream_ptr()
            (b, cols), k = m.shape, len(f.names)
            slot = [self._buf[o + 5 * k * i:] for i in range(len(_GROUPS))]          # est, noisy, gain
            call("maavss_metric_add_classes", ptr(m[:, f.col0:]), None, b, cols, k, ptr(slot[0]), st)
            if noisy is not None:
                mn = f.metric(self, noisy, ref, others)["raw"]
                if mn.shape != m.shape:
                    raise ValueError("noisy must have the shape of est")
                call("maavss_metric_add_classes", ptr(mn[:, f.col0:]), None, b, cols, k, ptr(slot[1]), st)
                call("maavss_metric_add_classes", ptr(m[:, f.col0:]), ptr(mn[:, f.col0:]), b, cols, k, ptr(slot[2]), st)

    def add_recording(self, enhancer, noisy, clean, frames=None, attn=None, others=None):
        """Enhance `noisy` [L] with `enhancer(noisy, frames= | attn=)` -> (wave, start) and measure the estimate and the noisy input against
        clean[start : start + len(wave)], the span the estimate covers; `others` ([L] or [K, L], with bss_filter) is cut to the same span."""
        self._check_eval()
        if enhancer.model is not self.model:
            raise ValueError("the Enhancer wraps another model than this Validator")
        if not isinstance(clean, torch.Tensor) or clean.dim() != 1 or clean.dtype != torch.float32:
            raise ValueError(f"clean must be a 1-D float32 tensor, got {getattr(clean, 'shape', type(clean))}")
        require_cuda(noisy, clean)
        wave, start = enhancer(noisy, frames=frames, attn=attn)
        n = wave.shape[0]
        if clean.shape[0] < start + n:
            raise ValueError(f"clean has {clean.shape[0]} samples, the estimate covers [{start}, {start + n})")
        if others is not None:
            if not isinstance(others, torch.Tensor) or others.dim() not in (1, 2) or others.shape[-1] < start + n:
                raise ValueError(f"others must be [L] or [K, L] and cover [{start}, {start + n}), got {getattr(others, 'shape', type(others))}")
            others = others[..., start:start + n][None]
        self.add_waves(wave, clean[start:start + n], noisy=noisy[start:start + n], others=others)

    def result(self):
        """The one device-to-host copy (it waits for the stream) -> dict:
        val_loss_stft, val_loss_attn (total squared error over total elements: a ragged last batch is weighted by its size), val_loss =
        stft + loss_coeff * attn, lsd_db (mean over windows), n_windows; per wave metric m in snr_db, si_sdr_db, seg_snr_db: m (the mean
        over the clips whose value is finite) and m_n_finite / _n_posinf / _n_neginf / _n_nan; with noisy inputs also noisy_m (and its
        counts) and m_improvement = the mean over clips of estimate minus noisy; n_clips.  A quantity nothing was added to is NaN.
        With intelligibility_sr also stoi, estoi, noisy_stoi, noisy_estoi, stoi_improvement, estoi_improvement (always all six) and
        their _n_finite / _n_nan counts: a clip without a 384 ms segment, or with a non-finite sample, counts as NaN.
        With bss_filter also sdr_db, sir_db, sar_db, their noisy_ and _improvement forms (always all nine) and the four counts of each:
        a clip with a status (a non-finite sample, a silent target, a pivot that is not positive) counts as NaN, one without another
        live source has sir_db = +inf.
        With audio_loss also val_loss_spectral_mag and val_loss_spectral_cplx (each sum over the total elements), val_loss_spectral =
        (1 - mix) mag + mix cplx and val_objective = val_loss_spectral + loss_coeff * val_loss_attn: what TrainStep(audio_loss=...)
        minimises, on the held-out data."""
        nan = float("nan")
        if self._buf is None:
            h = [0.0] * self._buf_len()
        else:
            h = self._buf.cpu().tolist()

        def ratio(s, n):
            return s / n if n > 0 else nan

        out = {"val_loss_stft": ratio(h[0], h[1]), "lsd_db": ratio(h[2], h[3]), "val_loss_attn": ratio(h[4], h[5]), "n_windows": int(h[3])}
        out["val_loss"] = out["val_loss_stft"] + self.loss_coeff * out["val_loss_attn"]
        for f, o in self._layout()[0]:
            for group in _GROUPS:
                for name in f.names:
                    s, nf, npos, nneg, nnan = h[o:o + 5]
                    o += 5
                    if f.clips:
                        total = int(nf + npos + nneg + nnan)
                        if group == "est":
                            out["n_clips"] = total
                        elif total == 0:
                            continue
                    key = {"est": name, "noisy": "noisy_" + name, "gain": name + "_improvement"}[group]
                    out[key] = ratio(s, nf)
                    out.update({f"{key}_{c}": int(n) for c, n in zip(_COUNTS, (nf, npos, nneg, nnan)) if c in f.counts})
        if self.audio_loss is not None:
            s_mag, s_cplx, n = h[-_SPEC_LEN:]
            out["val_loss_spectral_mag"], out["val_loss_spectral_cplx"] = ratio(s_mag, n), ratio(s_cplx, n)
            out["val_loss_spectral"] = ratio((1.0 - self.audio_loss.mix) * s_mag + self.audio_loss.mix * s_cplx, n)
            out["val_objective"] = out["val_loss_spectral"] + self.loss_coeff * out["val_loss_attn"]
        return out

    def improved(self, result, key="val_loss"):
        """True when result[key] is lower than every one seen before (and keeps it in `.best`): the reference's "save on
        improvement" (train_av_net.py:174-181); key="val_objective" follows the loss a TrainStep(audio_loss=...) trains on.  A NaN
        loss never improves."""
        loss = float(result[key])
        if loss == loss and (self.best is None or loss < self.best):
            self.best = loss
            return True
        return False
