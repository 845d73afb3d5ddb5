"""The clip-level waveform loss: SI-SDR or SNR of the inverse STFT of the model's output, as a training objective.

The per-bin losses (the reference's MSE, SpectralLoss) fit one training window of `hops_per_frame` frames.  A waveform objective needs
a clip: the `num_seq` windows of TrainStep.sliding_window_step predict consecutive groups of frames, and joined they are one gap-free
STFT whose inverse is a waveform.  include/maavss.h states the definition next to maavss_wave_loss; csrc/wave_loss.hip evaluates it
(the waves by maavss_istft's own kernels, the sums by the wave metrics' f64 chunk passes, the gradient by the adjoint of the inverse
STFT); tests/wave_loss_twin.py is its float64 restatement.

    stft = maavss_amd.STFT(256, 66)
    loss = maavss_amd.WaveformLoss(stft, kind="si_sdr")
    step = maavss_amd.TrainStep(model, num_seq=4, wave_loss=loss, wave_weight=0.1)      # sliding_window_step adds the clip term

The loss is in dB with the sign of a loss: -SI-SDR, lower is better.  Nothing here synchronises with the host.
"""
import math

import torch

from ._lib import call, ptr, query, require_cuda, stream_ptr, workspace
from .stft import STFT

KINDS = ("si_sdr", "snr")


class WaveformLoss:
    """l_b = 10 log10(E_b + eps) - 10 log10(P_b + eps) per row of pred, tgt f32 [B, 2, T, F] with x = stft.inverse(pred),
    s = stft.inverse(tgt): kind "snr" has E = sum (x - s)^2, P = sum s^2; kind "si_sdr" has alpha = sum x s / (sum s^2 + eps),
    E = sum (x - alpha s)^2, P = alpha^2 sum s^2.  `stft` is the maavss_amd.STFT the data was made with; only fft_len, hop, normalized,
    trim_stft_end and raw_window (the synthesis window of its inverse) are read."""

    def __init__(self, stft, kind="si_sdr", eps=1e-8):
        if not isinstance(stft, STFT):
            raise ValueError(f"stft must be a maavss_amd.STFT, got {stft!r}")
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not math.isfinite(eps) or not eps > 0.0:
            raise ValueError(f"eps must be a finite number > 0 (an energy added to the sums), got {eps!r}")
        self.stft, self.kind, self.eps = stft, kind, float(eps)

    def __repr__(self):
        return f"WaveformLoss(fft_len={self.stft.fft_len}, hop={self.stft.hop}, kind={self.kind!r}, eps={self.eps!r})"

    def check_operands(self, pred, tgt):
        for t, what in ((pred, "pred"), (tgt, "tgt")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 2 or t.numel() == 0:
                raise ValueError(f"{what} must be a non-empty float32 tensor [B, 2, T, F], got {tuple(getattr(t, 'shape', ()))} "
                                 f"{getattr(t, 'dtype', type(t))}")
        if pred.shape != tgt.shape:
            raise ValueError(f"pred {tuple(pred.shape)} and tgt {tuple(tgt.shape)} differ in shape")
        if pred.shape[3] != self.stft.n_bins():
            raise ValueError(f"F = {pred.shape[3]} bins, the STFT has n_bins() = {self.stft.n_bins()}")
        if pred.shape[2] < 2:
            raise ValueError(f"T = {pred.shape[2]}: the inverse STFT needs at least two frames")
        if not 0 < self.stft.hop <= self.stft.fft_len:
            raise ValueError(f"hop {self.stft.hop} must be in 1..fft_len = {self.stft.fft_len}")
        require_cuda(pred, tgt)

    def __call__(self, pred, tgt, grad_scale=None, into=None):
        """-> {"rows": f64 [B, 5] = (l_b, Sxx, Sss, Sxs, E_b), "loss": f64 scalar = the mean of l_b, "grad": f32 of pred's shape =
        grad_scale times the gradient of the SUM of l_b, or None, "waves": f32 [2, B, hop (T - 1)] = x and s as the op used them (a view
        of its workspace)}.  grad_scale=None is the forward-only form (no gradient is written); grad_scale = 1 / B gives the gradient of
        "loss".  `into`: f32 contiguous [K, B, 2, T / K, F] -- the gradient is ADDED there, frames [T / K * j, T / K * (j + 1)) to
        into[j], instead of returned ("grad" is None): TrainStep adds the clip's gradient to its windows' this way, by the kernel's own
        epilogue.  Device tensors; only enqueues launches on the current stream."""
        if grad_scale is not None and not math.isfinite(grad_scale):
            raise ValueError(f"grad_scale must be None or finite, got {grad_scale!r}")
        self.check_operands(pred, tgt)
        pred, tgt = pred.contiguous(), tgt.contiguous()
        b, _, t, f = pred.shape
        st = self.stft
        d_frames, d_block = t, 0
        grad = dst = None
        if into is not None:
            if grad_scale is None:
                raise ValueError("into= needs a grad_scale")
            if (not isinstance(into, torch.Tensor) or into.dtype != torch.float32 or into.dim() != 5 or not into.is_contiguous()
                    or into.shape[1:3] != (b, 2) or into.shape[4] != f or into.shape[0] * into.shape[3] != t):
                raise ValueError(f"into must be a contiguous float32 [K, {b}, 2, {t} / K, {f}], got {tuple(getattr(into, 'shape', ()))}")
            require_cuda(into)
            dst, d_frames, d_block = into, into.shape[3], into.stride(0)
        elif grad_scale is not None:
            grad = dst = torch.empty_like(pred)
        rows = torch.empty(b, 5, dtype=torch.float64, device=pred.device)
        nbytes = int(query("maavss_wave_loss_ws_bytes", b, t, st.fft_len, st.hop))
        if nbytes <= 0:
            raise ValueError(f"[{b}, 2, {t}, {f}] at fft_len {st.fft_len}, hop {st.hop} is more than one call takes")
        ws = workspace(nbytes, pred.device)
        window = st.raw_window if st.raw_window.device == pred.device else st.raw_window.to(pred.device)
        call("maavss_wave_loss", ptr(pred), ptr(tgt), b, t, f, ptr(window), st.fft_len, st.hop, 1 if st.normalized else 0,
             KINDS.index(self.kind), self.eps, 0.0 if grad_scale is None else float(grad_scale), ptr(dst), d_frames, d_block,
             1 if into is not None else 0, ptr(rows), ptr(ws), nbytes, stream_ptr())
        n = st.hop * (t - 1)
        waves = ws.view(torch.float32)[:2 * b * n].view(2, b, n)
        return {"rows": rows, "loss": rows[:, 0].mean(), "grad": grad, "waves": waves}
