"""The power-law compressed spectral loss: an audio objective beside the plain MSE of the raw STFT coefficients.

The reference trains on `nn.MSELoss()` of the real and imaginary STFT planes (train_avse_frames.py:166-170); a few loud bins carry that
sum.  This loss compresses first -- magnitudes |X|^c and complex coefficients X |X|^(c - 1) -- as is usual in speech enhancement and
audio-visual separation.  It works per bin on any number of frames and needs no inverse STFT, so it fits a training window of
`hops_per_frame` frames.  include/maavss.h states the definition next to maavss_spectral_loss; csrc/spectral_loss.hip evaluates it in
f64 in a fixed order; tests/spectral_loss_twin.py is its float64 restatement.

    loss = maavss_amd.SpectralLoss(compress=0.3, mix=0.3)
    step = maavss_amd.TrainStep(model, audio_loss=loss)          # losses[0] is this loss, losses[1] the attention MSE as before
    val = maavss_amd.Validator(model, audio_loss=loss)           # result()["val_objective"]

`compress=1, mix=1` is the MSE again.  Nothing here synchronises with the host.
"""
import math

import torch

from ._lib import call, ptr, query, require_cuda, stream_ptr, workspace


class SpectralLoss:
    """a_loss = ((1 - mix) sum (M_p - M_t)^2 + mix sum |p g_p - t g_t|^2) / (2 B T F) with r = re^2 + im^2 + eps, M = r^(compress / 2),
    g = r^((compress - 1) / 2), over pred, tgt f32 [B, 2, T, F] (plane 0 real, plane 1 imaginary)."""

    def __init__(self, compress=0.3, mix=0.3, eps=1e-12):
        for name, v in (("compress", compress), ("mix", mix), ("eps", eps)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
        if not 0.0 < compress <= 1.0:
            raise ValueError(f"compress must be in (0, 1], got {compress!r}")
        if not 0.0 <= mix <= 1.0:
            raise ValueError(f"mix must be in [0, 1], got {mix!r}")
        if not eps > 0.0:
            raise ValueError(f"eps must be > 0 (a power added to re^2 + im^2), got {eps!r}")
        self.compress, self.mix, self.eps = float(compress), float(mix), float(eps)

    def __repr__(self):
        return f"SpectralLoss(compress={self.compress!r}, mix={self.mix!r}, eps={self.eps!r})"

    @staticmethod
    def check_operands(pred, tgt):
        for t, what in ((pred, "pred"), (tgt, "tgt")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 2 or t.numel() == 0:
                raise ValueError(f"{what} must be a non-empty float32 tensor [B, 2, T, F], got {tuple(getattr(t, 'shape', ()))} "
                                 f"{getattr(t, 'dtype', type(t))}")
        if pred.shape != tgt.shape:
            raise ValueError(f"pred {tuple(pred.shape)} and tgt {tuple(tgt.shape)} differ in shape")
        require_cuda(pred, tgt)

    def __call__(self, pred, tgt, grad_scale=None):
        """-> {"rows": f64 [B, 2] = S_mag, S_cplx per row, "loss": f64 scalar = a_loss, "grad": f32 of pred's shape = grad_scale times the
        gradient of the SUM (1 - mix) S_mag + mix S_cplx, or None}.  grad_scale=None is the forward-only form (no gradient is written);
        grad_scale = 1 / pred.numel() gives the gradient of "loss".  Device tensors; only enqueues launches on the current stream."""
        if grad_scale is not None and not math.isfinite(grad_scale):
            raise ValueError(f"grad_scale must be None or finite, got {grad_scale!r}")
        self.check_operands(pred, tgt)
        pred, tgt = pred.contiguous(), tgt.contiguous()
        b, _, t, f = pred.shape
        rows = torch.empty(b, 2, dtype=torch.float64, device=pred.device)
        grad = None if grad_scale is None else torch.empty_like(pred)
        nbytes = int(query("maavss_spectral_loss_ws_bytes", b, t))
        ws = workspace(nbytes, pred.device)
        call("maavss_spectral_loss", ptr(pred), ptr(tgt), b, t, f, self.compress, self.mix, self.eps,
             0.0 if grad_scale is None else float(grad_scale), ptr(grad), ptr(rows), ptr(ws), nbytes, stream_ptr())
        sums = rows.sum(0)
        loss = ((1.0 - self.mix) * sums[0] + self.mix * sums[1]) / float(pred.numel())
        return {"rows": rows, "loss": loss, "grad": grad}
