"""Intelligibility scores on the device: short-time objective intelligibility (STOI, Taal et al. 2011) and its extended form (ESTOI,
Jensen & Taal 2016), the two figures speech-enhancement work reports next to SI-SDR (csrc/stoi.hip: f64 throughout, fixed order, no
floating-point atomics).  include/maavss.h states the definition next to maavss_stoi; tests/stoi_twin.py is its float64 restatement.
Nothing here waits for the device: `Validator(intelligibility_sr=...)` accumulates the scores, `Validator.result()` copies them."""
import torch

from ._lib import call, column_dict, ptr, query, require_cuda, require_same_shape, stream_ptr, wave_rows, workspace
from .audio_transform import AudioTransform

STOI_SR = 10000                      # the rate the measure is defined at
STOI_COLUMNS = ("stoi", "estoi", "n_kept", "n_segments")
_resample = AudioTransform(STOI_SR)  # holds no device memory until a rate other than 10 kHz is asked for; its tap tables are kept per rate


def stoi_metrics(est, ref, sr=STOI_SR):
    """est, ref: f32 cuda [L] or [B, L] sampled at `sr`, samples contiguous, any row stride >= 0 (rows may overlap) and any 4-byte-aligned
    offset -- a slice is taken as it is.  -> dict of device f64 tensors [B]: stoi, estoi, n_kept (frames left after silent-frame removal)
    and n_segments (384 ms segments scored), and "raw" [B, 4], the one buffer they are columns of.  A row without a segment (shorter than
    31 kept frames, a silent reference) or with a non-finite sample scores NaN with n_segments = 0.  sr != 10000 sends both through
    AudioTransform(10000) first, on the device.  Only enqueues launches on the current stream."""
    est, ref = wave_rows(est, "est"), wave_rows(ref, "ref")
    require_same_shape(est, ref)
    if isinstance(sr, bool) or not isinstance(sr, int) or sr < 1:
        raise ValueError(f"sr must be a positive integer (samples per second), got {sr!r}")
    if sr != STOI_SR:
        _resample.check(est, sr, batched=True)          # refuses a rate pair the resampler cannot serve, before any device work
    require_cuda(est, ref)
    if sr != STOI_SR:
        est, ref = _resample(est, sr, batched=True), _resample(ref, sr, batched=True)
    b, n = est.shape
    nbytes = int(query("maavss_stoi_ws_bytes", b, n))
    if nbytes == 0:
        raise ValueError(f"stoi_metrics: {b} rows of {n} samples are beyond the kernels' index range")
    out = torch.empty(b, len(STOI_COLUMNS), dtype=torch.float64, device=est.device)
    ws = workspace(nbytes, est.device)
    call("maavss_stoi", ptr(est), est.stride(0), ptr(ref), ref.stride(0), b, n, ptr(out), ptr(ws), nbytes, stream_ptr())
    return column_dict(out, STOI_COLUMNS)
