"""BSS-eval on the device: SDR, SIR and SAR (Vincent, Gribonval & Fevotte 2006) of an estimate against a known target and known other
sources, with a time-invariant distortion filter of `filt_len` taps -- what kind of error remains in a mix-and-separate output: leakage
of the other source (SIR) or something the network made up (SAR).  csrc/bss_eval.hip: correlations, one Cholesky factorisation of up to
2048 unknowns per row and two FIR projections, f64 throughout, fixed order, no floating-point atomics.  include/maavss.h states the
definition next to maavss_bss_eval; tests/bss_twin.py is its float64 restatement.
Nothing here waits for the device: `Validator(bss_filter=...)` accumulates the scores, `Validator.result()` copies them."""
import torch

from ._lib import call, column_dict, ptr, query, require_cuda, require_same_shape, stream_ptr, wave_rows, workspace

BSS_COLUMNS = ("s_tt", "s_ee", "s_ii", "s_aa", "s_pp", "sdr_db", "sir_db", "sar_db", "n_sources", "status")
BSS_DB = ("sdr_db", "sir_db", "sar_db")                  # columns 5..7 of a bss_eval_metrics row
BSS_MAX_FILTER = 512
BSS_MAX_OTHERS = 3
BSS_WORKSPACE_CAP = 1 << 30          # bytes: a batch whose workspace would be larger is processed in groups of rows


def _sources(t, b, n):
    """others -> [B, K, n] with contiguous samples and strides >= 0, or None for K = 0"""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() not in (2, 3):
        raise ValueError(f"others must be a float32 tensor [B, L] or [B, K, L], got {tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))}")
    t = t[:, None] if t.dim() == 2 else t
    if t.shape[0] != b or t.shape[2] != n:
        raise ValueError(f"others {tuple(t.shape)} does not go with est [{b}, {n}]")
    if t.shape[1] > BSS_MAX_OTHERS:
        raise ValueError(f"others holds K = {t.shape[1]} sources, at most {BSS_MAX_OTHERS} are served")
    if t.shape[1] == 0:
        return None
    if n > 1 and t.stride(2) != 1 or b > 1 and t.stride(0) < 0 or t.shape[1] > 1 and t.stride(1) < 0:
        t = t.contiguous()
    return t


def bss_eval_metrics(est, ref, others=None, filt_len=BSS_MAX_FILTER):
    """est, ref: f32 cuda [L] or [B, L]; others: None, [B, L] (K = 1) or [B, K, L] with K <= 3: the other sources of each row, an all-zero
    one is left out.  Samples contiguous, any row (and source) stride >= 0 (rows may overlap), any 4-byte-aligned offset: a slice is taken
    as it is.  1 <= filt_len <= 512 and L >= (K + 1) filt_len.  -> dict of device f64 tensors [B]: s_tt, s_ee, s_ii, s_aa, s_pp, sdr_db,
    sir_db, sar_db, n_sources, status (0 ok, 1 a non-finite sample, 2 a silent target, 3 a Cholesky pivot that is not positive: the
    scores of such a row are NaN), and "raw" [B, 10], the one buffer they are columns of.  A batch whose workspace would exceed
    BSS_WORKSPACE_CAP (1 GiB; a row of 1024 unknowns takes 9 MB, of 2048 35 MB) is processed in groups of rows; every row is computed on
    its own, so the grouping does not change a bit.  Only enqueues launches on the current stream."""
    est, ref = wave_rows(est, "est"), wave_rows(ref, "ref")
    require_same_shape(est, ref)
    b, n = est.shape
    if isinstance(filt_len, bool) or not isinstance(filt_len, int) or not 1 <= filt_len <= BSS_MAX_FILTER:
        raise ValueError(f"filt_len must be an integer in 1..{BSS_MAX_FILTER}, got {filt_len!r}")
    oth = _sources(others, b, n)
    k = 0 if oth is None else oth.shape[1]
    if n < (k + 1) * filt_len:
        raise ValueError(f"{n} samples are fewer than the (K + 1) filt_len = {(k + 1) * filt_len} unknowns of the projection")
    require_cuda(est, ref, oth)
    per_row = int(query("maavss_bss_eval_ws_bytes", 1, n, k, filt_len))
    if per_row == 0:
        raise ValueError(f"bss_eval_metrics: rows of {n} samples are beyond the kernels' index range")
    group = max(1, min(b, BSS_WORKSPACE_CAP // per_row, 65535))
    out = torch.empty(b, len(BSS_COLUMNS), dtype=torch.float64, device=est.device)
    nbytes = int(query("maavss_bss_eval_ws_bytes", group, n, k, filt_len))
    ws = workspace(nbytes, est.device)
    st = stream_ptr()
    for g0 in range(0, b, group):
        g1 = min(b, g0 + group)
        o = None if oth is None else oth[g0:g1]
        call("maavss_bss_eval", ptr(est[g0:g1]), est.stride(0), ptr(ref[g0:g1]), ref.stride(0), ptr(o), 0 if o is None else o.stride(0),
             0 if o is None else o.stride(1), k, g1 - g0, n, filt_len, ptr(out[g0:g1]), ptr(ws), nbytes, st)
    return column_dict(out, BSS_COLUMNS)
