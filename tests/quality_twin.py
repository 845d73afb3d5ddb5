"""numpy float64 twin of csrc/quality_metrics.hip (wave metrics, spectrum metrics) and the cases tests/test_quality_metrics_cpu.py and
tests/test_quality_metrics_gpu.py share.  The twin states the definitions literally; its sums are math.fsum, the correctly rounded exact
sum of the float64 terms.

Bounds the tests assert, u = 2^-53, n = the number of terms, and where they come from:
  Sxx, Syy, See, the squared-error sums
          every term is >= 0 and is the same float64 number on both sides: a product of two f32 values is exact in f64 (24 x 24
          significand bits); est - ref is one f64 rounding of two exactly converted f32 values and its square one more, done alike by the
          twin and by the kernel (which is compiled without contraction).  ANY order of f64 additions of n non-negative terms is within
          (n - 1) u S of their exact sum (each addition rounds a partial sum <= S; first order in u, (n u)^2 < 1e-17 for n <= 2^24).
          Gate: (n - 1) u S -- a row of one sample must match exactly.
  Sxy     the same argument with the terms' magnitudes: (n - 1) u sum |ref est|.
  Srr     r_i = est_i - alpha ref_i.  (a) Order of the additions: (n - 1) u Srr.  (b) The kernel's alpha differs from the twin's by its
          relative error d (a quotient of two sums above).  Srr(alpha (1 + d)) - Srr(alpha) = -2 alpha d sum r_i ref_i + (alpha d)^2 Sxx,
          and sum r_i ref_i = Sxy - alpha Sxx vanishes at the exact alpha: what is left is of second order in the summation errors.
          (c) Forming r_i costs up to two roundings, |eps_i| <= u (|alpha ref_i| + |r_i|) (one when the multiply-add is fused), which move
          the sum by at most 2 sum |r_i| |eps_i| <= 2 u (sqrt(alpha^2 Sxx Srr) + Srr) <= 2 u (sqrt(Syy Srr) + Srr), as alpha^2 Sxx <= Syy.
          That holds for the kernel and for the twin: 4 u sqrt(Syy Srr) covers both, fused or not; the 4 u Srr beside it is below (a) from
          five samples on, and below five samples both sides evaluate the same expressions on the same alpha.
          Gate: (n - 1) u Srr + 4 u sqrt(Syy Srr).
  dB      for rows of n <= 2^24 samples whose twin value lies in [-60, +100] dB the gate is 1e-4 dB.  Worst-case chain: each sum is within
          (n - 1) u <= 2^-29 = 1.9e-9 relative; Sxy is within 2^-29 sum |ref est| / |Sxy|, and at -60 dB Sxy^2 = 1e-6 Sxx Syy with
          sum |ref est| <= sqrt(Sxx Syy) (Cauchy-Schwarz), so alpha is within 1e3 * 1.9e-9 = 1.9e-6 and alpha^2 within 3.7e-6; Srr at
          +100 dB (Syy / Srr = 1e10) is within 1.9e-9 + 4 u 1e5 = 1.9e-9.  A relative error e of the ratio moves 10 log10 by
          (10 / ln 10) e = 4.34 e: 4.34 * 3.7e-6 = 1.6e-5 dB for SI-SDR, 4.34 * 3.7e-9 = 1.6e-8 dB for SNR and for every frame of the
          segmental SNR (the clamp is monotone and its mean cannot move by more than its terms); log10 itself adds ~1e-15.  So about
          2e-5 dB at worst, gate 1e-4.
  lsd_db  per bin the kernel takes one logarithm of the quotient of the floored powers, the twin the difference of two levels.  The
          powers re^2 + im^2 are the same f64 numbers on both sides (exact products, one rounding of the sum).  The quotient and its
          log10 round once each: 4.34 * 2 u = 1e-15 dB; the twin's two levels round at u (|level_a| + |level_b|) <= u * 2 * 770 dB for
          any f64 power, 1.7e-13 dB.  With |delta d| <= e_d per bin, sqrt(mean d^2) moves by at most e_d (triangle inequality of the
          2-norm) and so does the mean over frames; sqrt and the two means add a few u relative of a value <= 1e3 dB.  Gate: 1e-9 dB.
  counts, the NaN / +inf / -inf class of every output: exact.
"""
import math

import numpy as np

U53 = 2.0 ** -53
DB_TOL = 1e-4
DB_RANGE = (-60.0, 100.0)
LSD_TOL = 1e-9
SEG_LENS = (7, 256)
KINDS = ("noisy", "zeros_ref", "equal", "nan", "inf", "high_quality")


def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel().tolist())


def _db(q):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10.0 * np.log10(np.float64(q)))


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def klass(v):
    if v != v:
        return "nan"
    if v == math.inf:
        return "posinf"
    if v == -math.inf:
        return "neginf"
    return "finite"


def wave_row(est, ref, seg_len):
    """One row: est, ref f32 [L] -> dict(sxx, syy, sxy, sabs = sum |ref est|, see, srr, alpha, snr_db, si_sdr_db, seg_snr_db, n_frames).
    A non-finite sample: every value NaN, n_frames 0."""
    y, x = np.asarray(est, dtype=np.float32).astype(np.float64), np.asarray(ref, dtype=np.float32).astype(np.float64)
    assert x.shape == y.shape and x.ndim == 1
    nan = float("nan")
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        return dict(sxx=nan, syy=nan, sxy=nan, sabs=nan, see=nan, srr=nan, alpha=nan, snr_db=nan, si_sdr_db=nan, seg_snr_db=nan, n_frames=0)
    e = y - x
    sxx, syy, sxy, sabs, see = _fsum(x * x), _fsum(y * y), _fsum(x * y), _fsum(np.abs(x * y)), _fsum(e * e)
    alpha = _div(sxy, sxx)
    r = y - alpha * x
    srr = _fsum(r * r)
    snr = nan if sxx == 0.0 else _db(_div(sxx, see))
    si = _db(_div(alpha * alpha * sxx, srr))
    vals = []
    for f in range(x.size // seg_len):
        xf, ef = x[f * seg_len:(f + 1) * seg_len], e[f * seg_len:(f + 1) * seg_len]
        sx, se = _fsum(xf * xf), _fsum(ef * ef)
        if sx > 0.0:
            vals.append(min(max(_db(_div(sx, se)), -10.0), 35.0))
    seg = _fsum(vals) / len(vals) if vals else nan
    return dict(sxx=sxx, syy=syy, sxy=sxy, sabs=sabs, see=see, srr=srr, alpha=alpha, snr_db=snr, si_sdr_db=si, seg_snr_db=seg, n_frames=len(vals))


def spectrum_row(pred, tgt, floor=1e-10):
    """One row: pred, tgt f32 [2, T, F] -> dict(sqerr, lsd_db)."""
    p, t = np.asarray(pred, dtype=np.float32).astype(np.float64), np.asarray(tgt, dtype=np.float32).astype(np.float64)
    assert p.shape == t.shape and p.ndim == 3 and p.shape[0] == 2
    d = p - t
    pp, pt = p[0] * p[0] + p[1] * p[1], t[0] * t[0] + t[1] * t[1]
    pp, pt = np.where(pp < floor, floor, pp), np.where(pt < floor, floor, pt)
    with np.errstate(divide="ignore", invalid="ignore"):
        lv = 10.0 * np.log10(pp) - 10.0 * np.log10(pt)
    frames = [math.sqrt(_fsum(row * row) / row.size) for row in lv]
    return dict(sqerr=_fsum(d * d), lsd_db=_fsum(frames) / len(frames))


def wave_lengths(ch, seg_len):
    """The row lengths of the issue for one seg_len: 1, 63, 64, 65, around seg_len, around the chunk length, three chunks and a partial
    frame -- around both CH and the whole-frame chunk length floor(CH / seg_len) * seg_len when they differ."""
    cl = ch // seg_len * seg_len
    ls = {1, 63, 64, 65, seg_len - 1, seg_len, seg_len + 1, ch - 1, ch, ch + 1, cl - 1, cl, cl + 1, 2 * ch + seg_len // 2 + 3}
    return sorted(n for n in ls if n >= 1)


def make_wave(rng, n, kind):
    """-> (est, ref) f32 [n] of one content kind."""
    ref = (0.3 * rng.standard_normal(n)).astype(np.float32)
    est = (ref + 0.1 * rng.standard_normal(n)).astype(np.float32)
    if kind == "zeros_ref":
        ref = np.zeros(n, dtype=np.float32)
    elif kind == "equal":
        est = ref.copy()
    elif kind == "nan":
        est[n // 2] = np.nan
    elif kind == "inf":
        ref[n // 3] = np.inf
    elif kind == "high_quality":          # the estimate 90 dB above its error: Syy - Sxy^2 / Sxx would be all rounding noise
        est = (ref.astype(np.float64) + 0.3 * 10.0 ** (-90.0 / 20.0) * rng.standard_normal(n)).astype(np.float32)
    else:
        assert kind == "noisy"
    return est, ref


def check_wave_row(got, want, n, label=""):
    """got: the nine columns of one row (floats); want: wave_row's dict.  Asserts the bounds of the module docstring; prints the figures."""
    sxx, syy, sxy, see, srr, snr, si, seg, frames = (float(v) for v in got)
    assert int(frames) == want["n_frames"] and frames == int(frames), (label, frames, want["n_frames"])
    if want["sxx"] != want["sxx"]:
        assert all(v != v for v in (sxx, syy, sxy, see, srr, snr, si, seg)), (label, got)
        return
    for name, g, bound in (("sxx", sxx, (n - 1) * U53 * want["sxx"]), ("syy", syy, (n - 1) * U53 * want["syy"]),
                           ("see", see, (n - 1) * U53 * want["see"]), ("sxy", sxy, (n - 1) * U53 * want["sabs"])):
        err = abs(g - want[name])
        print(f"{label} {name} {g:.17g} |err| {err:.3g} bound {bound:.3g}")
        assert err <= bound, (label, name, g, want[name], err, bound)
    if want["srr"] == want["srr"]:
        bound = (n - 1) * U53 * want["srr"] + 4 * U53 * math.sqrt(want["syy"] * want["srr"])
        err = abs(srr - want["srr"])
        print(f"{label} srr {srr:.17g} |err| {err:.3g} bound {bound:.3g}")
        assert err <= bound, (label, "srr", srr, want["srr"], err, bound)
    else:
        assert srr != srr, (label, srr)
    for name, g in (("snr_db", snr), ("si_sdr_db", si), ("seg_snr_db", seg)):
        w = want[name]
        print(f"{label} {name} {g!r} twin {w!r}")
        assert klass(g) == klass(w), (label, name, g, w)
        if klass(w) == "finite" and DB_RANGE[0] <= w <= DB_RANGE[1]:
            assert abs(g - w) <= DB_TOL, (label, name, g, w)
