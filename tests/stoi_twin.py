"""numpy float64 twin of csrc/stoi.hip (maavss_amd.stoi_metrics): short-time objective intelligibility (STOI, Taal et al. 2011) and its
extended form (ESTOI, Jensen & Taal 2016) of one row of `est` against `ref`, both f32 at 10 kHz.  The twin states the definition of
include/maavss.h literally and is the contract the kernels are held to; tests/test_stoi_cpu.py and tests/test_stoi_gpu.py share its cases.

Two deviations from the widely used Python implementation, both stated in the header: the silent-frame mask compares squared norms
without an epsilon inside a logarithm, and a row without a complete 30-frame segment scores NaN (and is counted) instead of 1e-5."""
import math

import numpy as np

FS = 10000
FRAME = 256
HOP = 128
NFFT = 512
J = 15
FIRST_CF = 150.0
N = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = 2.0 ** -52
NAN = float("nan")

W = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, FRAME + 1) / (FRAME + 1))          # numpy.hanning(258)[1:-1]
CLIP = 1.0 + 10.0 ** (-BETA / 20.0)


def nframes(length):
    """The framing convention of the Python implementation: one frame fewer than fit when length - 256 is a multiple of 128."""
    return len(range(0, int(length) - FRAME, HOP))


def band_edges(shift=0):
    """-> (lo, hi): band j sums the bins [lo[j], hi[j]) of the 257 of a 512-point transform at 10 kHz.  `shift` moves every edge by
    that many bins (the sensitivity check of tests/test_stoi_cpu.py)."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    cf = FIRST_CF * 2.0 ** (np.arange(J) / 3.0)
    lo = [int(np.argmin((f - c * 2.0 ** (-1.0 / 6.0)) ** 2)) + shift for c in cf]
    hi = [int(np.argmin((f - c * 2.0 ** (1.0 / 6.0)) ** 2)) + shift for c in cf]
    return lo, hi


LO, HI = band_edges()


def frame_energies(ref):
    """E[k] = sum_n (w[n] ref[128 k + n])^2 in float64."""
    x = np.asarray(ref, dtype=np.float64)
    return np.array([float((((W * x[HOP * k:HOP * k + FRAME]) ** 2)).sum()) for k in range(nframes(x.size))], dtype=np.float64)


def margin_db(ref):
    """The smallest |10 log10(E[k] 1e4 / Emax)| over the frames: how far the closest frame is from the 40 dB decision."""
    e = frame_energies(ref)
    if e.size == 0 or e.max() == 0.0:
        return math.inf
    with np.errstate(divide="ignore"):
        return float(np.abs(10.0 * np.log10(e * 1e4 / e.max())).min())


def _compact(x, kept):
    """overlap-add at hop 128 of the kept windowed frames"""
    out = np.zeros(HOP * (len(kept) - 1) + FRAME, dtype=np.float64)
    for j, k in enumerate(kept):
        out[HOP * j:HOP * j + FRAME] += W * x[HOP * k:HOP * k + FRAME]
    return out


def _bands(x, lo, hi):
    """compacted signal -> [J, M] band magnitudes"""
    m = nframes(x.size)
    out = np.zeros((J, m), dtype=np.float64)
    for k in range(m):
        spec = np.fft.rfft(W * x[HOP * k:HOP * k + FRAME], NFFT)
        p = spec.real ** 2 + spec.imag ** 2
        for j in range(J):
            out[j, k] = math.sqrt(float(p[lo[j]:hi[j]].sum()))
    return out


def _norm(v, axis):
    return np.sqrt((v * v).sum(axis=axis, keepdims=True))


def _row_col_normalise(s):
    s = s - s.mean(axis=1, keepdims=True)
    s = s / (_norm(s, 1) + EPS)
    s = s - s.mean(axis=0, keepdims=True)
    return s / (_norm(s, 0) + EPS)


def stoi_row(est, ref, band_shift=0):
    """-> dict(stoi, estoi, n_kept, n_segments) of one row."""
    est, ref = np.asarray(est), np.asarray(ref)
    assert est.dtype == np.float32 and ref.dtype == np.float32 and est.shape == ref.shape and est.ndim == 1
    none = dict(stoi=NAN, estoi=NAN, n_kept=0, n_segments=0)
    if not (np.isfinite(est).all() and np.isfinite(ref).all()):
        return none
    y, x = est.astype(np.float64), ref.astype(np.float64)
    e = frame_energies(ref)
    if e.size == 0:
        return none
    kept = [k for k in range(e.size) if e[k] * 1e4 > e.max()]
    res = dict(none, n_kept=len(kept))
    m = len(kept) - 1
    if m < N:
        return res
    lo, hi = band_edges(band_shift)
    xb, yb = _bands(_compact(x, kept), lo, hi), _bands(_compact(y, kept), lo, hi)
    assert xb.shape == (J, m)
    d_sum, e_sum = 0.0, 0.0
    for end in range(N, m + 1):
        xs, ys = xb[:, end - N:end], yb[:, end - N:end]
        alpha = _norm(xs, 1) / (_norm(ys, 1) + EPS)
        yc = np.minimum(alpha * ys, xs * CLIP)
        xn = xs - xs.mean(axis=1, keepdims=True)
        yn = yc - yc.mean(axis=1, keepdims=True)
        xn = xn / (_norm(xn, 1) + EPS)
        yn = yn / (_norm(yn, 1) + EPS)
        d_sum += float((xn * yn).sum())
        e_sum += float((_row_col_normalise(xs) * _row_col_normalise(ys)).sum()) / N
    nseg = m - N + 1
    res.update(stoi=d_sum / (J * nseg), estoi=e_sum / nseg, n_segments=nseg)
    return res


def make_case(seed, length, snr_db=5.0, silent=()):
    """-> (est, ref) f32 [length]: ref is five tones between 300 Hz and 3.4 kHz, each under its own slow (2 to 7 Hz) envelope, on a
    noise floor 40 dB under them, with the spans `silent` [(start, stop)] scaled by 1e-4 (80 dB down: far under the 40 dB rule); est is
    ref plus white noise at `snr_db` (None or inf: est == ref)."""
    rng = np.random.default_rng(seed)
    t = np.arange(length) / FS
    ref = np.zeros(length)
    for f0, fm in ((310.0, 2.1), (620.0, 3.3), (1170.0, 4.7), (2230.0, 5.9), (3410.0, 6.8)):
        ph, pm = rng.uniform(0, 2 * np.pi, 2)
        ref += (0.55 + 0.45 * np.sin(2 * np.pi * fm * t + pm)) * np.sin(2 * np.pi * f0 * t + ph)
    ref = 0.1 * ref + 1e-3 * rng.standard_normal(length)
    for a, b in silent:
        ref[a:b] *= 1e-4
    ref = ref.astype(np.float32)
    if snr_db is None or snr_db == math.inf:
        return ref.copy(), ref
    noise = rng.standard_normal(length)
    gain = math.sqrt(float((ref.astype(np.float64) ** 2).mean()) / float((noise ** 2).mean()) / 10.0 ** (snr_db / 10.0))
    return (ref + gain * noise).astype(np.float32), ref


# The GPU cases at 10 kHz: (name, length, silent spans).  Frame counts 0, 0, 1, 30 (no segment), 31, 31 (one segment), 32 (two), 40 (the
# project's clip), 233; silence at the start, at the end, in the middle, and enough of it to leave fewer than 30 frames.
GPU_CASES = [
    ("L255", 255, ()), ("L256", 256, ()), ("L257", 257, ()), ("L4096", 4096, ()), ("L4097", 4097, ()), ("L4224", 4224, ()),
    ("L4225", 4225, ()), ("L5280", 5280, ()), ("L30000", 30000, ()),
    ("silent_start", 6000, ((0, 700),)), ("silent_end", 6000, ((5200, 6000),)), ("silent_middle", 6000, ((2000, 2600),)),
    ("silent_too_much", 4500, ((1000, 1800),)), ("L6000", 6000, ()),
]
BATCH = ("silent_start", "L6000", "silent_middle")          # three rows of one call that keep 41, 45 and 42 frames
OVERLAP = dict(n=5280, stride=700, rows=3, off_est=1, off_ref=3)


def gpu_case(name, snr_db=5.0):
    k = [c[0] for c in GPU_CASES].index(name)
    _, length, silent = GPU_CASES[k]
    return make_case(1000 + k, length, snr_db, silent)


def overlap_signals():
    """-> (est, ref) f32: one signal each, of which the rows [off + i stride, off + i stride + n) of OVERLAP are taken (rows overlap)."""
    o = OVERLAP
    return make_case(77, max(o["off_est"], o["off_ref"]) + (o["rows"] - 1) * o["stride"] + o["n"] + 5, 5.0, ((2500, 3100),))


def overlap_rows():
    o = OVERLAP
    est, ref = overlap_signals()
    return (np.stack([est[o["off_est"] + i * o["stride"]:][:o["n"]] for i in range(o["rows"])]),
            np.stack([ref[o["off_ref"] + i * o["stride"]:][:o["n"]] for i in range(o["rows"])]))


def bad_rows():
    """-> (est, ref, kinds) [6, 5280]: a NaN in est, an inf in ref, a NaN in the last sample of est (past the last frame), a silent
    reference, and two ordinary rows around them."""
    kinds = ("fine", "nan_est", "inf_ref", "silent_ref", "nan_tail", "fine")
    est, ref = [], []
    for i, kind in enumerate(kinds):
        e, r = make_case(300 + i, 5280, 5.0)
        if kind == "nan_est":
            e[1234] = np.nan
        elif kind == "inf_ref":
            r[4000] = np.inf
        elif kind == "silent_ref":
            r[:] = 0.0
        elif kind == "nan_tail":
            e[-1] = np.nan
        est.append(e)
        ref.append(r)
    return np.stack(est), np.stack(ref), kinds


def validator_batches():
    """-> two batches (est, ref, noisy) of 5280-sample clips, 3 and 2 rows: the estimate 10 dB over its noise, the noisy input 0 dB; the
    second batch's row 1 has a NaN in the estimate only."""
    out = []
    for b, rows in enumerate((3, 2)):
        est, ref, noisy = [], [], []
        for i in range(rows):
            e, r = make_case(500 + 10 * b + i, 5280, 10.0)
            q, r2 = make_case(500 + 10 * b + i, 5280, 0.0)
            assert np.array_equal(r, r2)
            est.append(e)
            ref.append(r)
            noisy.append(q)
        out.append([np.stack(est), np.stack(ref), np.stack(noisy)])
    out[1][0][1, 2000] = np.nan
    return out


def all_gpu_refs():
    """name -> ref rows [B, L] of every case the GPU test compares at 10 kHz (the mask decision depends on ref alone)."""
    refs = {name: gpu_case(name)[1][None] for name, _, _ in GPU_CASES}
    refs["overlap"] = overlap_rows()[1]
    refs["bad"] = bad_rows()[1]
    for b, (_, ref, _) in enumerate(validator_batches()):
        refs[f"validator{b}"] = ref
    return refs
