"""numpy float64 twin of csrc/wave_loss.hip (maavss_amd.WaveformLoss): the definition of include/maavss.h in closed form and in its order,
the cases tests/test_wave_loss_cpu.py and tests/test_wave_loss_gpu.py share, and the bounds they assert.

Definition.  N = fft_len, h = hop, L = h (T - 1), c = (normalized ? sqrt N : 1) / N, w = the synthesis window (the f32 values the kernel reads).
  1 waves     x = istft(pred), s = istft(tgt): per frame the inverse real DFT of the one-sided bins (imaginary parts of DC and Nyquist
              dropped, a trimmed Nyquist bin read as zero) times c N w, overlap-added, divided by den[p] = sum_t w[p - t h]^2, the N/2 samples
              of centre padding cut off
  2 sums      Sxx = sum x^2, Sss = sum s^2, Sxs = sum x s (math.fsum: the correctly rounded sum of the float64 terms)
  3 loss      snr: D = sum (x - s)^2, l = 10 log10(D + eps) - 10 log10(Sss + eps), E = D
              si_sdr: alpha = Sxs / (Sss + eps), E = sum (x - alpha s)^2 summed directly, l = 10 log10(E + eps) - 10 log10(alpha^2 Sss + eps)
              a non-finite sample makes the row NaN
  4 gradient  g = a x + b s (coefficients below), u = g / den, q_t[j] = c w[j] u[t h + j] on the zero-padded (not reflected) signal,
              d/dRe X_t[k] = m_k sum_j q_t[j] cos(2 pi j k / N), d/dIm X_t[k] = -m_k sum_j q_t[j] sin(2 pi j k / N), m_k = 2 inside, 1 at DC and
              Nyquist whose imaginary gradients are 0
The coefficients.  With k = 10 / ln 10: snr has dl/dx = 2 k (x - s) / (D + eps).  si_sdr: dE/dx = 2 (x - alpha s) + dE/dalpha dalpha/dx with
dE/dalpha = -2 sum s (x - alpha s) = -2 (Sxs - alpha Sss) = -2 alpha eps (because alpha (Sss + eps) = Sxs) and dalpha/dx = s / (Sss + eps); the
target power P = alpha^2 Sss has dP/dx = 2 alpha Sss s / (Sss + eps).  Hence a = 2 k / (E + eps) and
b = -2 k alpha ((1 + eps / (Sss + eps)) / (E + eps) + Sss / ((Sss + eps) (alpha^2 Sss + eps))).  At x = 0 alpha = 0 and b = 0: the gradient is zero.

Bounds of the GPU test (u = 2^-53, n = L), on the twin evaluated on the DEVICE's own f32 waves:
  Sxx, Sss, D, Sxs   the same sums by the same kernels as maavss_wave_metrics: quality_twin's (n - 1) u S and (n - 1) u sum |x s|.
  E (si_sdr)         quality_twin's Srr bound (n - 1) u E + 4 u sqrt(Sxx E) was derived for alpha = Sxy / Sxx, where the first-order term
                     -2 alpha d sum r_i ref_i of an alpha that is off by the relative d vanishes, sum r_i ref_i being zero at that alpha.
                     With eps in the denominator sum (x - alpha s) s = Sxs - alpha Sss = alpha eps is NOT zero, so that term stays:
                     2 alpha^2 eps d, with d <= (n - 1) u (sum |x s| / |Sxs| + 1) + 4 u (the two sums' bounds and the division).  Every other
                     step of the argument is unchanged (same sums, same kernel for the second pass).  It matters only where E is of the
                     size of eps^2 / Sss, i.e. for pred == tgt.
  l                  DB_TOL = 1e-4 dB where the twin's l, or -l (the quality the same argument was made for), lies in DB_RANGE.  The
                     argument of quality_twin carries over because eps only ADDS a positive constant to both arguments of the
                     logarithms: a relative error e of E or alpha^2 Sss is a relative error <= e of E + eps or alpha^2 Sss + eps.
  gradient           per row ||G - G_twin||_2 <= K_WGRAD 2^-24 (1 + sqrt(Sxx / (E + eps))) ||G_twin||_2 against the float64 END-TO-END twin
                     (on pred and tgt, not on the device's waves): f32 waves and an f32 transform carry a few 2^-24 relative, and forming
                     x - alpha s or x - s loses the factor sqrt(Sxx / E).
"""
import math

import numpy as np

import quality_twin as qt

U24 = 2.0 ** -24
U53 = qt.U53
K10 = 10.0 / math.log(10.0)

# (B, T, N, hop, trimmed, normalized): two frames, one pair; B T odd -- a pair straddles two rows, a lone last frame; the stitched avse_S
# shape with three windows; 16-fold overlap with every sample in the envelope's edge region; an odd hop close to N with the Nyquist bin
# trimmed; the two-buffer 1024-point transform; no overlap, unnormalised; more frame pairs than lanes and a row of five reduction chunks
SHAPES = ((1, 2, 256, 66, False, True), (3, 5, 256, 66, False, True), (2, 24, 256, 66, False, True), (2, 3, 512, 33, False, True),
          (2, 3, 256, 255, True, True), (1, 4, 1024, 130, True, True), (2, 3, 512, 512, False, False), (1, 300, 256, 66, False, True))
KINDS = ("si_sdr", "snr")
INPUTS = ("k0.3", "k0.003", "k3", "equal", "zero_pred", "zero_tgt", "nan", "inf")
FINITE_INPUTS = INPUTS[:6]
NOISY_INPUTS = INPUTS[:3]
EPS = 1e-8

# K_WGRAD: the largest ratio ||G - G_twin|| / (2^-24 (1 + sqrt(Sxx / (E + eps))) ||G_twin||) over the rows of all finite cases, measured on
# an MI355X by scripts/wave_loss_parity.py (profiles/wave_loss_parity.json); the gate is eight times that rounded up to a power of ten.
# K_CAP is a condition, not a measurement: beyond it the arithmetic is not f32-accurate.
# Measured: 2.64 (snr at k = 0.003, [2, 3, 512, 33]); every noisy case lay between 1.1 and 2.7, the silent ones at 0 or between 1.1 and
# 2.7, `equal` below 3e-3, the twin's zeros were zeros.  8 x 2.64 = 21.1 -> 100.
K_CAP = 1e3
K_WGRAD_MEASURED = 2.64
K_WGRAD = 1e2


def window(n_fft):
    """STFT.raw_window: the periodic Hamming window, rounded to f32 as the kernels read it."""
    k = np.arange(n_fft, dtype=np.float64)
    return (0.54 - 0.46 * np.cos(2.0 * math.pi * k / n_fft)).astype(np.float32).astype(np.float64)


def n_bins(n_fft, trimmed):
    return n_fft // 2 + (0 if trimmed else 1)


def make_case(shape, inp, seed=0):
    """-> (pred, tgt) f32 [B, 2, T, F]."""
    b, t, n, hop, trimmed, _ = shape
    f = n_bins(n, trimmed)
    rng = np.random.default_rng([seed, b, t, n, hop])
    tgt = (0.3 * rng.standard_normal((b, 2, t, f))).astype(np.float32)
    noise = 0.3 * rng.standard_normal((b, 2, t, f))
    k = {"k0.3": 0.3, "k0.003": 0.003, "k3": 3.0}.get(inp, 0.3)
    pred = (tgt + k * noise).astype(np.float32)
    if inp == "equal":
        pred = tgt.copy()
    elif inp == "zero_pred":
        pred = np.zeros_like(tgt)
    elif inp == "zero_tgt":
        tgt = np.zeros_like(tgt)
    elif inp == "nan":
        pred[b - 1, 1, t // 2, f // 3] = np.nan
    elif inp == "inf":
        tgt[0, 0, t - 1, f // 2] = np.inf
    return pred, tgt


def envelope(n_fft, hop, t):
    """den[p], p < h (T - 1) + N: the window-square sum over the frames covering p."""
    w = window(n_fft)
    den = np.zeros(hop * (t - 1) + n_fft)
    for i in range(t):
        den[i * hop:i * hop + n_fft] += w * w
    return den


def istft(spec, n_fft, hop, normalized):
    """spec [B, 2, T, F] (any float) -> float64 [B, h (T - 1)]."""
    spec = np.asarray(spec, dtype=np.float64)
    b, _, t, f = spec.shape
    z = np.zeros((b, t, n_fft // 2 + 1), dtype=np.complex128)
    with np.errstate(all="ignore"):
        z[:, :, :f] = spec[:, 0] + 1j * spec[:, 1]
        z.imag[:, :, 0] = 0.0
        z.imag[:, :, n_fft // 2] = 0.0
        scale = math.sqrt(n_fft) if normalized else 1.0
        frames = np.fft.irfft(z, n=n_fft, axis=2) * scale * window(n_fft)
        out = np.zeros((b, hop * (t - 1) + n_fft))
        for i in range(t):
            out[:, i * hop:i * hop + n_fft] += frames[:, i]
        out /= envelope(n_fft, hop, t)
    length = hop * (t - 1)
    return out[:, n_fft // 2:n_fft // 2 + length]


def wave_rows(x, s, kind, eps=EPS):
    """x, s [B, L] (f32 or f64) -> dict of per-row float64 arrays: rows [B, 5] = (l, Sxx, Sss, Sxs, E), sabs = sum |x s|, alpha, a, b."""
    x, s = np.asarray(x, dtype=np.float64), np.asarray(s, dtype=np.float64)
    nb = x.shape[0]
    rows, sabs, alpha, ca, cb = (np.full(sh, np.nan) for sh in ((nb, 5), nb, nb, nb, nb))
    for i in range(nb):
        xi, si = x[i], s[i]
        if not (np.isfinite(xi).all() and np.isfinite(si).all()):
            continue
        sxx, sss, sxs, sabs[i] = qt._fsum(xi * xi), qt._fsum(si * si), qt._fsum(xi * si), qt._fsum(np.abs(xi * si))
        if kind == "snr":
            d = xi - si
            e = qt._fsum(d * d)
            al, a = 1.0, 2.0 * K10 / (e + eps)
            l, b = 10.0 * math.log10(e + eps) - 10.0 * math.log10(sss + eps), -a
        else:
            assert kind == "si_sdr"
            al = sxs / (sss + eps)
            r = xi - al * si
            e = qt._fsum(r * r)
            d1, ps, d2 = e + eps, sss + eps, al * al * sss + eps
            l = 10.0 * math.log10(d1) - 10.0 * math.log10(d2)
            a = 2.0 * K10 / d1
            b = -2.0 * K10 * al * ((1.0 + eps / ps) / d1 + sss / (ps * d2))
        rows[i], alpha[i], ca[i], cb[i] = (l, sxx, sss, sxs, e), al, a, b
    return dict(rows=rows, sabs=sabs, alpha=alpha, a=ca, b=cb)


def adjoint(g, n_fft, hop, t, f, normalized, grad_scale):
    """g [B, L] = d/dx -> [B, 2, T, F] = grad_scale times d/d(re, im) of the STFT planes."""
    g = np.asarray(g, dtype=np.float64)
    b, length = g.shape
    assert length == hop * (t - 1)
    c = (math.sqrt(n_fft) if normalized else 1.0) / n_fft
    with np.errstate(all="ignore"):
        u = np.zeros((b, length + n_fft))
        u[:, n_fft // 2:n_fft // 2 + length] = g
        u /= envelope(n_fft, hop, t)
        cw = c * window(n_fft)
        q = np.stack([u[:, i * hop:i * hop + n_fft] * cw for i in range(t)], axis=1)      # [B, T, N]
        z = np.fft.rfft(q, axis=2)                                                          # sum q (cos - i sin)
        m = np.full(n_fft // 2 + 1, 2.0)
        m[0] = m[n_fft // 2] = 1.0
        re, im = m * z.real, m * z.imag
        im[:, :, 0] = 0.0
        im[:, :, n_fft // 2] = 0.0
        out = grad_scale * np.stack([re[:, :, :f], im[:, :, :f]], axis=1)
    bad = ~np.isfinite(g).all(axis=1)
    out[bad] = np.nan                      # a non-finite row: the whole gradient of that row is NaN
    return out


def loss_and_grad(pred, tgt, shape, kind, eps=EPS, grad_scale=1.0, waves=None):
    """The float64 end-to-end twin.  `waves` = (x, s) replaces the twin's own inverse STFT (the device's f32 waves, read back)."""
    _, t, n, hop, trimmed, normalized = shape
    f = n_bins(n, trimmed)
    x, s = waves if waves is not None else (istft(pred, n, hop, normalized), istft(tgt, n, hop, normalized))
    r = wave_rows(x, s, kind, eps)
    with np.errstate(all="ignore"):
        g = r["a"][:, None] * np.asarray(x, dtype=np.float64) + r["b"][:, None] * np.asarray(s, dtype=np.float64)
    r["grad"] = adjoint(g, n, hop, t, f, normalized, grad_scale)
    r["loss"] = float(np.mean(r["rows"][:, 0]))
    r["x"], r["s"] = x, s
    return r


def check_rows(got, want, n, kind, eps=EPS, label=""):
    """got [B, 5] from the device, want = wave_rows on the device's waves: the bounds of the module docstring.  Prints the figures."""
    for i in range(got.shape[0]):
        l, sxx, sss, sxs, e = (float(v) for v in got[i])
        wl, wxx, wss, wxs, we = (float(v) for v in want["rows"][i])
        if wl != wl:
            assert all(v != v for v in (l, sxx, sss, sxs, e)), (label, i, got[i])
            continue
        al, sabs = float(want["alpha"][i]), float(want["sabs"][i])
        e_bound = (n - 1) * U53 * we
        if kind == "si_sdr":
            d = (n - 1) * U53 * ((sabs / abs(wxs) if wxs != 0.0 else 0.0) + 1.0) + 4 * U53
            e_bound += 4 * U53 * math.sqrt(wxx * we) + 2.0 * al * al * eps * d
        for name, g, w, bound in (("Sxx", sxx, wxx, (n - 1) * U53 * wxx), ("Sss", sss, wss, (n - 1) * U53 * wss),
                                  ("Sxs", sxs, wxs, (n - 1) * U53 * sabs), ("E", e, we, e_bound)):
            err = abs(g - w)
            print(f"{label} row {i} {name} {g:.17g} |err| {err:.3g} bound {bound:.3g}")
            assert err <= bound, (label, i, name, g, w, err, bound)
        print(f"{label} row {i} l {l!r} twin {wl!r}")
        assert math.isfinite(l), (label, i, l)
        if qt.DB_RANGE[0] <= wl <= qt.DB_RANGE[1] or qt.DB_RANGE[0] <= -wl <= qt.DB_RANGE[1]:
            assert abs(l - wl) <= qt.DB_TOL, (label, i, l, wl)


def grad_ratios(got, r, eps=EPS):
    """Per row ||G - G_twin|| / (2^-24 (1 + sqrt(Sxx / (E + eps))) ||G_twin||); 0 where both are all zeros, inf where only the twin is."""
    out = []
    for i in range(got.shape[0]):
        want = r["grad"][i]
        if not np.isfinite(want).all():
            continue
        _, sxx, _, _, e = r["rows"][i]
        err = float(np.sqrt(np.sum((got[i].astype(np.float64) - want) ** 2)))
        ref = float(np.sqrt(np.sum(want ** 2)))
        if ref == 0.0:
            out.append(0.0 if err == 0.0 else math.inf)
        else:
            out.append(err / (U24 * (1.0 + math.sqrt(sxx / (e + eps))) * ref))
    return out


def round_up_to_power_of_ten(x):
    return 10.0 ** math.ceil(math.log10(x))
