"""The power-law compressed spectral loss and its gradient in float64: the restatement of include/maavss.h that
csrc/spectral_loss.hip is held to (tests/test_spectral_loss_cpu.py checks this file against torch.autograd, tests/test_spectral_loss_gpu.py
the kernels against this file), with the case list and the bounds of those tests.

Definition.  pred, tgt: f32 [B, 2, T, F], plane 0 real and plane 1 imaginary; compress c in (0, 1], mix lambda in [0, 1], eps > 0 (a
power).  Everything in float64 on the exactly converted inputs, every operation rounded on its own, in the order written in `terms` and
`loss_and_grad` (the kernel's order, so that a signed zero or a NaN comes out where the kernel's does).  Per bin, for pred (p) and tgt (t):

    r  = re^2 + im^2 + eps          M = pow(r, c / 2)          g = pow(r, (c - 1) / 2)      (two pows: c = 1 gives g = 1 exactly)
    e_r = p_r g_p - t_r g_t         e_i = p_i g_p - t_i g_t
    mag term = (M_p - M_t)^2        complex term = e_r^2 + e_i^2
    S_mag[b], S_cplx[b] = sums over the T F bins of row b (here: math.fsum, the correctly rounded sum)
    a_loss = ((1 - lambda) sum_b S_mag[b] + lambda sum_b S_cplx[b]) / (2 B T F)

    s = e_r p_r + e_i p_i      q = (c - 1) g_p / r_p      k = (1 - lambda) (M_p - M_t) c M_p / r_p
    d/dp_r = 2 grad_scale (k p_r + lambda (e_r g_p + q s p_r))      d/dp_i = 2 grad_scale (k p_i + lambda (e_i g_p + q s p_i))

The gradient is that of the SUM (1 - lambda) S_mag + lambda S_cplx times grad_scale; grad_scale = 1 / (2 B T F) makes it a_loss's.
"""
import math

import numpy as np

U24, U53 = 2.0 ** -24, 2.0 ** -53

# (B, T, F): one bin; one frame; B T no multiple of the four frames of a workgroup and odd plane offsets; an even F; a short odd F and five
# rows; F over 512 (nine bins per lane); a row of more frames than a wave has lanes
SHAPES = ((1, 1, 1), (1, 1, 257), (3, 5, 257), (2, 8, 256), (5, 3, 33), (2, 2, 513), (1, 70, 257))
# (compress, mix, eps): the defaults; magnitudes only; the MSE; complex only; plain magnitudes
PARAMS = ((0.3, 0.3, 1e-12), (0.5, 0.0, 1e-8), (1.0, 1.0, 1e-12), (0.3, 1.0, 1e-12), (1.0, 0.0, 1e-12))
KINDS = ("scale_0.3", "scale_1e-5", "zero_pred", "zero_tgt", "zero_both", "equal", "nan", "inf")
FINITE_KINDS = KINDS[:6]

# ---- the bounds of tests/test_spectral_loss_gpu.py ----------------------------------------------------------------------------------
# 1a  |got - twin| <= ulp_f32(max(|got|, |twin|)) / 2 + K_GRAD 2^-53 A per finite gradient element, A = `grad_magnitude`: the one rounding
#     to f32, plus the f64 roundings and the pow errors of either side, each relative to a quantity that A bounds (no cancellation in A).
# 1b  at least IDENTICAL_MIN of the elements carry the bits of the twin rounded once to f32.
# 2   |S_gpu - S_twin| <= (T F - 1) 2^-53 S + K_SUM 2^-53 Bsum per row, Bsum = `row_magnitude`: the kernel adds T F non-negative terms in
#     its own order (fsum here is exact to half an ulp), and each term's error is that of its difference, squared: 2 |d| err(d).
# K_GRAD and K_SUM: scripts/spectral_loss_parity.py measures the largest (|d| - ulp / 2) / (2^-53 A) and (|dS| - (T F - 1) 2^-53 S) /
# (2^-53 Bsum) over every case below on the GPU (profiles/spectral_loss_parity.json); the gate is eight times that, rounded up to a power
# of ten (the project's rule: room for another libm's pow), and may not exceed K_CAP -- beyond it the arithmetic is not f64.
# Measured on an MI355X: no finite gradient element of the 2 299 540 left its half f32 ulp (all bit-identical to the twin rounded once),
# so K_GRAD is the least the script gives, 10: ten f64 roundings of the no-cancellation magnitude.  The largest row-sum excess was 3.09
# (the one-bin shape, where the summation term is zero): 8 x 3.09 = 24.7 -> 100.
K_CAP = 1e4
K_GRAD = 1e1
K_SUM = 1e2
IDENTICAL_MIN = 0.999
# 5   TrainStep(audio_loss=SpectralLoss(1, 1)) against the default TrainStep, relative L2 per gradient tensor: measured by the same
#     script, gated at eight times that rounded up to a power of ten, capped at REL_L2_CAP.  Measured 2.62e-6 (the largest, on visual_encoder.1.bias; d_a itself is within
#     one f32 ulp of mse_pair's): 8 x 2.62e-6 = 2.1e-5 -> 1e-4, which the cap cuts to 1e-5.
REL_L2_CAP = 1e-5
TRAIN_REL_L2 = 1e-5

MSE_BLK = 512      # csrc/mse_term.h: the most workgroups of one maavss_mse_pair term, 4096 elements each below that


def mse_pair_bound(n):
    """Relative bound of maavss_mse_pair's f32 loss against the f64 mean of the exact squares, u = 2^-24: (m + 12) u.  A thread adds m =
    ceil(n / (256 G)) terms in f32, G = min(MSE_BLK, ceil(n / 4096)) workgroups (m u: every addition rounds a partial sum of non-negative
    terms), each term (pred - tgt)^2 with the difference rounded to f32 first (2 u); 6 additions of the wave reduction and 3 across the
    waves (9 u); the f32 store of the loss (u)."""
    g = min(MSE_BLK, -(-n // 4096))
    m = -(-n // (256 * g))
    return (m + 12) * U24


def ulp32(x):
    """The spacing of f32 at |x| (f64 array in, f64 out); the smallest subnormal at 0."""
    with np.errstate(all="ignore"):
        return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def make_case(shape, kind, seed=0):
    """-> pred, tgt f32 [B, 2, T, F].  tgt = scale randn, pred = tgt + 0.3 scale randn (a model part of the way there: M_p - M_t and
    p g_p - t g_t cancel); the kinds zero a tenth of the bins (both planes) in pred, tgt or both, make pred equal tgt, or put one NaN
    into pred / one inf into tgt."""
    assert kind in KINDS
    b, t, f = shape
    rng = np.random.default_rng([seed, b, t, f, KINDS.index(kind)])
    scale = 1e-5 if kind == "scale_1e-5" else 0.3
    tgt = (scale * rng.standard_normal((b, 2, t, f))).astype(np.float32)
    pred = (tgt + 0.3 * scale * rng.standard_normal((b, 2, t, f))).astype(np.float32)
    if kind.startswith("zero"):
        hole = rng.random((b, 1, t, f)) < 0.1
        hole[0, 0, 0, 0] = True                      # the one-bin shape has its hole too
        hole = np.broadcast_to(hole, pred.shape)
        if kind in ("zero_pred", "zero_both"):
            pred[hole] = 0.0
        if kind in ("zero_tgt", "zero_both"):
            tgt[hole] = 0.0
    elif kind == "equal":
        pred = tgt.copy()
    elif kind == "nan":
        pred[b - 1, 0, t // 2, f // 2] = np.nan
    elif kind == "inf":
        tgt[0, 1, t - 1, f - 1] = np.inf
    return pred, tgt


def terms(pred, tgt, c, lam, eps):
    """The per-bin quantities, float64 arrays [B, T, F]."""
    p, t = np.asarray(pred, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    assert p.shape == t.shape and p.ndim == 4 and p.shape[1] == 2
    c, lam, eps = float(c), float(lam), float(eps)
    hc, hg = 0.5 * c, 0.5 * (c - 1.0)
    pr, pi, tr, ti = p[:, 0], p[:, 1], t[:, 0], t[:, 1]
    with np.errstate(all="ignore"):
        rp = pr * pr + pi * pi + eps
        rt = tr * tr + ti * ti + eps
        Mp, Mt = np.power(rp, hc), np.power(rt, hc)
        gp, gt = np.power(rp, hg), np.power(rt, hg)
        er = pr * gp - tr * gt
        ei = pi * gp - ti * gt
        dm = Mp - Mt
        mag = dm * dm
        cplx = er * er + ei * ei
    return dict(pr=pr, pi=pi, tr=tr, ti=ti, rp=rp, rt=rt, Mp=Mp, Mt=Mt, gp=gp, gt=gt, er=er, ei=ei, dm=dm, mag=mag, cplx=cplx)


def row_sums(q):
    """-> rows f64 [B, 2]: S_mag, S_cplx by math.fsum (a non-finite term makes the sum non-finite: NaN, or the infinity)."""
    b = q["mag"].shape[0]
    rows = np.empty((b, 2))
    for i in range(b):
        for k, name in enumerate(("mag", "cplx")):
            v = q[name][i].ravel()
            rows[i, k] = math.fsum(v) if np.isfinite(v).all() else float(np.sum(v))
    return rows


def a_loss(rows, lam, n_elements):
    s_mag, s_cplx = math.fsum(rows[:, 0]), math.fsum(rows[:, 1])
    return ((1.0 - lam) * s_mag + lam * s_cplx) / float(n_elements), s_mag / float(n_elements), s_cplx / float(n_elements)


def gradient(q, c, lam, grad_scale):
    """-> f64 [B, 2, T, F], before the one rounding to f32."""
    c, lam = float(c), float(lam)
    cm1, oml, gs2 = c - 1.0, 1.0 - lam, 2.0 * float(grad_scale)
    with np.errstate(all="ignore"):
        s = q["er"] * q["pr"] + q["ei"] * q["pi"]
        qq = cm1 * q["gp"] / q["rp"]
        k = oml * q["dm"] * c * q["Mp"] / q["rp"]
        d_r = gs2 * (k * q["pr"] + lam * (q["er"] * q["gp"] + qq * s * q["pr"]))
        d_i = gs2 * (k * q["pi"] + lam * (q["ei"] * q["gp"] + qq * s * q["pi"]))
    return np.stack([d_r, d_i], axis=1)


def grad_magnitude(q, c, lam, grad_scale):
    """A, per gradient element: the gradient's expression with every difference replaced by the sum of the absolute values of its two
    sides -- what the result would be without cancellation, the scale its rounding errors are relative to."""
    c, lam = float(c), float(lam)
    cm1, oml, gs2 = abs(c - 1.0), 1.0 - lam, abs(2.0 * float(grad_scale))
    with np.errstate(all="ignore"):
        apr, api = np.abs(q["pr"]), np.abs(q["pi"])
        Er = apr * q["gp"] + np.abs(q["tr"]) * q["gt"]
        Ei = api * q["gp"] + np.abs(q["ti"]) * q["gt"]
        Dm = q["Mp"] + q["Mt"]
        s = Er * apr + Ei * api
        qq = cm1 * q["gp"] / q["rp"]
        k = oml * Dm * c * q["Mp"] / q["rp"]
        a_r = gs2 * (k * apr + lam * (Er * q["gp"] + qq * s * apr))
        a_i = gs2 * (k * api + lam * (Ei * q["gp"] + qq * s * api))
    return np.stack([a_r, a_i], axis=1)


def row_magnitude(q):
    """Bsum f64 [B, 2]: sum |dM| (M_p + M_t) and sum |e| (|p g_p| + |t g_t|) per row."""
    with np.errstate(all="ignore"):
        bm = np.abs(q["dm"]) * (q["Mp"] + q["Mt"])
        bc = (np.abs(q["er"]) * (np.abs(q["pr"]) * q["gp"] + np.abs(q["tr"]) * q["gt"])
              + np.abs(q["ei"]) * (np.abs(q["pi"]) * q["gp"] + np.abs(q["ti"]) * q["gt"]))
    b = bm.shape[0]
    return np.stack([bm.reshape(b, -1).sum(1), bc.reshape(b, -1).sum(1)], axis=1)


def loss_and_grad(pred, tgt, c, lam, eps, grad_scale=None):
    """Everything at once -> dict: rows [B, 2], loss, mag_mean, cplx_mean, grad (f64, None without grad_scale), A, Bsum."""
    q = terms(pred, tgt, c, lam, eps)
    rows = row_sums(q)
    loss, mag_mean, cplx_mean = a_loss(rows, float(lam), np.asarray(pred).size)
    out = dict(rows=rows, loss=loss, mag_mean=mag_mean, cplx_mean=cplx_mean, Bsum=row_magnitude(q), grad=None, A=None)
    if grad_scale is not None:
        out["grad"], out["A"] = gradient(q, c, lam, grad_scale), grad_magnitude(q, c, lam, grad_scale)
    return out


def grad_excess(got, twin, A):
    """(|got - twin| - ulp_f32 / 2) / (2^-53 A) per finite element (what K_GRAD bounds); -inf where the difference is inside the f32
    rounding alone.  got: f32 array; twin, A: f64."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(got - twin) - 0.5 * ulp32(np.maximum(np.abs(got), np.abs(twin)))
        ex = np.where(d > 0.0, d / (U53 * A), -np.inf)
    return np.where(np.isfinite(twin) & np.isfinite(got), ex, -np.inf)


def sum_excess(got, twin, Bsum, n_terms):
    """(|S_gpu - S_twin| - (n_terms - 1) 2^-53 S) / (2^-53 Bsum) per finite row sum (what K_SUM bounds)."""
    with np.errstate(all="ignore"):
        d = np.abs(got - twin) - (n_terms - 1) * U53 * np.abs(twin)
        ex = np.where(d > 0.0, d / (U53 * Bsum), -np.inf)
    return np.where(np.isfinite(twin) & np.isfinite(got), ex, -np.inf)


def round_up_to_power_of_ten(x):
    return 10.0 ** math.ceil(math.log10(x)) if x > 0.0 else 1.0
