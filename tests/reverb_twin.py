"""Float64 restatement of the reverberation kernels (include/maavss.h "reverberation", csrc/reverb.hip), operation for operation and in
the header's order of additions, and the bounds the tests hold the kernels to.  numpy only: the twin never touches the library.

Convolution.  Every product (double)h * (double)x of two f32 values is exact in f64 (48 significant bits, exponents far inside the f64
range), so a + h * x has the bits of fma(h, x, a) and the only freedom is the order of the additions.  The order: S = 4 partial sums
per output, tap k into partial k mod 4, taps ascending, each from +0.0, then (a0 + a1) + (a2 + a3), one rounding to f32.  `reverb`
adds a whole tap to all outputs at once, which is that order for every output.  The kernel must give these bytes exactly.

Synthesis.  lam and D = 10^(drr_db / 10) arrive as f64.  t_k = (double)g_k * exp((-lam) * k); E = sum t_k^2 in the stated order (each
square rounded, then added); s = sqrt(1 / (D * E)); h_k = f32(s * t_k).  The device's exp and numpy's are both within a few ulp but
are not the same function, so t_k differs from the twin's by a relative eps_t <= 8 * 2^-53 (4 ulp each side, generous); E, a sum of
at most K <= 32768 non-negative terms, then by at most 2 eps_t plus the change of its K roundings, (K + 2) * 2^-53 relative; s by half
of that plus two roundings; s * t_k by less than (K + 16) * 2^-52 < 2^-36 relative.  That is far below half an f32 ulp (2^-24), so the
two f32 roundings either agree or pick neighbouring values: TAP_ULPS = 1.

DRR from stored taps.  h_k = s t_k (1 + d_k), |d_k| <= 2^-24 (a tap below 2^-126 loses more, at most 2^-150 absolute: with
sum h^2 = 1 / D that moves the sum by less than K 2^-275 D relative, nothing), so sum h_k^2 = (1 / D) (1 + e) with
|e| <= 2^-23 + 2^-48 + the f64 terms above: |drr - drr_db| <= 10 / ln 10 * (2^-23 + 2^-48 + (K + 16) * 2^-51) dB (drr_bound_db).

Statistics of the drawn normals.  s is not observable from a row (normalising removed the scale of g), so the pooled statistics use
the scale of the EXPECTED energy: z_k = h_k / (s0 env_k), s0 = sqrt(1 / (D A)), A = sum env_k^2, which is g_k sqrt(A / B) with
B = sum g_k^2 env_k^2.  With c = 2 sum env^4 / A^2 (the relative variance of B) and n tail taps in each of R rows, to first order in
the fluctuations of B (delta method; Cov(sum g^2 / n, B / A) = 2 / n):
    pooled mean:      0,  standard error sqrt((1 + c) / (R n))
    pooled variance:  1 + c - 2 / n,  standard error sqrt((c - 2 / n) / R)       (c >= 2 / n by Cauchy-Schwarz)
    lag-1 autocorrelation sum z_k z_{k+1} / sum z_k^2 within rows:  0,  standard error sqrt((1 + c) / (R (n - 1)))
(normal_stats / normal_stats_expect).  tests/test_reverb_cpu.py checks these formulas on numpy's normals.
"""
import math

import numpy as np

S = 4                      # partial sums per output
MAX_TAPS = 32768
TAP_ULPS = 1               # synthesis: a tap against the twin's tap, in f32 ulps (derived above)


def reverb(src, start, floor, length, rirs, index):
    """src f32 [n_src]; start, floor, index: sequences of B ints; rirs f32 [R, K] -> out f32 [B, length]."""
    src64 = np.asarray(src, dtype=np.float32).astype(np.float64)
    rirs = np.asarray(rirs, dtype=np.float32)
    k_taps = rirs.shape[1]
    out = np.empty((len(start), length), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b, (s0, fl, r) in enumerate(zip(start, floor, index)):
            assert 0 <= fl <= s0 and s0 + length <= src64.shape[0]
            h = rirs[r].astype(np.float64)
            acc = np.zeros((S, length), dtype=np.float64)
            for k in range(k_taps):
                lo = max(0, k - (s0 - fl))              # outputs n < lo would read a sample below the floor: the term is left out
                if lo >= length:
                    break
                acc[k % S, lo:] += h[k] * src64[s0 + lo - k:s0 + length - k]
            out[b] = ((acc[0] + acc[1]) + (acc[2] + acc[3])).astype(np.float32)
    return out


def envelope(lam, k_taps):
    """exp((-lam) * k), k = 0 .. K - 1, f64."""
    return np.exp((-np.float64(lam)) * np.arange(k_taps, dtype=np.float64))


def lam_of(rt60, sr):
    return math.log(1000.0) / (rt60 * sr)


def tail_energy(sq):
    """sum of sq [K] f64 in the kernel's order: thread t of 256 adds quads t, t + 256, ... tap by tap; butterfly over each 64; pairwise."""
    k_taps = sq.shape[0]
    rounds = -(-k_taps // 1024)
    q = np.zeros(rounds * 1024, dtype=np.float64)
    q[:k_taps] = sq
    q = q.reshape(rounds, 256, 4)
    part = np.zeros(256, dtype=np.float64)
    for m in range(rounds):
        for c in range(4):
            part = part + q[m, :, c]
    v = part.reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    w = v[:, 0]
    return (w[0] + w[1]) + (w[2] + w[3])


def rir(noise, lam, drr_lin, predelay):
    """One response from its normals g (f32 [K]) -> (h f32 [K], the unrounded taps f64 [K], s)."""
    g = np.asarray(noise, dtype=np.float32).astype(np.float64)
    k_taps = g.shape[0]
    k0 = min(max(int(predelay), 1), k_taps)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = g * envelope(lam, k_taps)
        t[:k0] = 0.0
        energy = tail_energy(t * t)
        s = math.sqrt(1.0 / (drr_lin * energy)) if energy > 0.0 else 0.0
        exact = np.zeros(k_taps, dtype=np.float64) if s == 0.0 else s * t
    exact[:k0] = 0.0
    exact[0] = 1.0
    return exact.astype(np.float32), exact, s


def drr_db(h, predelay):
    """10 log10(1 / sum_{k >= k0} h_k^2) in f64 (math.fsum: the exactly rounded sum)."""
    tail = np.asarray(h, dtype=np.float64)[int(predelay):]
    return 10.0 * math.log10(1.0 / math.fsum(tail * tail))


def drr_bound_db(k_taps):
    return 10.0 / math.log(10.0) * (2.0 ** -23 + 2.0 ** -48 + (k_taps + 16) * 2.0 ** -51)


def ulp_distance_f32(a, b):
    """Per element, how many f32 values lie between a and b (0 = identical bits up to the sign of zero)."""
    def key(x):
        i = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def normal_stats(rirs, lam, drr_lin, predelay):
    """Pooled mean, variance (about 0) and lag-1 autocorrelation of z = h / (s0 env) over the tails of rirs [R, K] that share
    (lam, drr_lin, predelay) -> (mean, variance, autocorrelation)."""
    h = np.asarray(rirs, dtype=np.float64)
    env = envelope(lam, h.shape[1])[predelay:]
    s0 = math.sqrt(1.0 / (drr_lin * float(np.sum(env * env))))
    z = h[:, predelay:] / (s0 * env)
    return float(z.mean()), float((z * z).mean()), float((z[:, :-1] * z[:, 1:]).sum() / (z * z).sum())


def normal_stats_expect(rows, k_taps, lam, predelay):
    """-> ((expected mean, standard error), (variance, se), (autocorrelation, se)) of normal_stats for standard normal g."""
    env2 = envelope(lam, k_taps)[predelay:] ** 2
    n = env2.shape[0]
    c = 2.0 * float(np.sum(env2 * env2)) / float(np.sum(env2)) ** 2
    return ((0.0, math.sqrt((1.0 + c) / (rows * n))), (1.0 + c - 2.0 / n, math.sqrt((c - 2.0 / n) / rows)),
            (0.0, math.sqrt((1.0 + c) / (rows * (n - 1)))))
