"""The float64 restatement of csrc/bss_eval.hip (include/maavss.h states the same definition): BSS-eval SDR, SIR and SAR of an estimate
against a known target and K known other sources with a time-invariant distortion filter of L taps.  Dense lag matrices,
numpy.linalg.cholesky (a LinAlgError is status 3), the five sums taken directly from the materialised projections.  Also the seeded case
generators the CPU and GPU tests share: white and AR(1)-coloured sources; the estimate is a short FIR of the target (with a tap at L - 1,
so that a filter one tap too short is heard) plus a scaled other source plus noise."""
import functools
import math

import numpy as np

COLUMNS = ("s_tt", "s_ee", "s_ii", "s_aa", "s_pp", "sdr_db", "sir_db", "sar_db", "n_sources", "status")
SCORES = ("sdr_db", "sir_db", "sar_db")
SUMS = ("s_tt", "s_ee", "s_ii", "s_aa", "s_pp")


def lag_matrix(s, filt_len):
    """A[n, t] = s[n - t] for n in [0, N + L - 1), t in [0, L); s is zero outside [0, N)."""
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[0]
    a = np.zeros((n + filt_len - 1, filt_len))
    for t in range(filt_len):
        a[t:t + n, t] = s
    return a


def _db(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10.0 * np.log10(np.float64(num) / np.float64(den)))


def _bad(status, n_sources=0):
    nan = math.nan
    out = dict.fromkeys(SUMS + SCORES, nan)
    out.update(n_sources=n_sources, status=status)
    return out


def live_sources(ref, others):
    """-> the f64 live sources, the target first: another source is live when the sum of its squares is not 0."""
    live = [np.asarray(ref, dtype=np.float64)]
    for s in others:
        s = np.asarray(s, dtype=np.float64)
        if float((s * s).sum()) != 0.0:
            live.append(s)
    return live


def _project(a, ez):
    """-> (coefficients, A c) of the least-squares projection of ez on the columns of a by Cholesky, or None (a pivot is not positive)"""
    g, b = a.T @ a, a.T @ ez
    try:
        c = np.linalg.cholesky(g)
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(c).all():
        return None
    coef = np.linalg.solve(c.T, np.linalg.solve(c, b))
    return coef, a @ coef


def bss_row(est, ref, others=(), filt_len=512):
    """One row -> dict over COLUMNS (floats; n_sources and status ints).  others: a sequence of K arrays like ref (or [K, N])."""
    est, ref = np.asarray(est), np.asarray(ref)
    others = [np.asarray(o) for o in others]
    if not (np.isfinite(est).all() and np.isfinite(ref).all() and all(np.isfinite(o).all() for o in others)):
        return _bad(1)
    ref64 = ref.astype(np.float64)
    if float((ref64 * ref64).sum()) == 0.0:
        return _bad(2)
    live = live_sources(ref, others)
    ez = np.concatenate([est.astype(np.float64), np.zeros(filt_len - 1)])
    mats = [lag_matrix(s, filt_len) for s in live]
    first = _project(mats[0], ez)
    if first is None:
        return _bad(3, len(live))
    p_t = first[1]
    if len(live) > 1:
        full = _project(np.concatenate(mats, axis=1), ez)
        if full is None:
            return _bad(3, len(live))
        p = full[1]
    else:
        p = p_t
    out = dict(s_tt=float((p_t * p_t).sum()), s_ee=float(((ez - p_t) ** 2).sum()), s_ii=float(((p - p_t) ** 2).sum()),
               s_aa=float(((ez - p) ** 2).sum()), s_pp=float((p * p).sum()), n_sources=len(live), status=0)
    out.update(sdr_db=_db(out["s_tt"], out["s_ee"]), sir_db=_db(out["s_tt"], out["s_ii"]), sar_db=_db(out["s_pp"], out["s_aa"]))
    return out


def gram(ref, others, filt_len):
    """The Gram matrix of the live sources (for the condition number the CPU test bounds)."""
    a = np.concatenate([lag_matrix(s, filt_len) for s in live_sources(ref, others)], axis=1)
    return a.T @ a


# ---------------------------------------------------------------------------------------------------------------- seeded cases
def _source(rng, n, coloured):
    x = rng.standard_normal(n)
    if coloured:                                # AR(1), pole 0.7: a spectrum 15 dB from top to bottom
        for i in range(1, n):
            x[i] += 0.7 * x[i - 1]
    return 0.1 * x


def make_case(seed, filt_len, n, k, zero=(), coloured=False, leak=0.3, noise=0.05):
    """-> (est [n], ref [n], others [k, n]) f32.  est = h * ref + leak (others[0] - 0.5 others[1] + ...) + noise, h a filter of filt_len taps
    with taps at 0, 1, 2 and filt_len - 1; the other sources named in `zero` are all-zero (empty Mixer slots) and leak nothing."""
    rng = np.random.default_rng(seed)
    ref = _source(rng, n, coloured).astype(np.float32)
    others = np.stack([_source(rng, n, coloured) for _ in range(k)]).astype(np.float32) if k else np.zeros((0, n), dtype=np.float32)
    for z in zero:
        others[z] = 0.0
    h = np.zeros(filt_len)
    h[0] = 1.0
    if filt_len > 1:
        h[filt_len - 1] += 0.25
    if filt_len > 2:
        h[1] = 0.5
    if filt_len > 3:
        h[2] = -0.3
    est = np.convolve(ref.astype(np.float64), h)[:n]
    for j in range(k):
        est = est + leak * (-0.5) ** j * others[j]
    est = est + noise * 0.1 * rng.standard_normal(n)
    return est.astype(np.float32), ref, others


# (name, L, N, K, all-zero others, coloured): the shapes the issue sets
GPU_CASES = [
    ("L1", 1, 300, 1, (), False),
    ("L2_alone", 2, 64, 0, (), True),
    ("L33", 33, 700, 1, (), True),
    ("L64_one_empty", 64, 1500, 2, (1,), True),
    ("L65", 65, 1000, 1, (), False),
    ("L512_short", 512, 4000, 1, (), True),
    ("L512_clip", 512, 8448, 1, (), True),
    ("L64_chunked", 64, 70000, 1, (), True),
    ("L512_limit", 512, 2048, 3, (), False),
]


@functools.lru_cache(maxsize=None)
def gpu_case(name):
    k = [c[0] for c in GPU_CASES].index(name)
    _, filt_len, n, nk, zero, coloured = GPU_CASES[k]
    return make_case(2000 + k, filt_len, n, nk, zero, coloured)


def case_filter(name):
    return GPU_CASES[[c[0] for c in GPU_CASES].index(name)][1]


@functools.lru_cache(maxsize=None)
def gpu_case_want(name):
    est, ref, others = gpu_case(name)
    return bss_row(est, ref, others, case_filter(name))


# three rows of one call with J = 3, 2 and 1: L = 33, N = 700, K = 2
BATCH = dict(filt_len=33, n=700, k=2, zero=((), (0,), (0, 1)))


def batch_rows():
    """-> (est [3, n], ref [3, n], others [3, 2, n])"""
    b = BATCH
    rows = [make_case(2100 + i, b["filt_len"], b["n"], b["k"], z, True) for i, z in enumerate(b["zero"])]
    return tuple(np.stack([r[q] for r in rows]) for q in range(3))


# overlapping rows: row i of est, ref and the other source is [off + i stride, off + i stride + n) of one signal each
OVERLAP = dict(filt_len=33, n=700, stride=150, rows=3, off_est=1, off_ref=3, off_oth=2)


def overlap_signals():
    o = OVERLAP
    est, ref, others = make_case(2200, o["filt_len"], 3 + (o["rows"] - 1) * o["stride"] + o["n"] + 5, 1, (), True)
    return est, ref, others[0]


def overlap_rows():
    o = OVERLAP
    est, ref, oth = overlap_signals()
    cut = lambda s, off: np.stack([s[off + i * o["stride"]:][:o["n"]] for i in range(o["rows"])])
    return cut(est, o["off_est"]), cut(ref, o["off_ref"]), cut(oth, o["off_oth"])[:, None]


# more rows than workgroups fit on the device at once: row i is [off + i stride, off + i stride + n) of one signal each
MANY = dict(filt_len=33, n=700, stride=3, rows=1024, off=1, checked=(0, 511, 1023))


@functools.lru_cache(maxsize=None)
def many_signals():
    o = MANY
    est, ref, others = make_case(2500, o["filt_len"], o["off"] + (o["rows"] - 1) * o["stride"] + o["n"] + 8, 1, (), True)
    return est, ref, others[0]


def many_row(i):
    """-> (est, ref, others [1, n]) of row i"""
    o = MANY
    a = o["off"] + i * o["stride"]
    est, ref, oth = many_signals()
    return est[a:a + o["n"]], ref[a:a + o["n"]], oth[None, a:a + o["n"]]


# the project's clip in the benchmark's batch: 32 rows of 1024 unknowns, 17 panel workgroups each
CLIP_BATCH = dict(filt_len=512, n=8448, rows=32, checked=(31,))


@functools.lru_cache(maxsize=None)
def clip_batch():
    """-> (est [32, n], ref [32, n], others [32, 1, n]) f32: white sources, est = ref + 0.3 other + noise"""
    o = CLIP_BATCH
    rng = np.random.default_rng(2600)
    ref, oth = (0.1 * rng.standard_normal((o["rows"], o["n"])).astype(np.float32) for _ in range(2))
    est = (ref + 0.3 * oth + 0.005 * rng.standard_normal((o["rows"], o["n"]))).astype(np.float32)
    return est, ref, oth[:, None, :]


def bad_rows():
    """-> (est, ref, others [6, 1, n], kinds), L = 33, n = 700: a NaN in est, an inf in the other source, a silent target and a NaN in the
    last sample of ref, between ordinary rows."""
    kinds = ("fine", "nan_est", "inf_other", "silent_target", "nan_ref_tail", "fine")
    est, ref, oth = [], [], []
    for i, kind in enumerate(kinds):
        e, r, o = make_case(2300 + i, 33, 700, 1, (), True)
        if kind == "nan_est":
            e[123] = np.nan
        elif kind == "inf_other":
            o[0, 400] = np.inf
        elif kind == "silent_target":
            r[:] = 0.0
        elif kind == "nan_ref_tail":
            r[-1] = np.nan
        est.append(e)
        ref.append(r)
        oth.append(o)
    return np.stack(est), np.stack(ref), np.stack(oth), kinds


VALIDATOR_FILTER = 33


def validator_batches():
    """-> two ragged batches (est, ref, noisy, others [B, 1, n]) of 700-sample clips, 3 and 2 rows, for filt_len = 33: the estimate leaks a
    tenth of the other source, the noisy input all of it; the second batch's row 1 has a NaN in the estimate only."""
    out = []
    for b, rows in enumerate((3, 2)):
        cols = [[], [], [], []]
        for i in range(rows):
            e, r, o = make_case(2400 + 10 * b + i, VALIDATOR_FILTER, 700, 1, (), True, leak=0.1)
            q, r2, o2 = make_case(2400 + 10 * b + i, VALIDATOR_FILTER, 700, 1, (), True, leak=1.0)
            assert np.array_equal(r, r2) and np.array_equal(o, o2)
            for c, v in zip(cols, (e, r, q, o)):
                c.append(v)
        out.append([np.stack(c) for c in cols])
    out[1][0][1, 200] = np.nan
    return out
