"""Float64 restatement of the room-acoustic figures of a response table (include/maavss.h "room-acoustic figures of a response table",
csrc/rir_measure.hip), operation for operation and in the header's order of additions, the bounds the tests hold the kernel and this
twin to, and the cases the CPU and GPU tests share.  numpy only: the twin never touches the library.

Definition (one row h of K f32 taps).  Every square (double)h[k] (double)h[k] is exact in f64, so only the order of the additions
matters.  The taps form blocks of BLOCK = 32 (the last one cut at K):
    s[k] = s[k + 1] + h[k]^2        inside a block, from its last tap towards its first, from +0.0;      T[b] = s[32 b]
    C[B - 1] = +0.0,  C[b] = C[b + 1] + T[b + 1]       from the last block towards the first;            E[k] = s[k] + C[k / 32]
    energy = E[0]
    crossing of level l (threshold c_l = 10^(l / 10) as the caller formed it): the first j >= 1 with E[j] <= E[0] c_l
    t_l = (j - 1) + (d[j - 1] - l) / (d[j - 1] - d[j]),  d[i] = 10 log10(E[i] / E[0]);   NaN when no tap crosses
    edt = (6 t_-10) / sr,   t20 = (3 (t_-25 - t_-5)) / sr,   t30 = (2 (t_-35 - t_-5)) / sr
    early(kb) = per block f[b] = the squares of its taps below kb, first tap towards last, from +0.0; then ((f[0] + f[1]) + ...) from
                +0.0 over the blocks that hold a tap below kb;    late(kb) = E[kb], +0.0 when kb >= K
    c50_db = 10 log10(early / late) at kb = k_early,   drr_db the same at kb = k_direct
A padded tap adds +0.0 to a sum that is +0.0 or positive, which changes no bit: the twin pads where the kernel skips.

Bounds.  u = 2^-53.
  * energy, every E[k], early and late: the kernel's bits (the same exact terms in the same order): EQUALITY.  The comparisons
    E[j] <= E[0] c_l are then the same comparisons: the crossings are the twin's.
  * a dB value d = 10 log10(q): q = E[i] / E[0] is one correctly rounded division of equal operands, the same bits on both sides.
    log10 is not the same function on both sides; as tests/select_twin.py counts it, log10 to 1 ulp and the product with 10 per side
    are 3 u together, taken as 4 u:  |d - d'| <= 4 u |d|                                                            (db_err)
  * a crossing time: num = d[j - 1] - l and den = d[j - 1] - d[j] inherit db_err and round once per side (2 u each), the quotient
    f = num / den rounds once per side, and so does (j - 1) + f:
        |t - t'| <= (e_num + f e_den) / |den| + 2 u f + 2 u t,   e_num = db_err(d[j - 1]) + 2 u |num|,
                                                                 e_den = db_err(d[j - 1]) + db_err(d[j]) + 2 u |den|   (time_bound)
    (den = +inf, an exactly zero E[j]: f = 0 on both sides.)  The figures: edt 6 / sr of its time's bound, t20 3 / sr of the sum of
    its two, t30 2 / sr, plus the product, the difference and the division by sr, one rounding per side each: 6 u of the figure.
  * c50_db, drr_db: early / late is the same correctly rounded division on both sides; the log10 terms: 4 u |value|        (db_bound)
  * against an INDEPENDENT formulation that adds the same non-negative squares in another order (np.cumsum, math.fsum): a sum of m
    terms in any order lies within gamma(m - 1) = (m - 1) u / (1 - (m - 1) u) of the exact sum (Higham, eq. 4.4), two such sums
    within 2 gamma(K - 1); a dB value of a quotient of two such sums within (10 / ln 10) 4 gamma(K - 1), plus db_err    (order_db_err)
    and a time by time_bound with that in db_err's place.  The crossing is the same one only when E[j] and E[j - 1] keep away from
    E[0] c_l: `margins` measures that distance in units of 2 gamma(K - 1) E[0], and the tests ask for MARGIN of them.
Every bound is inflated by SLACK = 1 + 1e-6 in place of the second-order terms.
"""
import math

import numpy as np

BLOCK = 32
CHUNK = 8192                                   # taps the kernel stages at a time (256 blocks): the cases cross it
LEVELS_DB = (-5.0, -10.0, -25.0, -35.0)
THRESHOLDS = tuple(10.0 ** (level / 10.0) for level in LEVELS_DB)
FIGURES = ("energy", "edt", "t20", "t30", "c50_db", "drr_db")
U = 2.0 ** -53
SLACK = 1.0 + 1e-6
MARGIN = 64.0


def gamma(m):
    m = max(int(m), 0)
    return m * U / (1.0 - m * U)


def k_direct(direct_ms, sr):
    return math.floor(direct_ms * sr / 1000.0) + 1


def k_early(sr):
    return round(0.050 * sr)


# ---- the sums, in the header's order ---------------------------------------------------------------------------------------------------
def _blocks(h):
    x = np.asarray(h, dtype=np.float32).astype(np.float64)
    k_taps = x.shape[0]
    nblk = -(-k_taps // BLOCK)
    q = np.zeros(nblk * BLOCK, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q[:k_taps] = x * x
    return q.reshape(nblk, BLOCK), k_taps, nblk


def backward_energy(h):
    """E f64 [K]: the Schroeder backward integral of h in the stated order."""
    q, k_taps, nblk = _blocks(h)
    s_all = np.empty_like(q)
    s = np.zeros(nblk, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(BLOCK - 1, -1, -1):
            s = s + q[:, i]
            s_all[:, i] = s
        carry = np.zeros(nblk, dtype=np.float64)
        for b in range(nblk - 2, -1, -1):
            carry[b] = carry[b + 1] + s_all[b + 1, 0]
        e = s_all + carry[:, None]
    return e.reshape(-1)[:k_taps]


def early_energy(h, kb):
    """The sum of the squares of the taps below kb in the stated forward order."""
    q, k_taps, nblk = _blocks(h)
    index = np.arange(nblk * BLOCK).reshape(nblk, BLOCK)
    q = np.where(index < kb, q, 0.0)
    f = np.zeros(nblk, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(BLOCK):
            f = f + q[:, i]
        nb = nblk if kb >= k_taps else -(-kb // BLOCK)
        e = np.float64(0.0)
        for b in range(nb):
            e = e + f[b]
    return float(e)


def _db(x):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return 10.0 * np.log10(np.float64(x))


def _div(a, b):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.float64(a) / np.float64(b)


def crossing(e, c):
    """The first j >= 1 with E[j] <= E[0] c (None when there is none)."""
    with np.errstate(invalid="ignore", over="ignore"):
        hit = np.flatnonzero(e[1:] <= e[0] * np.float64(c))
    return int(hit[0]) + 1 if hit.size else None


def db_err(d):
    return 4.0 * U * abs(d) if math.isfinite(d) else 0.0


def order_db_err(d, k_taps):
    return 10.0 / math.log(10.0) * 4.0 * gamma(k_taps - 1) + db_err(d)


def time_bound(da, db, level, t, err=db_err):
    """What the crossing time t = (j - 1) + (da - level) / (da - db) may differ by between two sides whose dB values differ by err(d)."""
    if not (math.isfinite(da) and math.isfinite(t)):
        return 0.0                                       # NaN on both sides
    if not math.isfinite(db):
        return 2.0 * U * abs(t) * SLACK                  # f = 0 exactly on both sides
    num, den = da - level, da - db
    f = abs(num / den)
    e_num = err(da) + 2.0 * U * abs(num)
    e_den = err(da) + err(db) + 2.0 * U * abs(den)
    return ((e_num + f * e_den) / abs(den) + 2.0 * U * f + 2.0 * U * abs(t)) * SLACK


class Row:
    """One row's figures (energy, edt, t20, t30, c50_db, drr_db as floats) and what they were made of: e (E f64 [K]), j (the crossing of
    each level or None), t (its time in samples), bound (per figure: what the kernel's value may differ by; 0 = equality)."""


def measure_row(h, sr, kd, ke, thresholds=THRESHOLDS, err=db_err):
    h = np.asarray(h, dtype=np.float32)
    k_taps = h.shape[0]
    r = Row()
    r.e = e = backward_energy(h)
    r.j, r.t, r.da, r.db, tb = [], [], [], [], []
    for level, c in zip(LEVELS_DB, thresholds):
        j = crossing(e, c)
        if j is None:
            t = da = db = float("nan")
        else:
            da, db = float(_db(_div(e[j - 1], e[0]))), float(_db(_div(e[j], e[0])))
            t = float(np.float64(j - 1) + _div(np.float64(da) - level, np.float64(da) - np.float64(db)))
        r.j.append(j), r.t.append(t), r.da.append(da), r.db.append(db)
        tb.append(time_bound(da, db, level, t, err))
    sr = np.float64(sr)
    r.energy = float(e[0])
    r.edt = float((6.0 * np.float64(r.t[1])) / sr)
    r.t20 = float((3.0 * (np.float64(r.t[2]) - np.float64(r.t[0]))) / sr)
    r.t30 = float((2.0 * (np.float64(r.t[3]) - np.float64(r.t[0]))) / sr)
    r.early_e, r.late_e = early_energy(h, ke), float(e[ke]) if ke < k_taps else 0.0
    r.early_d, r.late_d = early_energy(h, kd), float(e[kd]) if kd < k_taps else 0.0
    r.c50_db = float(_db(_div(r.early_e, r.late_e)))
    r.drr_db = float(_db(_div(r.early_d, r.late_d)))
    rate = float(sr)

    def fig(v, times):
        return (times + 6.0 * U * abs(v) * SLACK) if math.isfinite(v) else 0.0

    r.bound = dict(energy=0.0, edt=fig(r.edt, 6.0 * tb[1] / rate), t20=fig(r.t20, 3.0 * (tb[2] + tb[0]) / rate),
                   t30=fig(r.t30, 2.0 * (tb[3] + tb[0]) / rate), c50_db=db_err(r.c50_db) * SLACK, drr_db=db_err(r.drr_db) * SLACK)
    return r


def measure(table, sr, direct_ms=2.5, thresholds=THRESHOLDS):
    """table f32 [n, K] -> the rows' Row objects."""
    kd, ke = k_direct(direct_ms, sr), k_early(sr)
    return [measure_row(h, sr, kd, ke, thresholds) for h in np.asarray(table, dtype=np.float32)]


def figures(rows):
    """-> f64 [n, 6] in FIGURES' order."""
    return np.array([[getattr(r, name) for name in FIGURES] for r in rows], dtype=np.float64)


def margins(row, k_taps):
    """Per level with a crossing: how far E[j] and E[j - 1] keep from E[0] c, in units of 2 gamma(K - 1) E[0] (the most two orders of
    adding the row's squares can move either side of the comparison) -> a list of (level, distance); empty without a crossing."""
    out = []
    unit = 2.0 * gamma(max(k_taps - 1, 1)) * row.e[0]
    for level, c, j in zip(LEVELS_DB, THRESHOLDS, row.j):
        if j is not None:
            lim = row.e[0] * c
            out.append((level, min(abs(row.e[j] - lim), abs(row.e[j - 1] - lim)) / unit if unit > 0 else math.inf))
    return out


def same_or_within(got, want, bound):
    """A figure against the twin's: NaN where the twin has NaN, the same infinity, equality where bound = 0, |diff| <= bound otherwise."""
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want) or bound == 0.0:
        return got == want
    return abs(got - want) <= bound


# ---- the cases the CPU and GPU tests share: name -> (table f32 [n, K], sr, direct_ms) ---------------------------------------------------
def decaying_noise(rng, rows, k_taps, sr, rt60s):
    """Rows g[k] exp(-ln(1000) k / (rt60 sr)) with a unit direct path: the shape of make_rirs' rooms, made on the host."""
    k = np.arange(k_taps, dtype=np.float64)
    t = np.stack([rng.standard_normal(k_taps) * 0.05 * np.exp(-math.log(1000.0) * k / (rt * sr)) for rt in rt60s[:rows]])
    t[:, 0] = 1.0
    return t.astype(np.float32)


def _tap_case(k_taps, seed):
    rng = np.random.default_rng(seed)
    sr = 16000
    if k_taps <= 2:
        return np.array([[1.0, 0.1][:k_taps], [-0.25, 0.9][:k_taps], [3.0, 0.0][:k_taps]], dtype=np.float32), sr, 0.0
    # decay times short enough that the short tables reach every level, and one row that does not reach the lower ones
    scale = min(k_taps, 8000) / 16000.0
    return decaying_noise(rng, 4, k_taps, sr, [0.2 * scale, 0.6 * scale, 1.0 * scale, 40.0 * scale]), sr, 0.0 if k_taps < 64 else 2.5


def _special(seed=21):
    rng = np.random.default_rng(seed)
    t = decaying_noise(rng, 5, 1500, 16000, [0.05, 0.08, 0.03, 0.06, 0.04])
    t[1] = 0.0                                                       # silent: energy 0, NaN elsewhere
    t[2] = 0.0
    t[2, :101] = 1.0                                                 # E[101] = 0 exactly: d = -inf, every lower level crosses at j = 101
    t[3, 700] = np.nan                                               # a NaN beside finite rows
    return t, 16000, 2.5


def _never():
    """K = 101 equal taps: E[j] / E[0] = (101 - j) / 101 > 0.0099 (and never exactly a threshold), so -5 and -10 dB are crossed and -25 and -35 dB never."""
    return np.stack([np.full(101, 1.0, dtype=np.float32), np.full(101, -0.5, dtype=np.float32)]), 16000, 2.5


TAP_COUNTS = (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 8200, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 300)
CASES = {f"k{k}": (lambda k=k: _tap_case(k, 100 + k)) for k in TAP_COUNTS}
CASES["special"] = _special
CASES["never"] = _never
CASES["rate44k"] = lambda: (decaying_noise(np.random.default_rng(5), 3, 6000, 44100, [0.04, 0.08, 0.02]), 44100, 1.0)

# ---- the calibration the CPU and GPU tests share: three rooms, two sources each, requested T20 of 0.15 to 0.25 s --------------------------
CAL_ROOMS = [((3.2, 2.6, 2.4), (1.1, 1.4, 1.2), [(2.4, 0.8, 1.5), (0.7, 2.0, 0.9)]),
             ((4.0, 3.5, 2.5), (1.7, 1.9, 1.2), [(2.9, 0.8, 1.4), (0.6, 2.7, 1.9)]),
             ((5.5, 4.2, 2.8), (2.0, 1.5, 1.3), [(4.1, 3.0, 1.6), (1.0, 3.3, 0.8)])]
CAL_TARGETS = (0.15, 0.2, 0.25)
CAL_SR, CAL_TAPS, CAL_TOL, CAL_MAX_ITER = 16000, 3072, 0.02, 12       # 3072 = the default measure_len for the longest target: ceil(0.75 * 0.25 * 16000 / 1024) * 1024
