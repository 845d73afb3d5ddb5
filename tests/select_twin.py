"""TEST INFRASTRUCTURE ONLY -- float64 restatement of the clip activity statistics and the selection rule (include/maavss.h,
"per-clip activity statistics of the clip bank"; maavss_amd/csrc/clip_select.hip; maavss_amd/sampler.py), the cases the CPU and GPU
tests share, and the bounds they gate on.

The sums below run in the header's order (thread- / lane-strided partial sums in index order, the xor butterfly, the pairwise
combination of four waves, index order after that), operation for operation.  The GPU tests therefore gate on EQUALITY, bit for bit
(NaN in the same places), wherever a statistic is made of those sums and correctly rounded divisions alone: energy, the recording
level, D_f, motion_mean and motion_peak (`same_bits`).  That is what holds the kernels to "the ONE order stated" in the header: another
lane count per segment, butterfly or wave combination changes bits.  rms_db and rel_db go through log10, which is not the same function
on both sides: they gate on the derived bounds below, and so does tests/test_clip_select_cpu.py, whose independent formulations
(np.sum, np.mean) add in another order.

Bounds.  u = 2^-53.  Every sum is of non-negative terms (exact squares, or |differences| that both sides round identically), so a sum
of m terms in ANY order lies within gamma(m - 1) = (m - 1) u / (1 - (m - 1) u) relative of the exact sum (Higham, Accuracy and
Stability of Numerical Algorithms, eq. 4.4), and two such sums within 2 gamma(m - 1) (1 + gamma) of each other.  Each later division
adds one rounding u per side.  With n = J hop clip samples, N the recording's samples, P map values a frame, T frames a clip:
    E_j            2 gamma(hop - 1)                                   relative
    energy         2 gamma(n - 1)                                     relative          REL["energy"]
    level          2 gamma(N - 1)                                     relative
    rms_db         (10 / ln 10) (2 gamma(n - 1) + 2 u) + 4 u |rms_db| absolute: the argument's error through d(10 log10 x) = (10 / ln 10) dx / x,
                   plus, per side, log10 to 1 ulp (HIP's documented f64 log10 error; glibc's is below it) and the product with 10: 1.5 u
                   each, 3 u together, taken as 4 u
    rel_db         the same with the argument's error 2 gamma(n - 1) + 2 gamma(N - 1) + 6 u (three divisions per side)
    D_f            2 gamma(P - 1) + 2 u <= 2 gamma(P + 1)            relative (terms identical on both sides; sum, one division)
    motion_mean    2 gamma(P + 1) + 2 gamma(T - 2) + 2 u <= 2 gamma(P + T + 1)   relative
    motion_peak    2 gamma(P + 1)                                     relative (a maximum of D_f)
Every bound is inflated by (1 + 1e-6) in place of the (1 + gamma) cross terms.  On the GPU only the rms_db and rel_db rows are used
(the others serve the CPU test and the margins).  peak, n_bad, n_active, recording and the reason bytes are exact: equality.  The decisions (n_active, reasons) are the twin's because the inputs keep a margin: see `margin_violations`.
"""
import math
from fractions import Fraction

import numpy as np

import bank_twin

U = 2.0 ** -53
CHUNK = 16384
SLACK = 1.0 + 1e-6
REASONS = ("too_quiet", "too_quiet_for_recording", "few_active_segments", "static", "scene_cut", "clipped", "nonfinite")
# the thresholds every test uses (min_active_fraction times J is formed where J is known)
THRESHOLDS = dict(min_rms_db=-50.0, min_rel_db=-20.0, min_active_fraction=0.5, min_motion=1e-3, max_motion_peak=0.3, max_peak=1.0)
RANGE_DB = 40.0


def gamma(m):
    m = max(int(m), 0)
    return m * U / (1.0 - m * U)


# ---- the sums, in the header's order ---------------------------------------------------------------------------------------------
def _strided(terms, width):
    """`width` partial sums: partial t adds terms t, t + width, ... in index order, from 0."""
    pad = -len(terms) % width
    rows = np.concatenate([terms, np.zeros(pad)]).reshape(-1, width)          # x + 0.0 = x: the padding changes no bit
    acc = np.zeros(width)
    with np.errstate(invalid="ignore", over="ignore"):
        for row in rows:
            acc = acc + row
    return acc


def _butterfly(v):
    """64 values -> what every lane holds after v[l] += v[l ^ o], o = 32, 16, 8, 4, 2, 1."""
    lanes = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[lanes ^ o]
    return v[0]


def _squares(x):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float64) ** 2


def recording_level(x):
    """Sum of squares of the recording's finite samples: chunk partials (256 threads, four waves), then the partials in index order."""
    x = np.asarray(x, dtype=np.float32)
    sq = np.where(np.isfinite(x), _squares(x), 0.0)
    total = 0.0
    for c0 in range(0, len(x), CHUNK):
        t = _strided(sq[c0:c0 + CHUNK], 256)
        w = [_butterfly(t[64 * k:64 * k + 64]) for k in range(4)]
        total = total + ((w[0] + w[1]) + (w[2] + w[3]))
    return total


def segment_energy(seg):
    return _butterfly(_strided(_squares(seg), 64))


def frame_motion(maps):
    """maps float32 [F, P] as stored (unpacked) -> D float64 [F - 1]."""
    m = np.asarray(maps, dtype=np.float32).astype(np.float64)
    return np.array([_butterfly(_strided(np.abs(m[f + 1] - m[f]), 64)) / float(m.shape[1]) for f in range(m.shape[0] - 1)])


def stored(maps, storage):
    """What the bank's batches read back: the maps themselves, or the 16-bit round trip."""
    maps = np.asarray(maps, dtype=np.float32)
    return maps if storage == "f32" else bank_twin.unpack(bank_twin.pack(maps))


def _db(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(np.float64(x))


def clip_row(audio, s, D, v, T, J, hop, level, n_rec_samples, range_db=RANGE_DB):
    """One clip's statistics (a dict of scalars) and its segment powers: audio = the bank's sample buffer, D = the bank's pair table."""
    n = J * hop
    x = np.asarray(audio[s:s + n], dtype=np.float32)
    E = np.array([segment_energy(x[j * hop:(j + 1) * hop]) for j in range(J)])
    energy = 0.0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for e in E:
            energy = energy + e
        rec_power = np.float64(level) / float(n_rec_samples)
        floor_p = rec_power * (10.0 ** (-range_db / 10.0))
        seg_power = E / float(hop)
        mean = np.float64(energy) / float(n)
        rel = _db(mean / rec_power)
    good = x[~np.isnan(x)]
    msum = mmax = 0.0
    if T > 1:
        for d in D[v:v + T - 1]:
            msum = msum + d
            mmax = d if d > mmax else mmax
        msum = msum / float(T - 1)
    row = dict(energy=energy, rms_db=_db(mean), rel_db=rel, peak=np.float32(np.abs(good).max() if len(good) else 0.0),
               n_bad=int((~np.isfinite(x)).sum()), n_active=int((seg_power >= floor_p).sum()), motion_mean=msum, motion_peak=mmax)
    return row, seg_power, floor_p


def select(table, segments, thresholds=None, reject_nonfinite=True):
    """The rule of maavss_bank_clip_select: a dict of columns -> uint8 reasons.  A threshold that is None is not tested."""
    th = dict(THRESHOLDS if thresholds is None else thresholds)
    n = len(table["recording"])
    m = np.zeros(n, dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        if th.get("min_rms_db") is not None:
            m |= (table["rms_db"] < th["min_rms_db"]).astype(np.uint8) << 0
        if th.get("min_rel_db") is not None:
            m |= (table["rel_db"] < th["min_rel_db"]).astype(np.uint8) << 1
        if th.get("min_active_fraction") is not None:
            m |= (table["n_active"].astype(np.float64) < th["min_active_fraction"] * segments).astype(np.uint8) << 2
        if th.get("min_motion") is not None:
            m |= (table["motion_mean"] < th["min_motion"]).astype(np.uint8) << 3
        if th.get("max_motion_peak") is not None:
            m |= (table["motion_peak"] > th["max_motion_peak"]).astype(np.uint8) << 4
        if th.get("max_peak") is not None:
            m |= (table["peak"] >= np.float32(th["max_peak"])).astype(np.uint8) << 5
    if reject_nonfinite:
        m |= (table["n_bad"] > 0).astype(np.uint8) << 6
    return m


# ---- the cases -------------------------------------------------------------------------------------------------------------------
RATES_A, RATES_B = (30, 16000), (30, 630)          # samples a frame: 533.33 (s_k of either parity) and 21 (s_k odd whenever k frame_hop is)
# frame_size, storage, clip_frames, frame_hop, hop, hops_per_frame, (fps, sr), recordings
CASES = [
    (8, "f32", 1, 1, 1, 1, RATES_A, 3),
    (8, "u16", 2, 1, 3, 1, RATES_B, 3),
    (16, "f32", 2, 2, 66, 8, RATES_A, 4),
    (16, "u16", 5, 1, 3, 8, RATES_B, 3),
    (40, "f32", 5, 2, 66, 1, RATES_B, 4),
    (40, "u16", 5, 5, 1, 8, RATES_A, 3),
    (40, "f32", 1, 1, 66, 8, RATES_A, 3),
    (16, "u16", 2, 2, 1, 1, RATES_A, 4),
    (8, "f32", 5, 5, 66, 8, RATES_B, 3),
    (224, "u16", 2, 1, 3, 8, RATES_B, 3),
    (224, "f32", 5, 2, 1, 1, RATES_A, 2),
]
CLIPS = (4, 3, 5, 2)          # clips of recordings 0 .. 3: unequal lengths


def case_id(case):
    s, storage, t, fh, hop, hpf, (fps, sr), n_rec = case
    return f"S{s}-{storage}-T{t}-fh{fh}-hop{hop}-hpf{hpf}-sr{sr}-R{n_rec}"


def sample_start(k, fh, fps, sr):
    return round(Fraction(k * fh * sr) / Fraction(fps))


_BUILT = {}


def build(case):
    """-> dict(recordings=[(audio f32 [L], maps f32 [F, P])], tables..., table=the twin's columns, seg=[(segment powers, floor)]).
    Computed once per case and shared; nobody writes to it.

    Recording 0: noise at 0.1 with clip 1 wholly silent, a sample at exactly 1.0 in clip 0, an inf at the end of clip 2 and a NaN at
    the end of clip 3 (behind the silent clip however much the clips overlap); maps that drift a little, with one jump between frames 0 and 1.  Recording 1: digital silence and frozen
    frames, between two loud neighbours.  Recording 2: loud noise, drifting maps.  Recording 3: noise at 0.001 (below -50 dB) whose
    frames freeze after the first."""
    if case in _BUILT:
        return _BUILT[case]
    size, storage, T, fh, hop, hpf, (fps, sr), n_rec = case
    P, J = (size // 8) ** 2, hpf * T
    n = J * hop
    rng = np.random.default_rng(1000 + CASES.index(case))
    recordings, tab = [], []
    f0 = s0 = 0
    for r in range(n_rec):
        c = CLIPS[r]
        starts = [sample_start(k, fh, fps, sr) for k in range(c)]
        F, L = (c - 1) * fh + T, starts[-1] + n
        drift = (0.3 + 0.05 * rng.random((F, P))).astype(np.float32)
        if r == 0:
            audio = (0.1 * rng.standard_normal(L + 7)).astype(np.float32)
            audio[starts[1]:starts[1] + n] = 0.0
            audio[starts[2] + n - 1] = np.inf
            audio[starts[3] + n - 1] = np.nan
            audio[0] = 1.0
            maps = drift
            maps[1:] += np.float32(0.5)
        elif r == 1:
            audio = np.zeros(L + 7, dtype=np.float32)
            audio[L:] = 0.7                                   # behind the last clip: never banked
            maps = np.repeat(drift[:1], F, axis=0)
        elif r == 2:
            audio = np.clip(0.5 * rng.standard_normal(L + 7), -0.99, 0.99).astype(np.float32)
            maps = drift
        else:
            audio = (0.001 * rng.standard_normal(L + 7)).astype(np.float32)
            maps = np.concatenate([drift[:1], np.repeat(drift[1:2], F - 1, axis=0)]) if F > 1 else drift
        recordings.append((audio, np.ascontiguousarray(maps)))
        tab.append((f0, s0, F, L, c, starts))
        f0, s0 = f0 + F, s0 + L
    bank_audio = np.concatenate([a[:t[3]] for (a, _), t in zip(recordings, tab)])
    bank_maps = stored(np.concatenate([m for _, m in recordings]), storage)
    D = frame_motion(bank_maps) if bank_maps.shape[0] > 1 else np.zeros(0)
    levels = [recording_level(bank_audio[t[1]:t[1] + t[3]]) for t in tab]
    rows, seg, where = [], [], []
    for r, (rf, rs, F, L, c, starts) in enumerate(tab):
        for k in range(c):
            v, s = rf + k * fh, rs + starts[k]
            row, seg_power, floor_p = clip_row(bank_audio, s, D, v, T, J, hop, levels[r], L)
            rows.append(dict(row, recording=r))
            seg.append((seg_power, floor_p))
            where.append((v, s, r))
    dtypes = dict(peak=np.float32, n_bad=np.int32, n_active=np.int32, recording=np.int32)
    table = {k: np.array([row[k] for row in rows], dtype=dtypes.get(k, np.float64)) for k in rows[0]}
    out = dict(recordings=recordings, tab=tab, where=where, table=table, seg=seg, levels=levels, D=D, bank_audio=bank_audio, bank_maps=bank_maps,
               P=P, J=J, n=n, T=T, hop=hop, reasons=select(table, J))
    _BUILT[case] = out
    return out


# ---- bounds and margins ----------------------------------------------------------------------------------------------------------
def bounds(b):
    """Per column: (absolute bound array) for a built case, from the twin's own values."""
    t, n, P, T = b["table"], b["n"], b["P"], b["T"]
    N = np.array([b["tab"][r][3] for r in t["recording"]], dtype=np.float64)
    k = 10.0 / math.log(10.0)
    g_n = 2.0 * gamma(n - 1)
    g_N = np.array([2.0 * gamma(x - 1) for x in N])
    with np.errstate(invalid="ignore"):
        out = dict(energy=g_n * np.abs(t["energy"]),
                   rms_db=k * (g_n + 2 * U) + 4 * U * np.abs(t["rms_db"]),
                   rel_db=k * (g_n + g_N + 6 * U) + 4 * U * np.abs(t["rel_db"]),
                   motion_mean=2.0 * gamma(P + T + 1) * np.abs(t["motion_mean"]),
                   motion_peak=2.0 * gamma(P + 1) * np.abs(t["motion_peak"]))
    return {c: v * SLACK for c, v in out.items()}


def close(got, want, bound):
    """Elementwise: equal where the twin is not finite (-inf, NaN in the same places), within the bound elsewhere."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    same_special = np.array_equal(np.isnan(got[~fin]), np.isnan(want[~fin])) and np.array_equal(got[~fin][~np.isnan(want[~fin])],
                                                                                                 want[~fin][~np.isnan(want[~fin])])
    with np.errstate(invalid="ignore"):
        return bool(same_special and np.all(np.isfinite(got[fin])) and np.all(np.abs(got[fin] - want[fin]) <= np.broadcast_to(bound, want.shape)[fin]))


def same_bits(got, want):
    """float64 arrays equal bit for bit, a NaN (of any payload) counting as equal to a NaN."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return bool(got.shape == want.shape and np.array_equal(np.isnan(got), nan)
                and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)))


def margin_violations(b, thresholds=None):
    """The condition on the inputs that makes the device's decisions the twin's: no statistic within 1000 times its bound of the
    threshold it is compared with, no segment power within 1000 times the bound of the comparison of the activity floor.  Values that
    are not finite decide the same on both sides (a comparison with NaN is false, -inf is below every threshold) and a comparison
    whose two sides are both exact -- a sum of zeros against a floor of zero, a frozen clip's 0 against a threshold -- has a bound of
    0: the margin asks for strictly more than 1000 times the bound, or for a bound of exactly 0.  -> list of descriptions."""
    th = dict(THRESHOLDS if thresholds is None else thresholds)
    t, bd, bad = b["table"], bounds(b), []
    for col, key in (("rms_db", "min_rms_db"), ("rel_db", "min_rel_db"), ("motion_mean", "min_motion"), ("motion_peak", "max_motion_peak")):
        if th.get(key) is None:
            continue
        for i, (v, e) in enumerate(zip(t[col], bd[col])):
            if np.isfinite(v) and e > 0 and abs(v - th[key]) <= 1000.0 * e:
                bad.append(f"clip {i}: {col} = {v!r} within {1000 * e:.3g} of {key} = {th[key]}")
    # n_active against min_active_fraction * J, peak against max_peak and n_bad against 0 compare exact values: nothing to keep clear of
    for i, (seg_power, floor_p) in enumerate(b["seg"]):
        N = b["tab"][t["recording"][i]][3]
        rel = 2.0 * gamma(b["hop"] - 1) + 2.0 * gamma(N - 1) + 6 * U
        for j, p in enumerate(seg_power):
            e = rel * max(abs(p), abs(floor_p)) * SLACK
            if np.isfinite(p) and np.isfinite(floor_p) and e > 0 and abs(p - floor_p) <= 1000.0 * e:
                bad.append(f"clip {i} segment {j}: power {p!r} within {1000 * e:.3g} of the floor {floor_p!r}")
    return bad
