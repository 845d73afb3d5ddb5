"""numpy float64 twin of csrc/tensor_stats.hip (per-segment statistics, torch.histc's f32 bin formula, clip_grad_norm_'s scale) and
the case table tests/test_grad_stats_cpu.py and tests/test_grad_stats_gpu.py share.

Bounds the tests assert, and where they come from:
  sumsq   every square of an f32 is exact in f64 (24 x 24 significand bits) and every term is >= 0, so ANY order of f64 additions of
          the n squares is within (n - 1) * 2^-53 relative of the exact sum (each addition rounds a partial sum that is <= the
          total; first order in u = 2^-53, (n u)^2 < 1e-20 for the sizes here).  The twin's own sum is math.fsum, the correctly
          rounded exact sum.  The gate is (n - 1) * 2^-53: a segment of one element must match exactly.
  norm / scale  single f32 roundings of f64 expressions of sumsq: 2^-24 from the rounding + the sumsq error halved by the square
          root (< 2^-30 for n <= 2^20) -- inside the 2^-23 relative gate.
  min, max, counts, histogram  exact.
"""
import math
import types

import numpy as np

U53 = 2.0 ** -53
U23 = 2.0 ** -23
BINS = (1, 64, 1024)


def seg_stats(x, exact=True):
    """x: f32 array -> dict(sumsq f64, min, max f32 (NaN without a finite element), nan, posinf, neginf).  `exact`: the correctly
    rounded sum (math.fsum); without it numpy's pairwise f64 sum (within ~log2(n) * 2^-53, for the multi-million-element tensors of
    the model-level test, whose gates are 2^-23)."""
    x = np.asarray(x, dtype=np.float32).ravel()
    fin = x[np.isfinite(x)]
    sq = fin.astype(np.float64) ** 2
    return dict(sumsq=math.fsum(sq.tolist()) if exact else float(sq.sum()),
                min=np.float32(fin.min()) if fin.size else np.float32(np.nan),
                max=np.float32(fin.max()) if fin.size else np.float32(np.nan),
                nan=int(np.isnan(x).sum()), posinf=int(np.isposinf(x).sum()), neginf=int(np.isneginf(x).sum()))


def hist_f32(x, bins):
    """torch.histc(x, bins) of the finite elements: bin = int((x - lo) * f32(bins) / (hi - lo)) in f32, one rounding per operation;
    bins -> bins - 1; lo == hi -> [lo - 1, hi + 1]; no finite element -> zeros."""
    x = np.asarray(x, dtype=np.float32).ravel()
    fin = x[np.isfinite(x)]
    if fin.size == 0:
        return np.zeros(bins, dtype=np.int64)
    lo, hi = np.float32(fin.min()), np.float32(fin.max())
    if lo == hi:
        lo, hi = np.float32(lo - np.float32(1)), np.float32(hi + np.float32(1))
    d = (fin - lo).astype(np.float32)
    e = (d * np.float32(bins)).astype(np.float32)
    q = (e / np.float32(hi - lo)).astype(np.float32)
    b = np.minimum(q.astype(np.int64), bins - 1)
    return np.bincount(b, minlength=bins).astype(np.int64)


def clip(stats, max_norm, grad_scale=1.0):
    """stats: the seg_stats of the selected segments -> (total_sumsq, norm64, scale64) in f64: clip_grad_norm_'s formula for the
    gradient after grad_scale (an f32 in the ABI), times grad_scale.  NaN with any NaN, otherwise +inf / 0 with an inf."""
    gs = float(np.float32(grad_scale))
    total = math.fsum(s["sumsq"] for s in stats)
    t = total
    if any(s["nan"] for s in stats):
        t = float("nan")
    elif any(s["posinf"] or s["neginf"] for s in stats):
        t = float("inf")
    norm = math.sqrt(t) * gs if t == t else float("nan")
    if max_norm is None:
        return total, norm, None
    c = float(max_norm) / (norm + 1e-6)
    c = 1.0 if c > 1.0 else c
    return total, norm, gs * c


def seg_lengths(ch):
    return [1, 3, 4, 5, 63, 64, 65, ch - 1, ch, ch + 1, 2 * ch + 7, 16]


# what each segment of the table holds, by position in seg_lengths()
KINDS = ["one", "all_nonfinite", "zeros", "repeated", "integers", "tiny", "with_nan", "with_infs", "unit", "integers", "mixed", "milli"]
FINITE = [k not in ("all_nonfinite", "with_nan", "with_infs") for k in KINDS]


def make_cases(ch, seed=20240):
    """-> (names, offsets, numels, buf): the synthetic layout (offsets 64-aligned as FlatParams makes them, padding zero) and its flat
    f32 buffer.  Seeded normal values at scales 1e-6 .. 1e2; every value is normal or zero (no denormals)."""
    rng = np.random.default_rng(seed)
    lens = seg_lengths(ch)
    names, offsets, off = [], [], 0
    for i, (k, kind) in enumerate(zip(lens, KINDS)):
        names.append(f"s{i:02d}_{kind}")
        offsets.append(off)
        off = (off + k + 63) // 64 * 64
    buf = np.zeros(off, dtype=np.float32)
    for o, k, kind in zip(offsets, lens, KINDS):
        v = rng.standard_normal(k)
        if kind == "all_nonfinite":
            v = np.array([np.nan, np.inf, -np.inf])[:k]
        elif kind == "zeros":
            v = np.zeros(k)
        elif kind == "repeated":
            v = np.full(k, 0.37)
        elif kind == "integers":
            v = rng.integers(-8, 9, size=k).astype(np.float64)
            v[0], v[-1] = -8, 8                      # range 16: with 64 bins every integer sits on a bin edge
        elif kind == "tiny":
            v = v * 1e-6
        elif kind == "with_nan":
            v[k // 2] = np.nan
        elif kind == "with_infs":
            v = v * 1e2
            v[5], v[k - 3], v[k // 2] = np.inf, -np.inf, np.inf
        elif kind == "mixed":
            v = v * 10.0 ** rng.integers(-6, 3, size=k)
        elif kind == "milli":
            v = v * 1e-3
        seg = v.astype(np.float32)
        tiny = np.isfinite(seg) & (seg != 0) & (np.abs(seg) < np.finfo(np.float32).tiny)
        seg[tiny] = 0
        buf[o:o + k] = seg
    return names, offsets, lens, buf


def fake_flat(names, offsets, numels, total, params=None, grads=None):
    """The part of trainer.FlatParams that TensorStats / ModelWatch read."""
    return types.SimpleNamespace(names=list(names), offsets=dict(zip(names, offsets)), shapes={n: (int(k),) for n, k in zip(names, numels)},
                                 total=int(total), params=params, grads=grads)
