"""TEST INFRASTRUCTURE ONLY -- restatement of maavss_bank_warp_maps (include/maavss.h, csrc/bank_warp.hip), numpy only.

    axis     output patch i of hp, box (off, len) in pixels:  D = 16 hp,  N = 2 off hp + (2 i + 1) len - 8 hp,  y0 = floor(N / D),
             r = N - y0 D,  w = float64(r) / float64(D),  lo = off // 8,  hi = (off + len - 1) // 8,
             a = clamp(y0, lo, hi),  b = clamp(y0 + 1, lo, hi)                     -- Python integers throughout
    value    m = the stored float32 map converted exactly to float64;
             r0 = (1 - wx) * m[a, c] + wx * m[a, d];  r1 = (1 - wx) * m[b, c] + wx * m[b, d];  v = float32((1 - wy) * r0 + wy * r1)
             a flipped clip writes v to column hp - 1 - j
    norm     mx = fmax over the frame's values from float32(-1e30);  rcp = float32(1) / mx;  stored = v * rcp in float32
    batch    the warped maps go through tests/bank_twin.expected_attn like stored ones

numpy's float64 and float32 operations are IEEE-754 operations rounded one at a time, so this is an exact statement.
"""
import numpy as np


def axis(i, hp, off, length):
    """-> (a, b, w): the two source patches and the weight of the second."""
    d = 16 * hp
    n = 2 * off * hp + (2 * i + 1) * length - 8 * hp
    y0 = n // d                                   # Python's floor division
    r = n - y0 * d
    assert 0 <= r < d
    w = np.float64(r) / np.float64(d)
    lo, hi = off // 8, (off + length - 1) // 8
    return min(max(y0, lo), hi), min(max(y0 + 1, lo), hi), w


def warp_frame(m, box, flip=False, frame_norm=True):
    """m float32 [hp, hp] (as bank_load returns it), box (top, left, height, width) -> float32 [hp, hp]."""
    m = np.asarray(m)
    assert m.dtype == np.float32 and m.ndim == 2 and m.shape[0] == m.shape[1]
    hp = m.shape[0]
    top, left, height, width = (int(x) for x in box)
    assert 0 <= top and 1 <= height and top + height <= 8 * hp and 0 <= left and 1 <= width and left + width <= 8 * hp
    m64 = m.astype(np.float64)
    rows = [axis(i, hp, top, height) for i in range(hp)]
    cols = [axis(j, hp, left, width) for j in range(hp)]
    ya, yb = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    xc, xd = np.array([c[0] for c in cols]), np.array([c[1] for c in cols])
    wy = np.array([r[2] for r in rows], dtype=np.float64)[:, None]
    wx = np.array([c[2] for c in cols], dtype=np.float64)[None, :]
    one = np.float64(1)
    with np.errstate(invalid="ignore", over="ignore"):
        r0 = (one - wx) * m64[ya][:, xc] + wx * m64[ya][:, xd]
        r1 = (one - wx) * m64[yb][:, xc] + wx * m64[yb][:, xd]
        v = ((one - wy) * r0 + wy * r1).astype(np.float32)
    if flip:
        v = v[:, ::-1]
    if frame_norm:
        mx = np.fmax.reduce(v.reshape(-1), initial=np.float32(-1e30))      # a maximum: the order does not matter
        assert mx.dtype == np.float32
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            rcp = np.float32(1) / mx
            v = v * rcp
    assert v.dtype == np.float32
    return np.ascontiguousarray(v)


def warp_clip(maps, size, box, flip=False, frame_norm=True):
    """maps float32 [T, (size // 8)^2] (a clip's unpacked maps) -> float32 [T, hp, hp]."""
    hp = size // 8
    maps = np.asarray(maps)
    return np.stack([warp_frame(f.reshape(hp, hp), box, flip, frame_norm) for f in maps])


def taps(hp, box):
    """-> per output patch the four source patches [(a, c), (a, d), (b, c), (b, d)] as an int array [hp, hp, 4, 2]."""
    top, left, height, width = (int(x) for x in box)
    out = np.empty((hp, hp, 4, 2), dtype=np.int64)
    for i in range(hp):
        a, b, _ = axis(i, hp, top, height)
        for j in range(hp):
            c, d, _ = axis(j, hp, left, width)
            out[i, j] = [(a, c), (a, d), (b, c), (b, d)]
    return out
