"""Float64 restatement of the image-source room responses (include/maavss.h "image-source room responses", csrc/room_rir.hip),
operation for operation, and the bounds the tests hold the kernel and this twin to.  numpy only: the twin never touches the library.

Definition (one row = one room, one microphone m, one source s; L the room, beta the six walls x0 x1 y0 y1 z0 z1).  Per axis a, lattice
index n in [-N_a, N_a] and parity p in {0, 1}:
    u_a = ((2 n) L_a + (1 - 2 p) s_a) - m_a        reflections: |n - p| off wall a0, |n| off wall a1
    d  = sqrt((ux ux + uy uy) + uz uz)             d0: the same with n = 0, p = 0 on every axis
    A  = (((((x0^e1 x1^e2) y0^e3) y1^e4) z0^e5) z1^e6) d0) / d         integer powers by ipow below, 0^0 = 1
    tau = (d - d0) (sr / c),  k0 = floor(tau),  f = tau - k0
    for m = -H + 1 .. H:  pos = ((m - f) + H) R,  i = min(floor(pos), 2 H R - 1),  t = pos - i,  w = T[i] + t (T[i + 1] - T[i])
                          q = rint((A w) 2^40) as int64 (ties to even),  acc[k0 + m] += q  when 0 <= k0 + m < K
    h[k] = f32((double)acc[k] 2^-40)
Every f64 operation is rounded on its own in the order written.  The sum is an integer sum: no order of the images can change it
(`taps(order=...)` visits them in any order).  i is capped so that pos = 2 H R (f = 0, m = H) reads T[2 H R - 1] and T[2 H R] with
t = 1: w = a + (0 - a) = 0 exactly, as T[2 H R] = 0.

The table T (kernel_table): g(x) = sinc(x) (1 + cos(pi x / H)) / 2 at x = i / R - H, the entries at integer x set to exactly 0 and to
exactly 1 at x = 0.  It is an INPUT of the entry point: the twin takes the table the Python layer built, so no sin or cos is compared.

Bound of the linear interpolation (test 2 of tests/test_room_rir_cpu.py holds the twin's taps to g evaluated directly).  Between two
nodes 1 / R apart, |lerp - g| <= max|g''| / (8 R^2).  With sinc(x) = int_0^1 cos(pi x t) dt:  |sinc| <= 1, |sinc'| <= pi / 2,
|sinc''| <= pi^2 / 3;  the Hann factor v has |v| <= 1, |v'| <= pi / (2 H), |v''| <= pi^2 / (2 H^2);  so
    max|g''| <= pi^2 (1 / 3 + 1 / (2 H) + 1 / (2 H^2))                                                  (g2_bound)
The nodes themselves and the three operations of the lerp are within 2^-48 of exact (a few f64 roundings of values <= 1; the zeroed
integer nodes differ from the computed ones by less than 2^-52).  A tap that one image reaches therefore lies within
    |A| (g2_bound / (8 R^2) + 2^-48) + 2^-40 + 2^-24 |h|                                                  (lerp_bound)
of A g(k - tau): the interpolation, one quantum of the fixed point, one rounding to f32.  Where the test forms tau by another route
(math.dist), the two values of tau (below 2^9 samples, each a few roundings of 2^-44) differ by less than tau_err = 2^-40, which
|g'| <= |sinc'| + |v'| <= pi / 2 + pi / (2 H) <= pi turns into at most |A| pi tau_err.

Bound against a float sum (test 3).  A tap with N_k contributions, each rounded to a multiple of 2^-40 (error <= 2^-41), against the
same terms added as f64 in any order (error <= N_k u sum|A w|, u = 2^-53):  N_k 2^-41 + N_k u sum|A w|                (float_sum_bound)
"""
import math

import numpy as np

SCALE = 2.0 ** 40
C_SOUND = 343.0
MAX_CELLS = 1 << 31


def kernel_table(half_width, resolution):
    """T f64 [2 H R + 1]: the windowed sinc at x = i / R - H, exact 0 at the integers and exact 1 at 0."""
    h, r = half_width, resolution
    x = np.arange(2 * h * r + 1, dtype=np.float64) / r - h
    t = np.sinc(x) * (0.5 * (1.0 + np.cos(np.pi * x / h)))
    t[::r] = 0.0
    t[h * r] = 1.0
    return t


def g_direct(x, half_width):
    """The kernel itself, not through the table (0 outside |x| < H)."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.abs(x) < half_width, np.sinc(x) * (0.5 * (1.0 + np.cos(np.pi * x / half_width))), 0.0)


def g2_bound(half_width):
    return math.pi ** 2 * (1.0 / 3.0 + 1.0 / (2.0 * half_width) + 1.0 / (2.0 * half_width ** 2))


def lerp_bound(amp, h, half_width, resolution, tau_err=0.0):
    return abs(amp) * (g2_bound(half_width) / (8.0 * resolution ** 2) + 2.0 ** -48 + math.pi * tau_err) + 2.0 ** -40 + 2.0 ** -24 * np.abs(h)


def float_sum_bound(count, abs_sum):
    return count * 2.0 ** -41 + count * 2.0 ** -53 * abs_sum


def ipow(b, e):
    """b^e by the stated algorithm, elementwise (b f64 scalar or array, e non-negative integers)."""
    e = np.array(e, dtype=np.int64)
    b = np.broadcast_to(np.asarray(b, dtype=np.float64), e.shape).copy()
    r = np.ones(e.shape, dtype=np.float64)
    while e.any():
        odd = (e & 1) == 1
        r[odd] = r[odd] * b[odd]
        b = b * b
        e >>= 1
    return r


def direct_distance(mic, src):
    u = [np.float64(1.0) * np.float64(s) - np.float64(m) for s, m in zip(src, mic)]      # (0 L + s) - m = s - m
    return np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])


def lattice_bounds(dims, mic, src, k_taps, half_width, sr, c=C_SOUND):
    """N_a = floor(Rmax / (2 L_a)) + 1 with Rmax = d0 + (K + H) c / sr: an image with |n| > N_a on axis a has |u_a| > 2 N_a L_a >= Rmax
    (|(1 - 2 p) s - m| < 2 L), so tau > K + H and its first tap k0 - H + 1 lies behind K - 1."""
    rmax = float(direct_distance(mic, src)) + (k_taps + half_width) * c / sr
    return [int(math.floor(rmax / (2.0 * float(l)))) + 1 for l in dims]


def cells(bounds):
    return 8 * (2 * bounds[0] + 1) * (2 * bounds[1] + 1) * (2 * bounds[2] + 1)


def _axis(length, s, m, b0, b1, n_max):
    """All (n, p) of one axis -> (u, b0^|n - p| , b1^|n|), flat over n-major, p-minor."""
    n = np.repeat(np.arange(-n_max, n_max + 1, dtype=np.int64), 2)
    p = np.tile(np.array([0, 1], dtype=np.int64), 2 * n_max + 1)
    u = ((2 * n).astype(np.float64) * np.float64(length) + (1 - 2 * p).astype(np.float64) * np.float64(s)) - np.float64(m)
    return u, ipow(b0, np.abs(n - p)), ipow(b1, np.abs(n))


def images(dims, mic, src, beta, k_taps, sr, half_width, c=C_SOUND, bounds=None):
    """Every image of the lattice box that reaches a tap in [0, K) -> (A, tau) flat f64 arrays (z-slab by z-slab: iz, then ix, iy), and
    the number of images of the box."""
    bounds = lattice_bounds(dims, mic, src, k_taps, half_width, sr, c) if bounds is None else bounds
    assert cells(bounds) <= MAX_CELLS
    ux, x0, x1 = _axis(dims[0], src[0], mic[0], beta[0], beta[1], bounds[0])
    uy, y0, y1 = _axis(dims[1], src[1], mic[1], beta[2], beta[3], bounds[1])
    uz, z0, z1 = _axis(dims[2], src[2], mic[2], beta[4], beta[5], bounds[2])
    d0 = direct_distance(mic, src)
    rate = np.float64(sr) / np.float64(c)
    xy = (ux * ux)[:, None] + (uy * uy)[None, :]
    pxy = ((x0 * x1)[:, None] * y0[None, :]) * y1[None, :]
    amps, taus = [], []
    for iz in range(uz.shape[0]):
        d = np.sqrt(xy + uz[iz] * uz[iz])
        tau = (d - d0) * rate
        k0 = np.floor(tau)
        keep = (k0 + half_width >= 0) & (k0 - half_width + 1 < k_taps)
        if not keep.any():
            continue
        amp = (((pxy[keep] * z0[iz]) * z1[iz]) * d0) / d[keep]
        amps.append(amp)
        taus.append(tau[keep])
    amp = np.concatenate(amps) if amps else np.zeros(0)
    tau = np.concatenate(taus) if taus else np.zeros(0)
    return amp, tau, cells(bounds)


def taps(amp, tau, k_taps, table, half_width, resolution, order=None):
    """The integer accumulator of the images (A, tau), visited in `order` (a permutation of their indices; None: as given)
    -> (acc int64 [K], count int64 [K] contributions per tap, abs_sum f64 [K] sum of |A w| per tap)."""
    if order is not None:
        amp, tau = amp[order], tau[order]
    h, r = half_width, resolution
    acc, count, abs_sum = np.zeros(k_taps, dtype=np.int64), np.zeros(k_taps, dtype=np.int64), np.zeros(k_taps, dtype=np.float64)
    k0 = np.floor(tau)
    f = tau - k0
    k0 = k0.astype(np.int64)
    for m in range(-h + 1, h + 1):
        pos = ((np.float64(m) - f) + np.float64(h)) * np.float64(r)
        i = np.minimum(np.floor(pos).astype(np.int64), 2 * h * r - 1)
        t = pos - i.astype(np.float64)
        w = table[i] + t * (table[i + 1] - table[i])
        aw = amp * w
        q = np.rint(aw * SCALE).astype(np.int64)
        k = k0 + m
        ok = (k >= 0) & (k < k_taps)
        np.add.at(acc, k[ok], q[ok])
        np.add.at(count, k[ok], 1)
        np.add.at(abs_sum, k[ok], np.abs(aw[ok]))
    return acc, count, abs_sum


def to_f32(acc):
    return (acc.astype(np.float64) * 2.0 ** -40).astype(np.float32)


class Response:
    """One row: h f32 [K], acc int64 [K], count [K], abs_sum [K], n_images (those that reach a tap), n_contrib, n_box, integer_tau (how
    many audible images besides the direct path fall exactly on a sample)."""


def response(dims, mic, src, beta, k_taps, sr=16000, half_width=8, resolution=32, c=C_SOUND, table=None, bounds=None):
    table = kernel_table(half_width, resolution) if table is None else np.asarray(table, dtype=np.float64)
    assert table.shape == (2 * half_width * resolution + 1,)
    amp, tau, n_box = images(dims, mic, src, beta, k_taps, sr, half_width, c, bounds)
    res = Response()
    res.acc, res.count, res.abs_sum = taps(amp, tau, k_taps, table, half_width, resolution)
    res.h = to_f32(res.acc)
    res.amp, res.tau = amp, tau
    res.n_images, res.n_contrib, res.n_box = int(amp.shape[0]), int(res.count.sum()), n_box
    res.integer_tau = int(((tau == np.floor(tau)) & (tau > 0) & (amp != 0)).sum())
    return res


def table_of(rooms, k_taps, sr=16000, half_width=8, resolution=32, c=C_SOUND, table=None):
    """rooms: a list of (dims, mic, [sources], beta) -> h f32 [sum of sources, K], row = room-major, source-minor."""
    return np.stack([response(d, m, s, b, k_taps, sr, half_width, resolution, c, table).h for d, m, srcs, b in rooms for s in srcs])


def brute_force(dims, mic, src, beta, k_taps, sr, half_width, resolution, table, bounds, c=C_SOUND):
    """The same definition as scalar Python floats, the images in another order (x outermost, parities before lattice indices,
    descending n), the taps summed as f64 -> h f64 [K]."""
    def power(b, e):
        r = 1.0
        while e:
            if e & 1:
                r = r * b
            b = b * b
            e >>= 1
        return r

    lx, ly, lz = (float(v) for v in dims)
    d0 = float(direct_distance(mic, src))
    rate = float(sr) / float(c)
    h, r = half_width, resolution
    out = [0.0] * k_taps
    for px in (1, 0):
        for py in (1, 0):
            for pz in (1, 0):
                for nx in range(bounds[0], -bounds[0] - 1, -1):
                    ux = (float(2 * nx) * lx + float(1 - 2 * px) * float(src[0])) - float(mic[0])
                    ax = power(float(beta[0]), abs(nx - px)) * power(float(beta[1]), abs(nx))
                    for ny in range(bounds[1], -bounds[1] - 1, -1):
                        uy = (float(2 * ny) * ly + float(1 - 2 * py) * float(src[1])) - float(mic[1])
                        axy = (ax * power(float(beta[2]), abs(ny - py))) * power(float(beta[3]), abs(ny))
                        for nz in range(bounds[2], -bounds[2] - 1, -1):
                            uz = (float(2 * nz) * lz + float(1 - 2 * pz) * float(src[2])) - float(mic[2])
                            d = math.sqrt((ux * ux + uy * uy) + uz * uz)
                            tau = (d - d0) * rate
                            k0 = math.floor(tau)
                            if k0 - h + 1 >= k_taps or k0 + h < 0:
                                continue
                            amp = (((axy * power(float(beta[4]), abs(nz - pz))) * power(float(beta[5]), abs(nz))) * d0) / d
                            f = tau - k0
                            for m in range(-h + 1, h + 1):
                                k = k0 + m
                                if 0 <= k < k_taps:
                                    pos = ((float(m) - f) + float(h)) * float(r)
                                    i = min(math.floor(pos), 2 * h * r - 1)
                                    t = pos - i
                                    out[k] += amp * (float(table[i]) + t * (float(table[i + 1]) - float(table[i])))
    return np.array(out, dtype=np.float64)


def t20(h, sr):
    """Reverberation time from the Schroeder integral of h: three times the time the backward-integrated energy takes from -5 to
    -25 dB (first crossings, linear interpolation between samples); NaN when the response does not reach -25 dB."""
    e = np.cumsum((np.asarray(h, dtype=np.float64) ** 2)[::-1])[::-1]
    db = 10.0 * np.log10(e / e[0] + 1e-300)

    def crossing(level):
        below = np.flatnonzero(db <= level)
        if below.size == 0 or below[0] == 0:
            return float("nan")
        j = below[0]
        return (j - 1) + (db[j - 1] - level) / (db[j - 1] - db[j])

    return 3.0 * (crossing(-25.0) - crossing(-5.0)) / sr


def eyring_beta(dims, rt60):
    lx, ly, lz = (float(v) for v in dims)
    volume, surface = lx * ly * lz, 2.0 * (lx * ly + ly * lz + lx * lz)
    return min(max(math.exp(-0.0805 * volume / (surface * rt60)), 0.0), 1.0)


# ---- the cases the CPU and GPU tests share: (name, K, H, R, sr, [(dims, mic, [sources], beta)]) ----------------------------------------------
def _u(b):
    return (b,) * 6


SIX = (0.9, 0.0, 0.7, 1.0, 0.55, 0.8)                                            # six different walls, a 0 and a 1
SMALL = ((2.0, 2.2, 2.1), (0.9, 1.3, 1.0), [(1.4, 0.7, 1.2)], _u(0.9))           # many images per tap: the densest shells
LARGE = ((10.0, 8.0, 4.0), (4.0, 3.0, 1.5), [(7.5, 5.0, 2.0)], _u(0.8))
MID = ((4.0, 3.5, 2.5), (1.7, 1.9, 1.2), [(2.9, 0.8, 1.4)], SIX)
MID3 = (MID[0], MID[1], [(2.9, 0.8, 1.4), (0.6, 2.7, 1.9), (3.3, 3.0, 0.5)], SIX)
MID5 = (MID[0], MID[1], MID3[2] + [(1.0, 1.0, 1.0), (2.0, 1.75, 2.2)], _u(0.75))
NEAR = ((3.5, 3.0, 2.5), (1.5, 1.5, 1.25), [(1.55, 1.5, 1.25)], _u(0.85))        # the source 0.05 m from the microphone
WALLS = ((3.5, 3.0, 2.5), (0.05, 1.1, 1.3), [(3.45, 2.95, 0.05)], _u(0.85))      # microphone and source 0.05 m from walls
# an exact integer tau needs (d - d0) (sr / c) exact: sr = 64 * 343 = 21952 makes sr / c = 64 exactly, and coordinates in multiples of
# 1 / 8 m make every axial image's distance (uy = uz = 0 and the like) a binary fraction: tau = 64 (d - d0) is an integer there
AXIAL = ((2.5, 3.0, 2.5), (0.75, 1.5, 1.25), [(1.25, 1.5, 1.25)], _u(0.8))
AXIAL_SR = 21952

CASES = [
    ("k1", 1, 8, 32, 16000, [MID]), ("k2", 2, 8, 32, 16000, [MID]), ("kH", 8, 8, 32, 16000, [MID]),
    ("k4095", 4095, 8, 32, 16000, [MID]), ("k4096", 4096, 8, 32, 16000, [MID3]), ("k4097", 4097, 8, 32, 16000, [SMALL]),
    ("k8200", 8200, 8, 32, 16000, [LARGE]),
    ("h1", 700, 1, 32, 16000, [MID]), ("h32", 700, 32, 32, 16000, [MID]), ("r1", 700, 8, 1, 16000, [MID]), ("h32r1", 300, 32, 1, 16000, [MID]), ("h1r1", 300, 1, 1, 16000, [MID]),
    ("big_table", 500, 32, 256, 16000, [MID]),                                          # 16385 entries: the table is read from global memory
    ("large300", 300, 8, 32, 16000, [LARGE]),
    ("near", 1500, 8, 32, 16000, [NEAR]), ("walls", 1500, 8, 32, 16000, [WALLS]), ("axial", 1200, 8, 32, AXIAL_SR, [AXIAL]),
    ("s5", 900, 8, 32, 16000, [MID5]),
    ("two_sizes", 1000, 8, 32, 16000, [SMALL, LARGE, NEAR]),                       # lattice bounds that differ from row to row
]
