"""TEST INFRASTRUCTURE ONLY -- twins of the f32 kernels that carry video into and out of the ViT (attention-map post-process,
patch gather, the Enhancer's window / stitch copies, the frame transform, the phasegram), and the error bounds derived from them.
Plain numpy and torch on the CPU.  The twins restate torch's definitions and the formulas the kernels' comments cite;
tests/test_video_edges_cpu.py checks each of them against an independent restatement before the GPU tests rely on them.

Every `mutant` / keyword switch below turns ONE deliberate defect on (px <= wp, a dropped clip_start clamp, ...): the CPU test
uses them to show that the committed cases tell such a kernel from a correct one."""
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of float32
F32 = np.float32


# ------------------------------------------------------------------------------------------------ 1. attention maps
def attn_pass1(att):
    """att [F, heads, n] -> (small [F, n], fmax [F]) in float32, one IEEE operation per step: head sum in head order, frame
    maximum, r = 1 / max, v = s * r, fmax = max v."""
    att = np.ascontiguousarray(att, dtype=F32)
    s = np.zeros((att.shape[0], att.shape[2]), F32)
    for h in range(att.shape[1]):
        s = s + att[:, h]
    r = F32(1) / s.max(1)
    v = s * r[:, None]
    return v, v.max(1)


def upsample8(small, hp, wp, H, W, px_le=False):
    """small [F, hp * wp] -> [F, H, W]: nearest x 8, zero outside the patch grid.  px_le: the defect `px <= wp` (column block wp
    reads the element behind the row)."""
    f = small.shape[0]
    out = np.zeros((f, H, W), F32)
    out[:, :hp * 8, :wp * 8] = np.repeat(np.repeat(small.reshape(f, hp, wp), 8, 1), 8, 2)
    if px_le and W > wp * 8:
        flat = np.concatenate([small.reshape(-1), np.zeros(1, F32)])
        idx = (np.arange(f)[:, None] * hp * wp + np.arange(hp)[None, :] * wp + wp)
        out[:, :hp * 8, wp * 8:] = np.repeat(flat[idx], 8, 1)[:, :, None]
    return out


def attn_maps(att, H, W, clip_frames, attn_diff, px_le=False, diff_crosses_clip=False):
    """The whole post-process -> (out [F, H, W], small, fmax).  attn_diff: d_t = v_t - v_{t-1} inside a clip, frame 0 zero, the clip
    maximum (starting at 0) in every fmax of the clip.  sc = 1 / max(fmax over the clip); out = small * sc.
    diff_crosses_clip: the defect of differencing over the whole frame axis."""
    hp, wp = H // 8, W // 8
    v, fmax = attn_pass1(att)
    f, n = v.shape
    if attn_diff:
        c = v.reshape(-1, clip_frames, n)
        d = np.zeros_like(c)
        d[:, 1:] = c[:, 1:] - c[:, :-1]
        if diff_crosses_clip:
            d[1:, 0] = c[1:, 0] - c[:-1, -1]
        m = np.maximum(F32(0), d.reshape(d.shape[0], -1).max(1))
        v, fmax = d.reshape(f, n), np.repeat(m, clip_frames)
    if clip_frames > 0:
        sc = np.repeat(F32(1) / fmax.reshape(-1, clip_frames).max(1), clip_frames)
        o = v * sc[:, None]
    else:
        o = v
    return upsample8(o, hp, wp, H, W, px_le), v, fmax


# ------------------------------------------------------------------------------------------------ 2. patchify
def patchify_ref(frames, dtype):
    """frames [F, 3, H, W] float32 tensor -> rows [F * (n + 1), 192] in torch.bfloat16 (dtype 0) or torch.float16 (2): F.unfold of
    the top-left 8hp x 8wp region in (c, dy, dx) order, rounded to nearest even; row 0 of each frame (the CLS slot) zeros."""
    f, _, h, w = frames.shape
    hp, wp = h // 8, w // 8
    td = torch.float16 if dtype == 2 else torch.bfloat16
    rows = torch.nn.functional.unfold(frames[:, :, :hp * 8, :wp * 8], 8, stride=8).transpose(1, 2)
    out = torch.zeros(f, hp * wp + 1, 192, dtype=td)
    out[:, 1:] = rows.to(td)
    return out.view(f * (hp * wp + 1), 192)


def round_bf16_bits(x):
    """float32 array -> uint16 bf16 bits by the IEEE rule on the integer image (round to nearest, ties to even); finite inputs."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ 3. window kernels
def clip_first_frame(clip_start, c, n_frames, clip_frames, clamp=True):
    f0 = int(clip_start[c])
    return min(max(f0, 0), n_frames - clip_frames) if clamp else f0


def clip_scale(maps, fmax, clip_start, clip_frames, attn_diff, clamp=True):
    """maps [n_frames, E], fmax [n_frames] or None -> clip_rcp [n_clips] = 1 / clip maximum: of the zero-padded temporal difference
    (attn_diff; the maximum starts at 0), of fmax, or of the clip's map values.  clamp=False: the defect of a dropped clip_start
    clamp (frames taken modulo n_frames, so that the twin still reads memory it owns)."""
    maps = np.asarray(maps, dtype=F32)
    n_frames = maps.shape[0]
    rcp = np.zeros(len(clip_start), F32)
    for c in range(len(clip_start)):
        fr = (clip_first_frame(clip_start, c, n_frames, clip_frames, clamp) + np.arange(clip_frames)) % n_frames
        m = maps[fr]
        if attn_diff:
            mx = F32(0) if clip_frames < 2 else np.maximum(F32(0), (m[1:] - m[:-1]).max())
        elif fmax is not None:
            mx = np.asarray(fmax, dtype=F32)[fr].max()
        else:
            mx = m.max()
        with np.errstate(divide="ignore"):
            rcp[c] = F32(1) / F32(mx)
    return rcp


def attn_windows(maps, clip_rcp, clip_start, clip_frames, num_seq, win_frames, w0, n_win, H, W, upsample, attn_diff,
                 clamp=True, zero_k0=True, px_le=False):
    """-> [n_win, win_frames, H, W]: window w = w0 + i, clip c = min(w // num_seq, n_clips - 1), clip frame
    k = min(w % num_seq + t, clip_frames - 1), recording frame f0 + k; value map * rcp, or (map_k - map_{k-1}) * rcp with 0 at k = 0.
    upsample: maps are [n_frames, (H/8)(W/8)], nearest x 8, zero outside the patch grid; else [n_frames, H * W]."""
    maps = np.asarray(maps, dtype=F32)
    n_frames, n_clips = maps.shape[0], len(clip_start)
    hp, wp = H // 8, W // 8
    rows = np.zeros((n_win * win_frames, maps.shape[1]), F32)
    for i in range(n_win):
        w = w0 + i
        c = min(w // num_seq, n_clips - 1)
        f0 = clip_first_frame(clip_start, c, n_frames, clip_frames, clamp)
        for t in range(win_frames):
            k = min(w % num_seq + t, clip_frames - 1)
            f = (f0 + k) % n_frames
            m = maps[f]
            if attn_diff:
                m = np.zeros_like(m) if (k == 0 and zero_k0) else m - maps[(f - 1) % n_frames]
            rows[i * win_frames + t] = m * clip_rcp[c]
    out = upsample8(rows, hp, wp, H, W, px_le) if upsample else rows
    return out.reshape(n_win, win_frames, H, W)


def stft_windows(y, hops_per_frame, num_seq, win_frames, w0, n_win):
    """y [n_clips, 2, clip_rows, F] -> [n_win, 2, a * win_frames, F] = STFT frames a j .. a (j + win_frames) of clip c."""
    a = hops_per_frame
    out = np.zeros((n_win, 2, a * win_frames, y.shape[3]), F32)
    for i in range(n_win):
        w = w0 + i
        c, j = min(w // num_seq, y.shape[0] - 1), w % num_seq
        out[i] = y[c, :, a * j:a * (j + win_frames)]
    return out


def stitch(pred, clip_absmax, n_clips, num_seq, w0, out):
    """pred [n_win, 2, a, F] -> rows a w .. a w + a - 1 of out [2, a * n_clips * num_seq, F] (in place; the other rows are left
    alone) = pred * g_c, g_c = clip_absmax[c] + 1e-7 in float32, or 1."""
    a = pred.shape[2]
    for i in range(pred.shape[0]):
        w = w0 + i
        c = min(w // num_seq, n_clips - 1)
        g = F32(1) if clip_absmax is None else F32(clip_absmax[c]) + F32(1e-7)
        out[:, a * w:a * w + a] = pred[i] * g
    return out


# ------------------------------------------------------------------------------------------------ 4. video transform
def vt_taps(n_in, S, antialias):
    """taps per output coordinate the tables hold: torch's 2 for bilinear; its interp_size-based maximum is below
    2 ceil(in / S) + 3 for the antialiased filter."""
    return 2 * ((n_in + S - 1) // S) + 3 if antialias else 2


def vt_tables(n_in, S, antialias, short=False, fold=True):
    """Tap tables of one axis exactly as torch's float32 resize derives them (align_corners=False) -> start [S] int64,
    count [S] int64, weights [S, taps] float32 (zero behind `count`).
      bilinear (area_pixel_compute_source_index, guard_index_and_lambda): all float32 --
        scale = float(in) / float(S); real = max(scale * (o + 0.5f) - 0.5f, 0), the product and the subtraction as ONE fused
        multiply-add (what torch's CPU build and a kernel built with -ffp-contract=fast both make of that expression; the two-rounding
        form differs from torch in the last bit at 37 -> 20, 37 -> 68, 53 -> 68); start = min(int(real), in - 1);
        l1 = clamp(real - start, 0, 1); weights (1 - l1, l1); the second tap is clamped to the last pixel in the gather.
      antialias (HelperInterpLinear::_compute_indices_min_size_weights_aa): float32 variables, double where a literal makes it so --
        support = float(1.0 * scale) or 1 (scale < 1); invscale = float(1.0 / scale) or 1; center = float(scale * (o + 0.5));
        start = max(int(center - support + 0.5), 0); count = clamp(min(int(center + support + 0.5), in) - start, 0, taps);
        w_j = triangle(float((float(j + start) - center + 0.5) * invscale)) -- the integer meets the float32 centre first, so that
        difference is a float32 one -- each divided by their float32 running sum.
    tests/test_video_edges_cpu.py holds these tables to torch's bit for bit (the resize of one-hot rows is the weight table).
    fold: where the bilinear gather clamps both taps onto the last pixel (start == in - 1; always so for a one-pixel axis) they are
    one tap of weight 1 -- (1 - l1) + l1 in exact arithmetic, but only within 2^-24 of it in float32, which would keep the resize of
    a one-pixel crop from being constant.  fold=False gives torch's table as it stands.
    short: the defect of a tap count one too small (the last tap dropped, no renormalisation)."""
    taps = vt_taps(n_in, S, antialias)
    start, count = np.zeros(S, np.int64), np.zeros(S, np.int64)
    wts = np.zeros((S, taps), F32)
    scale = F32(n_in) / F32(S)
    for o in range(S):
        if antialias:
            support = F32(1.0 * float(scale)) if scale >= 1 else F32(1)
            invscale = F32(1.0 / float(scale)) if scale >= 1 else F32(1)
            center = F32(float(scale) * (o + 0.5))
            st = max(int(float(center) - float(support) + 0.5), 0)
            cn = min(max(min(int(float(center) + float(support) + 0.5), n_in) - st, 0), taps)
            tot = F32(0)
            for j in range(cn):
                x = F32(abs((float(F32(j + st) - center) + 0.5) * float(invscale)))
                v = F32(1) - x if x < 1 else F32(0)
                wts[o, j] = v
                tot = F32(tot + v)
            if tot != 0:
                wts[o, :cn] = wts[o, :cn] / tot
        else:
            real = F32(float(scale) * (o + 0.5) - 0.5)                      # exact in double, rounded once: the fused form
            real = F32(0) if real < 0 else real
            st = min(int(real), n_in - 1)
            cn = 2
            l1 = min(max(F32(real - F32(st)), F32(0)), F32(1))
            wts[o, 0], wts[o, 1] = (F32(1), F32(0)) if fold and st >= n_in - 1 else (F32(1) - l1, l1)
        if short:
            wts[o, cn - 1] = 0
        start[o], count[o] = st, cn
    return start, count, wts


def vt_affine(mean, std):
    """the float32 constants of the entry point: a = 1 / (255 std), b = -mean / std (formed in double, rounded once)"""
    mean, std = [float(F32(m)) for m in mean], [float(F32(s)) for s in std]
    return (np.array([F32(1.0 / (255.0 * s)) for s in std], np.float64), np.array([F32(-m / s) for m, s in zip(mean, std)], np.float64))


def vt_resize_f64(crop, S, antialias, short=False):
    """crop [F, h, w, 3] uint8 -> (acc [F, 3, S, S] float64 = the separable sum over the float32 tables, horizontal first;
    adds [S, S] = x taps + y taps used per output pixel)."""
    f, h, w, _ = crop.shape
    ys, yc, wy = vt_tables(h, S, antialias, short)
    xs, xc, wx = vt_tables(w, S, antialias, short)
    src = crop.astype(np.float64)
    ix = np.minimum(xs[:, None] + np.arange(wx.shape[1])[None], w - 1)              # [S, tx]
    iy = np.minimum(ys[:, None] + np.arange(wy.shape[1])[None], h - 1)              # [S, ty]
    hs = (src[:, :, ix, :] * wx.astype(np.float64)[None, None, :, :, None]).sum(3)  # [F, h, S, 3]
    acc = (hs[:, iy] * wy.astype(np.float64)[None, :, :, None, None]).sum(2)        # [F, S(oy), S(ox), 3]
    return acc.transpose(0, 3, 1, 2), (yc[:, None] + xc[None, :]).astype(np.float64)


def video_transform(video, boxes, clip_frames, S, mean, std, antialias, autocontrast, short=False):
    """video [F, H0, W0, 3] uint8 (numpy), boxes [(top, left, h, w)] per clip -> (want, bound), float64 [F, 3, S, S].
    want: float64 summation over the float32 tables, the affine step with the entry point's float32 a_c, b_c, then autocontrast from
    the twin's own minimum and maximum.
    bound, per element, on a float32 evaluation of the same tables in any order:
      u (x taps + y taps + 2) sum|w_y||w_x| p a_c  +  one float32 ulp of the result
    (every product and every addition of the two sums, the multiplication by a_c and the addition of b_c round once, each an error
    of at most u times a partial result that sum|w||w| p a_c bounds; the weights are >= 0, so that sum is acc a_c).
    With autocontrast, r = (v - lo) * scale, scale = 1 / (hi - lo): the errors e of v and e* (the plane's largest e) of lo reach r times
    scale, hi - lo carries the relative error 2 e* / (hi - lo), and the subtraction, the difference hi - lo, the division and the
    product round once each: bound_r = (e + e*) scale + r (2 e* / (hi - lo) + 4u) + ulp(r).
    A plane with hi == lo (a one-pixel crop: its float32 weights sum to exactly 1, which tests/test_video_edges_cpu.py asserts) takes
    autocontrast's scale = 1, min = 0 branch, clamp(v, 0, 1)."""
    a, b = vt_affine(mean, std)
    want = np.zeros((video.shape[0], 3, S, S))
    bound = np.zeros_like(want)
    for c, (top, left, h, w) in enumerate(boxes):
        sl = slice(c * clip_frames, (c + 1) * clip_frames)
        crop = video[sl, top:top + h, left:left + w]
        acc, adds = vt_resize_f64(crop, S, antialias, short)
        v = acc * a[None, :, None, None] + b[None, :, None, None]
        e = U * (adds[None, None] + 2) * acc * a[None, :, None, None] + ulp32(v)
        if autocontrast:
            lo, hi = v.min((2, 3), keepdims=True), v.max((2, 3), keepdims=True)
            es = e.max((2, 3), keepdims=True)
            flat_plane = hi == lo
            span = np.where(flat_plane, 1.0, hi - lo)
            r = np.clip(np.where(flat_plane, v, (v - lo) / span), 0, 1)
            e = np.where(flat_plane, e, (e + es) / span + r * (2 * es / span + 4 * U)) + ulp32(r)
            v = r
        want[sl], bound[sl] = v, e
    return want, bound


def ulp32(x):
    """spacing of float32 at |x| (elementwise)"""
    return np.spacing(np.abs(np.asarray(x)).astype(F32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ 5. phasegram
D_SCAN = 32     # additions on the path of one scanned element: 16 in the thread, 6 wave steps, 3 wave totals, 1 offset (rounded up)
ATAN_ULPS = 8   # allowance for atan2f itself, in units of u pi


def phasegram_spectrum(frames):
    """frames [B, T, P, P] float32 tensor -> float64 complex spectrum in OUTPUT coordinates: fft2, then fftshift over all four axes,
    as the reference calls it."""
    return torch.fft.fftshift(torch.fft.fft2(frames.double()))


def self_conjugate_mask(P):
    m = torch.zeros(P, P, dtype=torch.bool)
    for u in (0, P // 2):
        for v in (0, P // 2):
            m[u, v] = True
    return m


def phasegram_undecided(z, delta):
    """z [B, T, P, P] complex128 (output coordinates) -> bool mask of the bins whose float32 phase is not decidable given an error of
    delta on the spectrum: |z| <= 2 delta, or Re <= delta and |Im| <= delta (the branch cut).  The four self-conjugate bins are real
    by construction (the kernel zeroes their imaginary part): only their sign can be lost, |Re| <= delta."""
    und = (z.abs() <= 2 * delta) | ((z.real <= delta) & (z.imag.abs() <= delta))
    sc = self_conjugate_mask(z.shape[-1])
    und[..., sc] = z.real[..., sc].abs() <= delta
    return und


def phasegram_left_out(und, diff, cumulative):
    """und [B, T, P, P] -> bool [B, T, P * P] of the output elements that are not compared: with `cumulative` the whole frame of an
    undecided bin, without it the element; with `diff` the same element (frame) of the successor too."""
    b, t = und.shape[:2]
    out = und.reshape(b, t, -1).clone()
    if cumulative:
        out = out.any(-1, keepdim=True).expand(b, t, und.shape[-1] ** 2).clone()
    if diff:
        out[:, 1:] |= out[:, :-1].clone()
    return out


def phasegram_bound(z, delta, diff, cumulative, normalize, ref):
    """Per-element bound [B, T, P * P] (float64) on |kernel - ref| for the decided elements, ref = the float64 phasegram
    [B, T, P * P]: the phase of a bin is off by at most asin(delta / |z|) plus atan2f's own ATAN_ULPS u pi (nothing but the latter
    at a self-conjugate bin); along the scan those add up, the float32 scan adds D_SCAN u sum|phase| and the scale two roundings,
    all divided by 2 pi N; (phase + pi) / 2 pi costs three roundings instead; `diff` adds the bounds of both frames and one rounding;
    `normalize` multiplies by 1 / max and adds the relative error of the maximum (at most the largest bound) and two roundings."""
    b, t, p, _ = z.shape
    n = p * p
    mag = z.abs().clamp_min(2 * delta)
    e = torch.asin(torch.clamp(delta / mag, max=1.0))
    e[..., self_conjugate_mask(p)] = 0.0
    e = (e + ATAN_ULPS * U * math.pi).reshape(b, t, n)
    ph = torch.angle(z).reshape(b, t, n)
    if cumulative:
        val = torch.cumsum(ph, -1) / (2 * math.pi * n)
        bound = (torch.cumsum(e, -1) + D_SCAN * U * torch.cumsum(ph.abs(), -1)) / (2 * math.pi * n) + 2 * U * val.abs()
    else:
        val = (ph + math.pi) / (2 * math.pi)
        bound = e / (2 * math.pi) + 3 * U
    if diff:
        d = torch.zeros_like(val)
        d[:, 1:] = val[:, 1:] - val[:, :-1]
        bd = torch.zeros_like(bound)
        bd[:, 1:] = bound[:, 1:] + bound[:, :-1] + U * d[:, 1:].abs()
        val, bound = d, bd
    if normalize:
        m = float(val.abs().max())
        bound = bound / m + ref.abs() * (float(bound.max()) / m + 2 * U) + U * ref.abs()
    return bound
