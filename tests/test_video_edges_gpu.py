"""The f32 kernels that carry video into and out of the ViT, off their benched shapes and through the C-ABI: the attention-map
post-process (vit_misc.hip), the patch gather, the Enhancer's window and stitch copies (av_windows.hip), the frame transform
(video_transform.hip) and the phasegram (phasegram.hip), each held to its twin in oracle/video_edges_ref.py at the shapes of
tests/video_edges_cases.py -- bit for bit where every step is one IEEE operation, within a bound derived from the twin where the
kernel sums.  tests/test_video_edges_cpu.py checks the twins, the caps and the sensitivity of these cases on the CPU.

Workspaces are handed over full of NaN, outputs carry sentinel elements behind their end that must survive, and every bounded
comparison prints its worst error as a fraction of its bound (`pytest -s`)."""
import numpy as np
import pytest
import torch

import video_edges_cases as cs
from oracle import video_edges_ref as vref

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
GUARD = 4096                # floats behind an output that must stay untouched


def _call(name, *args):
    from maavss_amd import _lib
    _lib.call(name, *args)
    torch.cuda.synchronize()


def _st():
    from maavss_amd import _lib
    return _lib.stream_ptr()


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return (t if dtype is None else t.to(dtype)).cuda()


def guarded(numel, fill=SENTINEL):
    return torch.full((numel + GUARD,), fill, device="cuda", dtype=torch.float32)


def guard_intact(buf, numel):
    return bool((buf[numel:] == SENTINEL).all())


def poisoned(numel):
    return torch.full((max(numel, 1),), float("nan"), device="cuda", dtype=torch.float32)


def assert_bits(got, want, what):
    """got: device float32 tensor, want: numpy float32 of the same element count -> every element identical (signs of zero too)"""
    g = got.detach().cpu().contiguous().view(torch.int32).reshape(-1)
    w = torch.from_numpy(np.ascontiguousarray(want, dtype=np.float32)).view(torch.int32).reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not torch.equal(g, w):
        bad = (g != w).nonzero().reshape(-1)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {g.numel()} elements differ, first at flat index {i}: "
                             f"got {got.reshape(-1)[i].item()!r}, want {float(np.asarray(want).reshape(-1)[i])!r}")


# ------------------------------------------------------------------------------------------------ 1. attention maps
@pytest.mark.parametrize("case", cs.ATTN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_attention_maps_bit_for_bit(case):
    """maavss_vit_attn_maps, _checked and _pass1 against the float32 twin: head sum in head order, frame max, r = 1 / max, v = s r,
    fmax = max v, the clip difference and its maximum, sc = 1 / clip max, out = v sc upsampled -- no step can be contracted into
    an fma and the division is correctly rounded, so every element of out (and of small and fmax for pass 1) must be identical.
    n = 1 .. 784 (one to four trips of the j += 256 loops, waves that hold only the identity), W % 8 = 4 (px < wp false),
    clip_frames 0 and 1, and 1025 frames of 128 x 128, where pass 2 runs its 16384 blocks a second, ragged time."""
    h, w, heads, frames, tc, diff = case
    n = (h // 8) * (w // 8)
    att = dev(cs.attn_input(case))
    want, _, _ = cs.attn_want(case)
    numel = frames * h * w
    out, ws = guarded(numel), poisoned(frames * (n + 1))
    _call("maavss_vit_attn_maps", att.data_ptr(), out.data_ptr(), ws.data_ptr(), frames, heads, h, w, tc, diff, _st())
    assert_bits(out[:numel], want, f"attn_maps {case}")
    assert guard_intact(out, numel)
    out2, ws2, flag = guarded(numel), poisoned(frames * (n + 1)), torch.zeros(1, dtype=torch.int32, device="cuda")
    _call("maavss_vit_attn_maps_checked", att.data_ptr(), out2.data_ptr(), ws2.data_ptr(), frames, heads, h, w, tc, diff, flag.data_ptr(), _st())
    assert torch.equal(out2, out) and int(flag.item()) == 0
    small, fmax = guarded(frames * n), guarded(frames)
    _call("maavss_vit_attn_maps_pass1", att.data_ptr(), small.data_ptr(), fmax.data_ptr(), frames, heads, n, flag.data_ptr(), _st())
    ws_, wf_ = vref.attn_pass1(cs.attn_input(case))
    assert_bits(small[:frames * n], ws_, f"pass1 small {case}")
    assert_bits(fmax[:frames], wf_, f"pass1 fmax {case}")
    assert guard_intact(small, frames * n) and guard_intact(fmax, frames) and int(flag.item()) == 0


@pytest.mark.parametrize("case", [cs.ATTN_CASES[0], cs.ATTN_CASES[3], cs.ATTN_CASES[6]], ids=lambda c: "x".join(map(str, c)))
def test_attention_maps_nonfinite_flag(case):
    """One inf, and one NaN, in one head of the last frame at patch n - 1 (n = 1, 65 and 257: the last patch belongs to thread 0 of
    the first trip, to thread 64 and to thread 0 of the second trip) sets the flag; a flag that was 1 stays 1 on finite input."""
    h, w, heads, frames, tc, diff = case
    n = (h // 8) * (w // 8)
    out, ws = guarded(frames * h * w), poisoned(frames * (n + 1))
    for bad in (float("inf"), float("nan")):
        att = cs.attn_input(case).copy()
        att[frames - 1, heads - 1, n - 1] = bad
        a = dev(att)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        _call("maavss_vit_attn_maps_checked", a.data_ptr(), out.data_ptr(), ws.data_ptr(), frames, heads, h, w, tc, diff, flag.data_ptr(), _st())
        assert int(flag.item()) == 1, (case, bad)
        flag.zero_()
        small, fmax = guarded(frames * n), guarded(frames)
        _call("maavss_vit_attn_maps_pass1", a.data_ptr(), small.data_ptr(), fmax.data_ptr(), frames, heads, n, flag.data_ptr(), _st())
        assert int(flag.item()) == 1, (case, bad)
    a = dev(cs.attn_input(case))
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    _call("maavss_vit_attn_maps_checked", a.data_ptr(), out.data_ptr(), ws.data_ptr(), frames, heads, h, w, tc, diff, flag.data_ptr(), _st())
    assert int(flag.item()) == 1
    assert_bits(out[:frames * h * w], cs.attn_want(case)[0], f"attn_maps after the flag runs {case}")


# ------------------------------------------------------------------------------------------------ 2. patchify
@pytest.mark.parametrize("dtype", [0, 2], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", cs.PATCHIFY_CASES, ids=lambda c: "x".join(map(str, c)))
def test_patchify_bit_for_bit(case, dtype):
    """F.unfold of the top-left 8hp x 8wp region rounded to nearest even, zeros in the CLS row, at H % 8 = 4 and 7 and W % 8 = 4;
    frame 0 carries +-0, bf16 and f16 ties with even and odd lower neighbours, f16 subnormals and 70000 (inf in f16)."""
    frames, h, w = case
    x = cs.patchify_input(case)
    want = vref.patchify_ref(x, dtype)
    rows = want.shape[0]
    a = torch.full((rows + 4, 192), 0x7777, dtype=torch.int16, device="cuda")
    xc = x.cuda()
    _call("maavss_vit_patchify", xc.data_ptr(), a.data_ptr(), frames, h, w, dtype, _st())
    got = a.cpu()
    assert torch.equal(got[:rows], want.view(torch.int16)), f"patchify {case} dtype {dtype}"
    assert bool((got[rows:] == 0x7777).all())
    sp = got[1, :8].tolist() + got[1, 8:16].tolist()             # first patch, channel 0, rows 0 and 1
    ref = torch.tensor(cs.PATCHIFY_SPECIALS_F16 if dtype == 2 else cs.PATCHIFY_SPECIALS_BF16)
    assert sp == ref.to(torch.float16 if dtype == 2 else torch.bfloat16).view(torch.int16).tolist()


# ------------------------------------------------------------------------------------------------ 3. window kernels
@pytest.mark.parametrize("frame_elems,clip_frames", cs.CLIP_SCALE_CASES)
def test_clip_scale_bit_for_bit(frame_elems, clip_frames):
    """fmax, raw-map and attn_diff modes; clip starts in front of the recording, at frame 0, at the last valid frame and behind it."""
    n_frames = cs.CLIP_SCALE_FRAMES
    start = cs.clip_starts(n_frames, clip_frames)
    maps = cs.rand((n_frames, frame_elems), "clip_scale", frame_elems, clip_frames).numpy()
    fmax = (cs.rand((n_frames,), "clip_scale_fmax", frame_elems, clip_frames) + 0.5).numpy()
    m, f, s = dev(maps), dev(fmax), dev(start)
    for mode in ("fmax", "maps", "diff"):
        rcp = guarded(len(start))
        _call("maavss_av_clip_scale", m.data_ptr(), f.data_ptr() if mode == "fmax" else None, s.data_ptr(), len(start), n_frames, clip_frames,
              frame_elems, int(mode == "diff"), rcp.data_ptr(), _st())
        want = vref.clip_scale(maps, fmax if mode == "fmax" else None, start, clip_frames, mode == "diff")
        assert_bits(rcp[:len(start)], want, f"clip_scale E {frame_elems} T {clip_frames} {mode}")
        assert guard_intact(rcp, len(start))


def _attn_windows(name, diff):
    p = cs.attn_win_problem(name, diff)
    h, w, up, n_frames, tc, num_seq, win, w0, n_win = p["case"]
    e = p["maps"].shape[1]
    # one allocation: a NaN-filled frame in front of the maps, so that a read in front of frame 0 shows
    buf = torch.full(((n_frames + 1) * e,), float("nan"), device="cuda")
    buf[e:] = dev(p["maps"]).reshape(-1)
    maps = buf[e:]
    rcp, start = dev(p["rcp"]), dev(p["clip_start"])
    numel = n_win * win * h * w
    out = guarded(numel)
    _call("maavss_av_attn_windows", maps.data_ptr(), rcp.data_ptr(), start.data_ptr(), len(p["clip_start"]), n_frames, tc, num_seq, win, w0,
          n_win, h, w, up, diff, out.data_ptr(), _st())
    assert_bits(out[:numel], p["want"], f"attn_windows {name} diff {diff}")
    assert guard_intact(out, numel)


@pytest.mark.parametrize("diff", [0, 1])
@pytest.mark.parametrize("name", list(cs.ATTN_WIN_CASES))
def test_attn_windows_bit_for_bit(name, diff):
    """upsample on (44 x 28: both remainders 4; 64 x 64) and off (8 x 12, 64 x 64), attn_diff on and off, the four clip starts (the clip at
    recording frame 0 with k = 0 sits behind a NaN-filled frame of the same allocation), num_seq - 1 + win_frames == clip_frames,
    num_seq = 1, win_frames = 1, w0 > 0 with the batch ending inside a clip."""
    _attn_windows(name, diff)


def test_attn_windows_grid_stride_wrap():
    """205 windows of 5 frames at 128 x 128: the 16384 blocks take a second, ragged trip."""
    _attn_windows("wrap", 1)


@pytest.mark.parametrize("name", list(cs.STFT_WIN_CASES))
def test_stft_windows_bit_for_bit(name):
    """float4 path ((a, F) = (8, 129), (4, 5)), scalar path ((3, 5), (1, 129)), w0 > 0, one grid-stride wrap per instantiation, and
    clip_rows = 89 with F = 129, a = 8: a F is a multiple of 4 but the planes of y start at odd multiples of 4 bytes, so the entry
    point must take the scalar kernel (before the fix it issued misaligned float4 loads)."""
    a, f, rows, n_clips, num_seq, win, w0, n_win = cs.STFT_WIN_CASES[name]
    y = cs.randn((n_clips, 2, rows, f), "stft_win", name)
    want = vref.stft_windows(y.numpy(), a, num_seq, win, w0, n_win)
    numel = want.size
    out, yc = guarded(numel), y.cuda()
    _call("maavss_av_stft_windows", yc.data_ptr(), n_clips, rows, f, a, num_seq, win, w0, n_win, out.data_ptr(), _st())
    assert_bits(out[:numel], want, f"stft_windows {name}")
    assert guard_intact(out, numel)


@pytest.mark.parametrize("use_absmax", [False, True])
@pytest.mark.parametrize("name", list(cs.STITCH_CASES))
def test_stitch_bit_for_bit(name, use_absmax):
    """float4 and scalar instantiations with and without clip_absmax (g = absmax + 1e-7 in float32, then one product), w0 > 0: the rows
    of `out` in front of and behind the batch keep their sentinel; one grid-stride wrap per instantiation."""
    a, f, n_clips, num_seq, w0, n_win = cs.STITCH_CASES[name]
    pred = cs.randn((n_win, 2, a, f), "stitch", name)
    amax = (cs.rand((n_clips,), "stitch_amax", name) + 0.5)
    numel = 2 * a * n_clips * num_seq * f
    want = np.full((2, a * n_clips * num_seq, f), SENTINEL, np.float32)
    vref.stitch(pred.numpy(), amax.numpy() if use_absmax else None, n_clips, num_seq, w0, want)
    out, pc, ac = guarded(numel), pred.cuda(), amax.cuda()
    _call("maavss_av_stitch", pc.data_ptr(), ac.data_ptr() if use_absmax else None, n_clips, num_seq, a, f, w0, n_win, out.data_ptr(), _st())
    assert_bits(out[:numel], want, f"stitch {name} absmax {use_absmax}")
    assert guard_intact(out, numel)


# ------------------------------------------------------------------------------------------------ 4. video transform
def _video_transform(video, boxes, cf, S, aa, ac):
    from maavss_amd import _lib
    f, h0, w0, _ = video.shape
    nbytes = _lib.query("maavss_video_transform_ws_bytes", f, cf, h0, w0, S, int(aa), int(ac))
    assert nbytes > 0
    ws = torch.full(((nbytes + 7) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    hb = torch.tensor(boxes, dtype=torch.int32)
    db, src = hb.cuda(), dev(video)
    numel = f * 3 * S * S
    out = guarded(numel)
    _call("maavss_video_transform", src.data_ptr(), db.data_ptr(), hb.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, f, cf, h0, w0, S,
          *cs.VT_MEAN, *cs.VT_STD, int(aa), int(ac), _st())
    assert guard_intact(out, numel)
    return out[:numel].cpu().view(f, 3, S, S)


@pytest.mark.parametrize("S,clip_frames", cs.VT_CASES)
def test_video_transform_within_derived_bound(S, clip_frames):
    """37 x 53 source, S = 8, 12, 20 and 68 (one full 64-column block and 4 columns, four 16-row blocks and 4 rows: ox < S and oy >= S
    both false somewhere, blocks mostly empty), boxes: full frame, one pixel, one row, one column, 2 x 3, 33 x 47; antialias x
    autocontrast.  Reference: the float32 tap tables as torch derives them, summed in float64 (horizontal first), the entry
    point's float32 a_c, b_c, autocontrast from the twin's own minimum and maximum.  Every element must be within
    u (x taps + y taps + 2) sum|w_y||w_x| p a_c + 1 ulp, propagated through (v - lo) * scale with autocontrast.  The one-pixel box
    gives constant planes, which autocontrast must pass on as clamp(v, 0, 1) exactly (scale = 1, min = 0).
    Before the bilinear tables folded the two taps that the gather clamps onto the last pixel into one tap of weight 1, the one-pixel
    box failed here at S = 20 (plain bilinear): (1 - l1) + l1 is 1 only within 2^-24, the planes were not constant, and autocontrast
    stretched the rounding noise to [0, 1].
    Measured on MI355X, worst |got - want| / bound over antialias x autocontrast: S = 8: 0.17 (clips of 1 frame) / 0.32 (of 2),
    12: 0.38 / 0.35, 20: 0.34 / 0.34, 68: 0.41 / 0.47; largest |got - want| 5.4e-7."""
    video, boxes = cs.vt_video(), cs.vt_boxes(clip_frames)
    worst = 0.0
    got_plain = {}
    for aa in (False, True):
        for ac in (False, True):
            want, bound = cs.vt_want(S, clip_frames, aa, ac)
            got = _video_transform(video, boxes, clip_frames, S, aa, ac)
            assert bool(torch.isfinite(got).all())
            if not ac:
                got_plain[aa] = got
            ratio = np.abs(got.double().numpy() - want) / bound
            print(f"[video transform] S {S} clip_frames {clip_frames} antialias {int(aa)} autocontrast {int(ac)}: "
                  f"worst |got - want| / bound {ratio.max():.3f}, max |got - want| {np.abs(got.double().numpy() - want).max():.2e}", flush=True)
            worst = max(worst, float(ratio.max()))
            if clip_frames == 1:                       # clip 1 is the one-pixel box
                plane = got_plain[aa][1]
                assert bool((plane == plane[:, :1, :1]).all()), f"S {S} antialias {aa}: the resize of one pixel is not constant"
                if ac:
                    assert torch.equal(got[1], plane.clamp(0, 1)), f"S {S} antialias {aa}: constant planes must take scale = 1, min = 0"
            assert ratio.max() <= 1.0, (S, clip_frames, aa, ac, float(ratio.max()))
    print(f"[video transform] S {S} clip_frames {clip_frames}: worst ratio {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 5. phasegram
def _phasegram(case, diff, cum, norm):
    b, t, p = case
    frames = cs.phase_frames(case)
    z, und = cs.phase_spectrum(case)
    ref = cs.phase_ref(case, diff, cum, norm)
    degenerate = t == 1 and diff                   # the zero row alone; NaN with normalize (see cases.phase_ref)
    bound = torch.zeros_like(ref) if degenerate else vref.phasegram_bound(z, cs.phase_delta(case), diff, cum, norm, ref)
    left = vref.phasegram_left_out(und, diff, cum)
    assert float(left.any(-1).float().mean()) <= cs.UNDECIDED_MAX_SHARE
    numel = b * t * p * p
    out, ws, amax, fc = guarded(numel), poisoned(numel), poisoned(1), frames.cuda()
    _call("maavss_video_phasegram", fc.data_ptr(), b, t, p, diff, cum, norm, ws.data_ptr(), amax.data_ptr(), out.data_ptr(), _st())
    assert guard_intact(out, numel)
    got = out[:numel].cpu().double().view(b, t, p * p)
    if degenerate:
        assert bool(torch.isnan(got).all() if norm else (got == 0).all()), (case, diff, cum, norm)
        return
    assert bool(torch.isfinite(got).all())
    ratio = ((got - ref).abs() / bound.clamp_min(1e-300))[~left]
    print(f"[phasegram] {case} diff {diff} cumulative {cum} normalize {norm}: worst |got - ref| / bound {float(ratio.max()):.3f}, "
          f"max |got - ref| {float((got - ref).abs()[~left].max()):.2e}, left out {int(left.any(-1).sum())} of {b * t} frames", flush=True)
    if diff:
        assert bool((got[:, 0] == 0).all())
    assert float(ratio.max()) <= 1.0, (case, diff, cum, norm, float(ratio.max()))


@pytest.mark.parametrize("case", cs.PHASE_SMALL, ids=lambda c: "x".join(map(str, c)))
def test_phasegram_within_derived_bound(case):
    """(B, T, P) = (1, 1, 32), (3, 5, 32), (2, 3, 64), (5, 4, 64): the all-axes fftshift at odd B and T and at T = 1, all eight
    diff / cumulative / normalize combinations, against video_phasegram_ref on the float64 copy of the frames.  delta (the
    allowance on the kernel's spectrum) is 4 x the measured |fft2 float32 - fft2 float64| of the case (video_edges_cases.PHASE_NOISE:
    1.03e-5, 4.21e-5, 1.38e-4, 1.82e-4); no bin of these inputs is undecided, no frame is left out.  Per-element bound:
    oracle.video_edges_ref.phasegram_bound.  At T = 1 with `diff` the reference returns no frame at all; expected there is the zero row
    the kernel documents, NaN with `normalize` (0 * 1 / 0; see video_edges_cases.phase_ref).
    Measured on MI355X, worst |got - ref| / bound over the option sets: 0.13, 0.09, 0.11, 0.08 in the order of the cases (the
    non-cumulative sets; the cumulative ones stay below 0.02); largest |got - ref| 3.8e-6."""
    for diff, cum, norm in cs.PHASE_OPTIONS:
        _phasegram(case, diff, cum, norm)


@pytest.mark.parametrize("diff,cum,norm", cs.PHASE_WRAP_OPTIONS)
def test_phasegram_grid_stride_wrap(diff, cum, norm):
    """3 x 171 frames of 32 x 32 (513 frames = 2052 blocks' worth): the diff and scale kernels' 2048 blocks take a second trip.
    delta = 4 x 6.26e-5; seed 80 has no undecided bin, no frame is left out.  Measured on MI355X: 0.003 of the bound with
    (diff, cumulative, normalize) = (1, 1, 1), 0.034 with (0, 0, 1)."""
    _phasegram(cs.PHASE_WRAP, diff, cum, norm)
