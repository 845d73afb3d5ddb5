"""Shapes, seeds and inputs shared by tests/test_video_edges_cpu.py (which checks the twins of oracle/video_edges_ref.py, the
exactness conditions and the caps on exactly these inputs) and tests/test_video_edges_gpu.py (which holds the HIP kernels to them).
One seed per (case, tensor); references are computed once per case and reused."""
import functools

import numpy as np
import torch

from conv3d_edges_cases import UNDECIDED_MAX_SHARE, _seed      # noqa: F401  (the share is re-exported)
from oracle import avfm_ref_cpu as aref
from oracle import video_edges_ref as vref


def _gen(*key):
    return torch.Generator().manual_seed(_seed("video_edges", *key))


def rand(shape, *key):
    return torch.rand(*shape, generator=_gen(*key))


def randn(shape, *key):
    return torch.randn(*shape, generator=_gen(*key))


# ------------------------------------------------------------------------------------------------ 1. attention maps
# (H, W, heads, frames, clip_frames, attn_diff)
ATTN_CASES = (
    (8, 8, 1, 1, 0, 0),           # n = 1, one head, no clip normalisation
    (64, 64, 6, 2, 2, 0),         # n = 64, exactly one wave
    (72, 60, 12, 3, 3, 1),        # n = 63, W % 8 = 4, 12 heads
    (44, 104, 6, 4, 2, 1),        # n = 65, H % 8 = 4
    (120, 136, 6, 2, 1, 0),       # n = 255, clips of one frame
    (128, 128, 6, 2, 2, 0),       # n = 256, clips of two frames
    (12, 2060, 6, 2, 1, 0),       # n = 257 as 1 x 257, H % 8 and W % 8 both 4
    (224, 224, 6, 1, 1, 0),       # n = 784, four trips of the j += 256 loops
    (128, 128, 6, 1025, 5, 0),    # pass 2: 4 198 400 float4 > 16384 x 256, a ragged second trip
)
ATTN_WRAP = ATTN_CASES[-1]


@functools.lru_cache(maxsize=None)
def attn_input(case):
    """att [frames, heads, n] float32 numpy: positive rows that sum to 1 over n, as a softmax row does."""
    h, w, heads, frames, _, _ = case
    n = (h // 8) * (w // 8)
    att = rand((frames, heads, n), "att", case) + 1e-3
    return (att / att.sum(-1, keepdim=True)).numpy()


@functools.lru_cache(maxsize=None)
def attn_want(case):
    h, w, _, _, clip_frames, attn_diff = case
    return vref.attn_maps(attn_input(case), h, w, clip_frames, attn_diff)


# ------------------------------------------------------------------------------------------------ 2. patchify
PATCHIFY_CASES = ((1, 8, 8), (2, 44, 28), (3, 15, 12))      # (frames, H, W): one patch; H % 8 = W % 8 = 4; H % 8 = 7, one column
# first patch of frame 0, channel 0, row-major.  bf16 keeps 8 significant bits, f16 11: a value 1 + 2^-8 (1 + 2^-11) lies halfway
# between two bf16 (f16) neighbours with an even lower one, 1 + 2^-7 + 2^-8 (1 + 2^-10 + 2^-11) with an odd lower one.
PATCHIFY_SPECIALS = (
    0.0, -0.0,
    1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 2.0 ** -7 + 2.0 ** -8),
    1 + 2.0 ** -11, 1 + 2.0 ** -10 + 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 2.0 ** -10 + 2.0 ** -11),
    2.0 ** -15, -(2.0 ** -15), 1.5 * 2.0 ** -24, -1.5 * 2.0 ** -24,       # f16 subnormals; the second a tie 2^-24 | 2^-23
    70000.0, -70000.0,                                                      # inf in f16
)
# what the IEEE rule (nearest, ties to even) makes of them
PATCHIFY_SPECIALS_BF16 = (
    0.0, -0.0, 1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6),
    1.0, 1.0, -1.0, -1.0,                              # both f16 ties lie below the bf16 midpoint 1 + 2^-8
    2.0 ** -15, -(2.0 ** -15), 1.5 * 2.0 ** -24, -1.5 * 2.0 ** -24,
    70144.0, -70144.0,
)
PATCHIFY_SPECIALS_F16 = (
    0.0, -0.0, 1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 2.0 ** -7 + 2.0 ** -8),
    1.0, 1 + 2.0 ** -9, -1.0, -(1 + 2.0 ** -9),
    2.0 ** -15, -(2.0 ** -15), 2.0 ** -23, -(2.0 ** -23),
    float("inf"), float("-inf"),
)


def patchify_input(case):
    frames, h, w = case
    x = randn((frames, 3, h, w), "patchify", case)
    x[0, 0, :2, :8] = torch.tensor(PATCHIFY_SPECIALS, dtype=torch.float32).view(2, 8)
    return x


# ------------------------------------------------------------------------------------------------ 3. window kernels
def clip_starts(n_frames, clip_frames):
    """in front of the recording, its first frame, the last valid start, behind the recording"""
    return np.array([-3, 0, n_frames - clip_frames, n_frames - clip_frames + 4], np.int32)


CLIP_SCALE_FRAMES = 9
CLIP_SCALE_CASES = tuple((e, t) for e in (1, 255, 257) for t in (2, 5))       # (frame_elems, clip_frames)

# name: (H, W, upsample, n_frames, clip_frames, num_seq, win_frames, w0, n_win); four clips each (clip_starts)
ATTN_WIN_CASES = {
    "up44x28": (44, 28, 1, 9, 5, 3, 3, 0, 12),       # H % 8 = W % 8 = 4; num_seq - 1 + win_frames == clip_frames; every window
    "up64x64": (64, 64, 1, 9, 5, 5, 1, 2, 5),        # win_frames = 1; w0 > 0, the batch ends inside clip 1
    "full8x12": (8, 12, 0, 6, 2, 1, 2, 0, 4),        # num_seq = 1; W % 8 = 4
    "full64x64": (64, 64, 0, 9, 5, 3, 3, 4, 6),      # w0 inside clip 1, ends inside clip 3
}
# 205 windows x 5 frames x 128 x 32 float4 = 4 198 400 > 16384 x 256: a ragged second trip of the grid-stride loop
ATTN_WIN_WRAP = (128, 128, 1, 300, 5, 1, 5, 0, 205)


def attn_win_problem(name, attn_diff):
    """-> dict(maps [n_frames, E], clip_start, rcp (the twin's clip scale of those maps), want)"""
    case = ATTN_WIN_WRAP if name == "wrap" else ATTN_WIN_CASES[name]
    h, w, up, n_frames, tc, num_seq, win, w0, n_win = case
    e = (h // 8) * (w // 8) if up else h * w
    maps = (rand((n_frames, e), "attn_win", name) + 0.05).numpy()
    if name == "wrap":
        n_clips = n_win // num_seq
        start = torch.randint(-3, n_frames - tc + 4, (n_clips,), generator=_gen("attn_win_start", name)).to(torch.int32).numpy()
        start[:4] = clip_starts(n_frames, tc)
    else:
        start = clip_starts(n_frames, tc)
    rcp = vref.clip_scale(maps, None, start, tc, attn_diff)
    want = vref.attn_windows(maps, rcp, start, tc, num_seq, win, w0, n_win, h, w, up, attn_diff)
    return dict(case=case, maps=maps, clip_start=start, rcp=rcp, want=want)


# name: (a, F, clip_rows, n_clips, num_seq, win_frames, w0, n_win)
STFT_WIN_CASES = {
    "vec8x129": (8, 129, 40, 3, 3, 3, 2, 6),
    "vec4x5": (4, 5, 16, 3, 2, 3, 0, 6),
    "scalar3x5": (3, 5, 15, 3, 3, 3, 2, 6),
    "scalar1x129": (1, 129, 5, 3, 3, 3, 0, 9),
    # a F = 1032 is a multiple of 4, clip_rows F = 89 x 129 is not: plane starts are not 16-byte aligned, so only the scalar kernel may run
    "rows89": (8, 129, 89, 3, 3, 3, 1, 7),
    # 1630 windows x 2 x 5160 / 4 = 4 205 400 float4 > 16384 x 256
    "wrap_vec": (8, 129, 112, 163, 10, 5, 0, 1630),
    # 3260 windows x 2 x 645 = 4 205 400 floats > 16384 x 256
    "wrap_scalar": (1, 129, 24, 163, 20, 5, 0, 3260),
}
STFT_WIN_VECTOR = {"vec8x129": True, "vec4x5": True, "scalar3x5": False, "scalar1x129": False, "rows89": False, "wrap_vec": True,
                   "wrap_scalar": False}

# name: (a, F, n_clips, num_seq, w0, n_win)
STITCH_CASES = {
    "vec8x129": (8, 129, 3, 3, 2, 5),
    "vec4x5": (4, 5, 3, 2, 1, 4),
    "scalar3x5": (3, 5, 3, 3, 2, 5),
    "scalar1x129": (1, 129, 3, 3, 1, 7),
    "wrap_vec": (8, 129, 813, 10, 0, 8130),          # 8130 x 2 x 1032 / 4 = 4 195 080 float4 > 16384 x 256
    "wrap_scalar": (1, 129, 1630, 10, 0, 16300),     # 16300 x 2 x 129 = 4 205 400 floats > 16384 x 256
}
GRID_CAP = 16384 * 256


def stft_win_items(name):
    a, f, _, _, _, win, _, n_win = STFT_WIN_CASES[name]
    return n_win * 2 * a * win * f // (4 if STFT_WIN_VECTOR[name] else 1)


def stitch_items(name):
    a, f, _, _, _, n_win = STITCH_CASES[name]
    return n_win * 2 * a * f // (4 if (a * f) % 4 == 0 else 1)


# ------------------------------------------------------------------------------------------------ 4. video transform
VT_SOURCE = (37, 53)
VT_FRAMES = 4
VT_SIZES = (8, 12, 20, 68)       # 68: one full 64-column block and 4 columns, four 16-row blocks and 4 rows
# (top, left, h, w): full frame, the last pixel, one row, one column, a tiny crop (upsampled), a general crop
VT_BOXES = ((0, 0, 37, 53), (36, 52, 1, 1), (0, 0, 1, 53), (5, 52, 32, 1), (17, 20, 2, 3), (3, 4, 33, 47))
VT_CASES = tuple((s, cf) for s in VT_SIZES for cf in (1, 2))
VT_MEAN = (0.485, 0.456, 0.406)
VT_STD = (0.229, 0.224, 0.225)


def vt_boxes(clip_frames):
    """four clips of one frame take the first four boxes, two clips of two frames the last two: every size runs every box"""
    return VT_BOXES[:4] if clip_frames == 1 else VT_BOXES[4:]


@functools.lru_cache(maxsize=None)
def vt_video():
    g = _gen("vt_video")
    return torch.randint(0, 256, (VT_FRAMES, VT_SOURCE[0], VT_SOURCE[1], 3), generator=g, dtype=torch.uint8).numpy()


@functools.lru_cache(maxsize=None)
def vt_want(S, clip_frames, antialias, autocontrast):
    return vref.video_transform(vt_video(), vt_boxes(clip_frames), clip_frames, S, VT_MEAN, VT_STD, antialias, autocontrast)


# ------------------------------------------------------------------------------------------------ 5. phasegram
PHASE_SMALL = ((1, 1, 32), (3, 5, 32), (2, 3, 64), (5, 4, 64))       # (B, T, P): all eight option combinations
PHASE_WRAP = (3, 171, 32)                                            # 513 frames: the diff and scale kernels' 2048 blocks wrap
PHASE_WRAP_OPTIONS = ((1, 1, 1), (0, 0, 1))                          # (diff, cumulative, normalize)
PHASE_OPTIONS = tuple((d, c, n) for d in (0, 1) for c in (0, 1) for n in (0, 1))
# seeds of torch.rand(B, T, P, P), found by a search on the CPU for inputs without an undecided bin (test_video_edges_cpu.py
# asserts that from the float64 reference alone), and per case the largest |fft2 float32 - fft2 float64| over the case's bins that
# torch (pocketfft) gave when the seeds were chosen.  delta, the allowance on the kernel's spectrum, is 4 x that: the kernel's
# radix-2 form with float32 twiddles has more stages than pocketfft's mixed radix.
PHASE_SEEDS = {(1, 1, 32): 0, (3, 5, 32): 0, (2, 3, 64): 0, (5, 4, 64): 0, (3, 171, 32): 80}
PHASE_NOISE = {(1, 1, 32): 1.03e-5, (3, 5, 32): 4.21e-5, (2, 3, 64): 1.38e-4, (5, 4, 64): 1.82e-4, (3, 171, 32): 6.26e-5}
PHASE_DELTA_FACTOR = 4.0


def phase_frames(case, seed=None):
    b, t, p = case
    return torch.rand(b, t, p, p, generator=torch.Generator().manual_seed(PHASE_SEEDS[case] if seed is None else seed))


def phase_noise(frames):
    """largest elementwise |fft2 in float32 - fft2 in float64| over the frames"""
    return float((torch.fft.fft2(frames).to(torch.complex128) - torch.fft.fft2(frames.double())).abs().max())


def phase_delta(case):
    return PHASE_DELTA_FACTOR * PHASE_NOISE[case]


@functools.lru_cache(maxsize=None)
def phase_spectrum(case):
    """(z in output coordinates, undecided-bin mask)"""
    z = vref.phasegram_spectrum(phase_frames(case))
    return z, vref.phasegram_undecided(z, phase_delta(case))


@functools.lru_cache(maxsize=None)
def phase_ref(case, diff, cumulative, normalize):
    """video_phasegram_ref on the float64 copy of the frames -> [B, T, P * P].  At T = 1 with `diff` the reference's torch.cat builds its
    zero row from an empty difference and returns no frame at all (and with `normalize` fails on the maximum of an empty tensor):
    expected there is the zero first row the kernel documents, and with `normalize` that row times 1 / 0 -- NaN in every element, as
    the reference's own `pg * (1 / max|pg|)` makes of a zero tensor."""
    b, t, p = case
    if t == 1 and diff:
        ref = torch.zeros(b, 1, p * p, dtype=torch.float64)
        return ref * (1.0 / ref.abs().max()) if normalize else ref
    return aref.video_phasegram_ref(phase_frames(case).double()[:, None], bool(diff), bool(cumulative), bool(normalize))[:, 0]
