"""Shapes and inputs shared by tests/test_f32_edges_cpu.py (which shows the float64 references and the derived bounds are
sound on exactly these inputs) and tests/test_f32_edges_gpu.py (which holds the HIP kernels to them)."""
import torch
import torch.nn.functional as F

from oracle import stft_ref_cpu as sref

FFTS = (256, 512, 1024)
HOP = 66                                   # calc_hop_size(., 8, 30, 16000)

# (batch, n_frames): odd n_frames with an even total (pairs straddle clips 0|1 and 2|3), an odd total (the last pair holds
# one frame), a single frame alone in its pair
STFT_ODD = ((4, 7), (3, 5), (1, 1))
STFT_WRAP = (131, 127)                     # 16 637 frames = 8 319 pairs > 2048 workgroups x 4 pairs: the grid-stride loop wraps


def stft_hop(fft_len, n_frames):
    """66 (100 at 1024 points), except for the single frame: every clip must be longer than n_fft / 2 for the reflection."""
    if n_frames == 1:
        return fft_len // 2 + HOP
    return HOP if fft_len < 1024 else 100


def stft_length(fft_len, n_frames):
    return n_frames * stft_hop(fft_len, n_frames) + 13          # not a multiple of the hop


def loud_audio(batch, length, seed):
    """synthetic_audio with clip b scaled by 0.2 + 0.3 (b mod 4): neighbouring clips differ clearly in loudness (a per-clip
    maximum credited to the wrong clip is off by 30 % or more), and the loudest clip (x 1.1) keeps the spectrum within
    what plain synthetic_audio gives, the input test_stft_matches_oracle states the kernel's 5e-6 for: max|y| 1.6 / 2.0 /
    2.7 here against 1.5 / 1.9 / 2.8 there at 256 / 512 / 1024 points (the sinusoids' bins; the window sums to ~10 x its
    norm)."""
    scale = 0.2 + 0.3 * (torch.arange(batch) % 4).float()
    return sref.synthetic_audio(batch, length, seed) * scale[:, None]


def noise_like(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def stft_max_frames(fft_len):
    """(length, hop, n_frames): a short clip and the largest frame count the entry point admits for it; the last sample of
    the last frame reflects exactly onto index 0 ((n_frames - 1) hop + n_fft / 2 - 1 == 2 (length - 1))."""
    length = fft_len // 2 + 69
    hop = {256: 53, 512: 131, 1024: 59}[fft_len]
    span = 2 * length - 1 - fft_len // 2
    assert span % hop == 0
    return length, hop, span // hop + 1


def istft_hops(fft_len):
    """(hop, frames): every regime of the overlap-add bounds -- all frames cover every sample (1), the benched 66, an odd
    hop just above n_fft / 8, exactly two / fewer than two frames per sample, and no overlap at all."""
    return ((1, 9), (66, 7), (133, 7), (fft_len // 2, 7), (fft_len // 2 + 1, 7), (fft_len - 1, 7), (fft_len, 7))


ISTFT_IDLE = ((1, 3), (3, 5), (1, 2))      # (batch, frames): totals 3, 15, 2 leave idle waves in a 4- (2-) frame workgroup

LSTM_CASES = ((1, 1), (1, 16), (31, 3), (32, 2), (33, 5), (64, 1), (65, 2))      # (batch, L); the kernels' batch slab is 32
LSTM_IN = 64


def lstm_problem(b, l, dtype=torch.float64):
    """-> (module, x [b, l, 64], dout [b, l, 512]) in `dtype`, seeded."""
    torch.manual_seed(100 * b + l)
    lstm = torch.nn.LSTM(LSTM_IN, 256, 1, bias=False, batch_first=True, bidirectional=True).to(dtype)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(b, l, LSTM_IN, generator=g).to(dtype)
    dout = torch.randn(b, l, 512, generator=g).to(dtype)
    return lstm, x, dout


# (B, H, W, C, Ho, Wo): overlapping windows, identity, global, the STFT encoder's kind of map
POOL_SHAPES = ((2, 7, 13, 5, 3, 4), (1, 9, 9, 3, 9, 9), (2, 6, 10, 4, 1, 1), (1, 33, 257, 16, 4, 16))


def pool_problem(shape):
    """-> x [B, C, H, W], dout [B, C, Ho, Wo] (float32, NCHW views for torch; the kernel takes NHWC)."""
    b, h, w, c, ho, wo = shape
    return noise_like((b, c, h, w), 3) + 0.5, noise_like((b, c, ho, wo), 4) + 0.5


# (rows, C, layout): layout "rows" = contiguous [rows][C], "pad" = row stride C + 3, "nchw" = [C][rows] (row stride 1)
CSUM_CASES = tuple((r, c, "rows") for r, c in ((1, 3), (255, 4), (256, 1), (257, 7), (5000, 33))) + ((257, 7, "pad"), (257, 7, "nchw"))


def csum_problem(rows, c):
    """-> x [rows, C] uniform in [0.75, 1.25) and a prior out [C].  Every row moves a sum by >= 0.75, far above the bound
    (~rows^2 2^-24) up to a few hundred rows; at 5000 rows the worst-case bound itself reaches 1.5, which is what
    csum_integers is for."""
    g = torch.Generator().manual_seed(5)
    return 0.75 + 0.5 * torch.rand(rows, c, generator=g), torch.randn(c, generator=g) * 10


def csum_integers(rows, c):
    """Integer-valued x in [-8, 8] and prior: every partial sum in any order is an integer below 2^24, hence exact in
    float32, so the kernel's result must EQUAL the float64 sum -- one dropped, doubled or misaddressed element shows."""
    g = torch.Generator().manual_seed(8)
    return (torch.randint(-8, 9, (rows, c), generator=g).float() + (torch.arange(c) % 3).float(),
            torch.randint(-100, 101, (c,), generator=g).float())


def pool_ref(x, dout, ho, wo):
    """float64 torch: (out, dx)."""
    x64 = x.double().requires_grad_(True)
    out = F.adaptive_avg_pool2d(x64, (ho, wo))
    dx, = torch.autograd.grad(out, x64, dout.double())
    return out.detach(), dx
