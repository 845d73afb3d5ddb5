"""Shapes and inputs shared by test_conv3d_edges_cpu.py (which checks the references and the exactness conditions) and
test_conv3d_edges_gpu.py (which holds the HIP kernels to them).  Tensors are in the reference layout (NCDHW); the float64
references are computed once per case and reused by every test that needs them."""
import functools

import torch

from oracle import conv3d_ref as cref

# ------------------------------------------------------------------------------------------------ 1. implicit GEMM
# name: (B, T, H, W, pad)
IGEMM_SHAPES = {
    "a": (1, 1, 5, 5, 0),        # 1 x 1 output; its input gradient is pad 4 from a 1 x 1 image
    "b": (3, 1, 15, 9, 2),       # 16-row tile with one row below the image; T = 1 with three clips
    "c": (1, 2, 30, 17, 2),      # 16-row tiles, last tile row 14 rows, last tile column one column; exactly 8 tiles
    "d": (1, 3, 17, 33, 2),      # 14-row tiles, second tile 3 rows; 18 tiles in a 24-block grid
    "e": (1, 1, 20, 20, 1),      # pad 1 forward, pad 3 input gradient
    "f": (1, 2, 34, 21, 0),      # pad 0 forward; input gradient pad 4 onto 34 x 21
    "g": (1, 2, 42, 8, 2),       # three full 14-row tiles
    "h": (2, 2, 10, 10, 3),      # the fifth layer's pad
}
IGEMM_OUT = {"a": (1, 1), "b": (15, 9), "c": (30, 17), "d": (17, 33), "e": (18, 18), "f": (30, 17), "g": (42, 8), "h": (12, 12)}
IGEMM_TILES = {"a": 1, "b": 3, "c": 8, "d": 18, "e": 4, "f": 8, "g": 6, "h": 4}      # counted by hand from the table above
PAIRS = ((16, 32), (32, 64), (64, 64), (64, 16), (32, 16), (64, 32), (16, 64))      # every instantiated (C_in, C_out)
MODEL_PAIRS = PAIRS[:4]                                                             # the four model layers (dgrad, wgrad)
REAL_SHAPE = "c"

# ------------------------------------------------------------------------------------------------ 2. weight gradient
WGRAD_SHAPES = {
    "one": (1, 1, 5, 5, 0),          # one position, one tile
    "h15": (1, 3, 15, 20, 2),        # 16-row tile with a missing row; last tile column 4 wide
    "t12": (1, 2, 20, 40, 2),        # 14-row tiles, the second with 6 rows; last tile column exactly 8 wide; 12 tiles
    "w9": (1, 1, 28, 25, 2),         # last tile column 9 wide; full 14-row tiles
    "t11": (1, 11, 8, 8, 2),         # 11 tiles, one per frame: the default nchunk leaves an empty last chunk
}
WGRAD_TILES = {"one": 1, "h15": 6, "t12": 12, "w9": 4, "t11": 11}
WGRAD_NCHUNK = {"one": (None, 9), "h15": (None,), "t12": (None, 1, 5, 12, 17), "w9": (None,), "t11": (None,)}
WGRAD_REAL_SHAPE = "t12"

# ------------------------------------------------------------------------------------------------ 3. first layer
C1_SHAPES = ((1, 1, 3, 2), (1, 3, 16, 16), (2, 2, 31, 15), (3, 1, 17, 33))      # (B, T, H, W)
C1_BN_CASES = ((2, 2, 31, 15, 2), (1, 3, 17, 33, 2), (1, 2, 17, 22, 3))         # (B, T, H, W, pool)
UNDECIDED_MAX_SHARE = 0.01


def ints(shape, lo, hi, seed):
    """integers lo..hi (inclusive) as float32"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=torch.Generator().manual_seed(seed)).float()


def randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def to_cl(x):      # NCDHW -> channels-last [B,T,H,W,C]
    return x.permute(0, 2, 3, 4, 1).contiguous()


def from_cl(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def _seed(*key):
    """one seed per (case, tensor): no two tensors of the suite share their data"""
    return sum(ord(ch) * (31 ** i) for i, ch in enumerate(repr(key))) % (2 ** 31 - 1)


@functools.lru_cache(maxsize=None)
def conv_case(family, name, ci, co):
    """Integer case of the implicit GEMM ('igemm') or the weight gradient ('wgrad'): x in -2..2, w in -1..1, dy in -2..2 and the
    float64 y, input gradient gx and weight gradient gw."""
    b, t, h, w, pad = (IGEMM_SHAPES if family == "igemm" else WGRAD_SHAPES)[name]
    x = ints((b, ci, t, h, w), -2, 2, _seed(family, name, ci, co, "x"))
    wgt = ints((co, ci, 3, 5, 5), -1, 1, _seed(family, name, ci, co, "w"))
    y = cref.conv3d_f64(x, wgt, pad)
    dy = ints(y.shape, -2, 2, _seed(family, name, ci, co, "dy"))
    gx, gw = cref.conv3d_grads_f64(x, wgt, dy, pad)
    prior = ints(wgt.shape, -3, 3, _seed(family, name, ci, co, "prior"))      # the accumulate form's dw
    return dict(x=x, w=wgt, dy=dy, y=y, gx=gx, gw=gw, prior=prior, pad=pad, dims=(b, t, h, w))


def rounded(x, mode):
    """what the MFMA mode does to an operand: 1 = f32 (nothing), 0 = bf16, 2 = IEEE half"""
    return x if mode == 1 else x.to(torch.float16 if mode == 2 else torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def real_case(family, name, ci, co, mode):
    """randn operands rounded the way `mode` rounds them, and the float64 results from those."""
    b, t, h, w, pad = (IGEMM_SHAPES if family == "igemm" else WGRAD_SHAPES)[name]
    x = randn((b, ci, t, h, w), _seed(family, name, ci, co, "rx"))
    wgt = randn((co, ci, 3, 5, 5), _seed(family, name, ci, co, "rw"), (ci * 75) ** -0.5)
    xr, wr = rounded(x, mode), rounded(wgt, mode)
    y = cref.conv3d_f64(xr, wr, pad)
    dy = randn(y.shape, _seed(family, name, ci, co, "rdy"))
    gx, gw = cref.conv3d_grads_f64(xr, wr, rounded(dy, mode), pad)
    return dict(x=x, w=wgt, dy=dy, y=y, gx=gx, gw=gw, pad=pad)


@functools.lru_cache(maxsize=None)
def c1_case(b, t, h, w):
    """Integer case of the first layer: x in 0..3 (an image), w in -1..1, dy in -2..2; tensors as the kernels take them
    (x [B,T,H,W], y / dy channels-last)."""
    x = ints((b, t, h, w), 0, 3, _seed("c1", b, t, h, w, "x"))
    wgt = ints((16, 1, 3, 5, 5), -1, 1, _seed("c1", b, t, h, w, "w"))
    y = cref.conv3d_f64(x[:, None], wgt, 2)
    dy = ints(y.shape, -2, 2, _seed("c1", b, t, h, w, "dy"))
    _, gw = cref.conv3d_grads_f64(x[:, None], wgt, dy, 2)
    prior = ints(wgt.shape, -3, 3, _seed("c1", b, t, h, w, "prior"))
    return dict(x=x, w=wgt, dy=to_cl(dy), y=to_cl(y), y_ncdhw=y, dy_ncdhw=dy, gw=gw, prior=prior)


def c1_bn_inputs(b, t, h, w, pool):
    """Real-valued inputs of the fused BatchNorm weight gradient, as test_conv3d_c1_wgrad_bn_mfma_matches_the_f32_kernel builds them."""
    x = torch.rand(b, t, h, w, generator=torch.Generator().manual_seed(_seed("bn", b, t, h, w, "x")))
    wgt = randn((16, 1, 3, 5, 5), _seed("bn", b, t, h, w, "w"), 0.1)
    gamma = 1 + 0.3 * randn((16,), _seed("bn", b, t, h, w, "gamma"))
    beta = 0.2 * randn((16,), _seed("bn", b, t, h, w, "beta"))
    dout = randn((b, t, h // pool, w // pool, 16), _seed("bn", b, t, h, w, "dout"))
    return x, wgt, gamma, beta, dout
