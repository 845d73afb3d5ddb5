"""Shapes and inputs shared by test_bn_pool_edges_cpu.py (which checks the references and the exactness conditions) and
test_bn_pool_edges_gpu.py (which holds csrc/bn_pool.hip to them).  Tensors are channels-last [B,T,H,W,C], as the kernels take them.

Statistics: integer-valued inputs, so every partial sum a workgroup forms in float32 is an exact integer and the float64 reference
forms the same sums.  Pool: inputs on the grid of multiples of 1/8 in [-2, 2] with extra weight on both ends, so that the maximum
of a window is attained more than once in about a third of the 2 x 2 and most of the 3 x 3 windows (whichever sign gamma has): the
argmax rule -- first maximum in dy * P + dx order -- then decides where the gradient goes."""
import collections
import functools

import torch

from oracle import dense_edges_ref as dref

EPS, MOMENTUM = 1e-5, 0.1                     # ops.BN_EPS, ops.BN_MOMENTUM
LEAKY, TANH = 0, 1                            # ops.BN_LEAKY, ops.BN_TANH
MAX_ULP = 1                                   # statistics: equality, or one float32 ulp (a contraction of s2 / count - m * m in double)
OUT_TOL = (1e-5, 1e-5)                        # test_bn_pool_act's tolerances (rtol, atol): out
DY_TOL, DPARAM_TOL = (1e-4, 2e-5), (1e-4, 1e-4)      # ... dy; dgamma and dbeta
MIN_Z = 1e-4                                  # |pre-activation| stays above this: float32 and float64 agree on the side of LeakyReLU's kink

# ---------------------------------------------------------------------------------------------- statistics
# (rows, C): one row; less than one row phase set; one and two workgroups; three; the cap of 512 workgroups with a
# rows-per-workgroup count (1026) that is no multiple of the 256 row phases of C = 4
STATS_CASES = ((1, 4), (1, 64), (63, 16), (63, 4), (1024, 64), (1025, 4), (1025, 16), (2049, 16), (2049, 64), (525000, 4))
TWO_LEVEL_CASES = ((1300, 4), (1300, 64))     # (partial rows, C): bn_finalize's two-level reduction (nblk > 512)
TWO_LEVEL_COUNT = 1300 * 1024


def stats_nblk(rows):
    """maavss_bn_stats_nblk as include/maavss.h documents it: one workgroup per 1024 rows, at most 512"""
    return max(1, min(512, (rows + 1023) // 1024))


@functools.lru_cache(maxsize=None)
def stats_input(rows, c):
    """integers in [-4, 4] plus a per-channel offset in {0, 1, 2}; and prior running statistics"""
    gen = torch.Generator().manual_seed(100 + rows + c)
    y = torch.randint(-4, 5, (rows, c), generator=gen).float() + (torch.arange(c) % 3).float()
    rm0 = torch.randn(c, generator=gen) * 0.1
    rv0 = 1 + 0.1 * torch.randn(c, generator=gen).abs()
    return y, rm0, rv0


@functools.lru_cache(maxsize=None)
def two_level_partials(nblk, c):
    """synthetic integer partial sums [nblk][2][C]: totals below 2^24, variance positive at TWO_LEVEL_COUNT elements"""
    gen = torch.Generator().manual_seed(200 + c)
    s1 = torch.randint(-500, 501, (nblk, 1, c), generator=gen).float()
    s2 = torch.randint(4000, 12001, (nblk, 1, c), generator=gen).float()
    return torch.cat([s1, s2], 1).contiguous()


@functools.lru_cache(maxsize=None)
def stats_reference(rows, c):
    """float32 (mean, invstd, running_mean, running_var) rounded once from float64"""
    y, rm0, rv0 = stats_input(rows, c)
    s1, s2 = dref.bn_sums_f64(y)
    return tuple(t.float() for t in dref.bn_finalize_f64(s1, s2, float(rows), EPS, MOMENTUM, rm0, rv0))


@functools.lru_cache(maxsize=None)
def two_level_reference(nblk, c):
    part = two_level_partials(nblk, c).double()
    _, rm0, rv0 = stats_input(1, c)
    return tuple(t.float() for t in dref.bn_finalize_f64(part[:, 0].sum(0), part[:, 1].sum(0), float(TWO_LEVEL_COUNT), EPS, MOMENTUM, rm0, rv0))


# ---------------------------------------------------------------------------------------------- forward / backward
Pool = collections.namedtuple("Pool", "tag b t h w c pool act blocks")
POOL_CASES = (
    Pool("c4-p2-drop", 1, 2, 5, 7, 4, 2, LEAKY, False),        # C = 4: one thread owns a position; last row and column dropped
    Pool("c8-p3-fit", 2, 1, 6, 6, 8, 3, LEAKY, False),         # no remainder
    Pool("c64-p3-one", 1, 1, 3, 3, 64, 3, LEAKY, False),       # one window only
    Pool("c64-p3-drop", 2, 2, 7, 8, 64, 3, LEAKY, False),      # one row and two columns dropped
    Pool("c64-p2-drop", 1, 3, 11, 11, 64, 2, LEAKY, False),
    Pool("c8-p1-tanh", 1, 2, 9, 17, 8, 1, TANH, False),        # the STFT encoder's form: no pool
    Pool("c4-p1", 1, 1, 4, 4, 4, 1, LEAKY, False),
    Pool("c8-p2-blocks", 1, 1, 16, 24, 8, 2, LEAKY, True),     # constant 8 x 8 blocks: every window is one value four times
    Pool("c4-p2-wrap", 3, 11, 250, 6, 4, 2, LEAKY, False),     # 4125 pooled rows, 8250 input rows: both row walks wrap their 4096-block grids
)
POOL_IDS = [p.tag for p in POOL_CASES]
C4_CASE = POOL_CASES[0]
ROUTING_CASES = (POOL_CASES[7], POOL_CASES[3], POOL_CASES[0])      # exact routing of a single pooled gradient
# the layout of test_bn_pool_strided_output: the pooled tensor is the [B, C, T * S] block of a [B, C, 2 * T * S] sequence buffer
STRIDED = Pool("strided", 2, 4, 6, 6, 16, 3, LEAKY, False)


def grid_values():
    return torch.arange(-16, 17).float() / 8


@functools.lru_cache(maxsize=None)
def pool_input(p, small_gamma=False, batch_stats=False):
    """dict of float32 CPU tensors: y, mean, invstd, gamma, beta, dout.  mean / invstd are arbitrary given values, or (batch_stats)
    the batch's own statistics rounded from float64, as the backward formula assumes.  small_gamma: channel 1 below 1e-2."""
    gen = torch.Generator().manual_seed(300 + 17 * p.h + p.w + p.c + 5 * p.pool)
    shape = (p.b, p.t, p.h, p.w, p.c)
    if p.blocks:
        coarse = torch.randint(-40, 41, (p.b, p.t, p.h // 8, p.w // 8, p.c), generator=gen)
        y = coarse.repeat_interleave(8, 2).repeat_interleave(8, 3)
    else:
        y = torch.randint(-40, 41, shape, generator=gen)
    y = (y.float() / 8).clamp(-2, 2)
    sign = torch.where(torch.rand(p.c, generator=gen) < 0.5, -1.0, 1.0)
    sign[0], sign[p.c - 1] = 1.0, -1.0                                     # both signs in every case
    gamma = sign * (0.5 + torch.rand(p.c, generator=gen))
    beta = 0.2 * torch.randn(p.c, generator=gen)
    if small_gamma:
        gamma[1], beta[1] = -3e-3, 0.25
    if batch_stats:
        yd = y.double().view(-1, p.c)
        s1, s2 = dref.bn_sums_f64(yd)
        mean, invstd, _, _ = dref.bn_finalize_f64(s1, s2, float(yd.shape[0]), EPS, MOMENTUM)
        mean, invstd = mean.float(), invstd.float()
    else:
        mean = 0.3 * torch.randn(p.c, generator=gen)
        invstd = 0.5 + torch.rand(p.c, generator=gen)
    dout = torch.randn(p.b, p.t, p.h // p.pool, p.w // p.pool, p.c, generator=gen)
    return dict(y=y.contiguous(), mean=mean, invstd=invstd, gamma=gamma, beta=beta, dout=dout)


@functools.lru_cache(maxsize=None)
def fwd_reference(p, small_gamma=False, batch_stats=False):
    """(out float64, argmax uint8 or None)"""
    d = pool_input(p, small_gamma, batch_stats)
    return dref.bn_pool_act_fwd_f64(d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"], p.pool, p.act)


@functools.lru_cache(maxsize=None)
def bwd_reference(p, small_gamma=False):
    """the written-out backward pass for the batch statistics given in float32, with the reference argmax"""
    d = pool_input(p, small_gamma, True)
    _, arg = fwd_reference(p, small_gamma, True)
    return dref.bn_pool_act_bwd_f64(d["dout"], d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"], p.pool, p.act, arg)


def routing_dout(p):
    """a pooled gradient that is zero outside one position (every channel of it): the last one, whose window ends where the pool's
    coverage ends"""
    dout = torch.zeros(p.b, p.t, p.h // p.pool, p.w // p.pool, p.c)
    dout[-1, -1, -1, -1, :] = 64.0
    return dout


@functools.lru_cache(maxsize=None)
def routing_reference(p):
    d = pool_input(p, False, True)
    _, arg = fwd_reference(p, False, True)
    return dref.bn_pool_act_bwd_f64(routing_dout(p), d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"], p.pool, p.act, arg)


def seq_strides(p):
    """element strides (b, t, pooled position, c) of the pooled tensor inside the [B, C, 2 * T * S] sequence buffer"""
    s = (p.h // p.pool) * (p.w // p.pool)
    return (p.c * 2 * p.t * s, s, 1, 2 * p.t * s)


def to_seq(pooled_cl, fill):
    """channels-last pooled tensor -> the sequence buffer holding it in its first half, `fill` in the other"""
    b, t, hp, wp, c = pooled_cl.shape
    s = hp * wp
    seq = torch.full((b, c, 2 * t * s), float(fill), dtype=pooled_cl.dtype, device=pooled_cl.device)
    seq[:, :, :t * s] = pooled_cl.permute(0, 4, 1, 2, 3).reshape(b, c, t * s)
    return seq
