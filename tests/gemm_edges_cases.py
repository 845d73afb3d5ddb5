"""Shapes and inputs shared by test_gemm_edges_cpu.py (which checks the reference and the exactness conditions) and
test_gemm_edges_gpu.py (which holds csrc/gemm.hip and csrc/linear_skinny.hip to them).

Notation follows ops.gemm: C[M,N] = act(alpha * op(A) @ op(B)^T) (+ C); A is stored [M,K] ([K,M] with trans_a), B [N,K] ([K,N] with
trans_b).  Inputs: A = i + j / 256 (|i| <= 3, 0 <= j < 256), B integer in [-3, 3], prior C integer in [-100, 100]: every product
and every partial sum, in any order, is a multiple of 2^-9 below 2^15, so f32 stores, f32 atomics and the ordered deterministic
reduction all return the float64 result bit for bit.  A's fraction does not survive bf16, so the reference of modes 0 and 2 is
formed from the operands rounded as the mode rounds them."""
import collections
import functools

import torch

from oracle import dense_edges_ref as dref

BF16, F32, F16 = 0, 1, 2                      # ops.MODE_*
NONE, TANH, SIGMOID = 0, 1, 2                 # ops.ACT_*
ACT_ALPHA = 2.0 ** -6                         # activations: z = alpha * sum spans roughly +-3
ACT_RTOL, ACT_ATOL = 1e-4, 2e-5               # test_gemm_epilogues' tolerances for the weight-streaming forms
SENTINEL = 12345.0                            # what the output buffer holds outside (and, with beta = 0, inside) C

Case = collections.namedtuple("Case", "tag m n k ta tb tc mode alpha beta act split_k odd off seed")


def G(tag, m, n, k, ta=False, tb=False, tc=False, mode=F32, alpha=1.0, beta=0, act=NONE, split_k=0, odd=(0, 0, 0), off=(0, 0, 0), seed=0):
    """odd: per operand (A, B, C) 1 = leading dimension one float wider than a multiple of 4; off: floats between the buffer's start
    (16-byte aligned) and the operand's first element."""
    return Case(tag, m, n, k, ta, tb, tc, mode, alpha, beta, act, split_k, tuple(odd), tuple(off), seed)


# (alpha, beta, act) variants run on a single-slice and on a multi-slice shape of each weight-streaming form; the act = 0 twin of
# an activation case pins its pre-activation value exactly
EPILOGUES = ((0.5, 1, NONE), (-2.0, 0, NONE), (ACT_ALPHA, 0, NONE), (ACT_ALPHA, 1, NONE), (ACT_ALPHA, 0, TANH), (ACT_ALPHA, 1, SIGMOID))


def _with_epilogues(base):
    return [base._replace(tag=f"{base.tag}/a{al:g}b{be}f{ac}", alpha=al, beta=be, act=ac) for al, be, ac in EPILOGUES]


# ---- fwd form: M <= 32, N >= 512, N % 4 == 0, K % 16 == 0, K slices of 512, 128 columns per workgroup, 16 per wave
FWD_SINGLE = G("fwd/16x640x512", 16, 640, 512)
FWD_MULTI = G("fwd/32x640x1040", 32, 640, 1040)                  # slices of 512, 512 and 16 columns
FWD = [G("fwd/1x512x16", 1, 512, 16), G("fwd/15x516x496", 15, 516, 496), FWD_SINGLE,
       G("fwd/17x516x528", 17, 516, 528),                       # the three tails at once: rows past 16, 4 columns, a 16-wide K slice
       FWD_MULTI] + _with_epilogues(FWD_SINGLE) + _with_epilogues(FWD_MULTI)
FWD_OUTSIDE = [G("fwd-out/M33", 33, 640, 512), G("fwd-out/N508", 16, 508, 512), G("fwd-out/N514", 16, 514, 512),
               G("fwd-out/K520", 16, 640, 520),
               G("fwd-out/lda", 16, 640, 512, odd=(1, 0, 0)), G("fwd-out/ldb", 16, 640, 512, odd=(0, 1, 0)),
               G("fwd-out/ldc", 16, 640, 512, odd=(0, 0, 1), alpha=0.5, beta=1),
               G("fwd-out/A+1", 16, 640, 512, off=(1, 0, 0)), G("fwd-out/B+1", 16, 640, 512, off=(0, 1, 0)),
               G("fwd-out/C+1", 16, 640, 512, off=(0, 0, 1), alpha=-2.0, beta=1),
               G("fwd-out/K1040-ldb-C+1", 32, 640, 1040, odd=(0, 1, 0), off=(0, 0, 1), alpha=ACT_ALPHA, act=TANH)]

# ---- dx form (trans_b): M <= 32, N >= 256, N % 4 == 0, K >= 512, K slices of 512 rows, 64 columns per workgroup
DX_SINGLE = G("dx/16x256x512", 16, 256, 512, tb=True)
DX_MULTI = G("dx/32x320x1030", 32, 320, 1030, tb=True)           # slices of 512, 512 and 6 rows
DX = [G("dx/1x256x512", 1, 256, 512, tb=True),
      G("dx/15x260x513", 15, 260, 513, tb=True),                # clamped lanes (260 = 4 * 64 + 4) and a last slice of one row
      G("dx/16x320x576", 16, 320, 576, tb=True), G("dx/17x260x1030", 17, 260, 1030, tb=True), DX_SINGLE, DX_MULTI,
      G("dx/17x260x1030/A+1", 17, 260, 1030, tb=True, odd=(1, 0, 0), off=(1, 0, 0)),      # A is read by scalars: still the dx form
      ] + _with_epilogues(DX_SINGLE) + _with_epilogues(DX_MULTI)
DX_OUTSIDE = [G("dx-out/K511", 16, 256, 511, tb=True), G("dx-out/N252", 16, 252, 512, tb=True), G("dx-out/N258", 16, 258, 512, tb=True),
              G("dx-out/ldb", 16, 256, 512, tb=True, odd=(0, 1, 0)), G("dx-out/C+1", 16, 256, 1030, tb=True, off=(0, 0, 1), alpha=0.5, beta=1)]

# ---- dw form (trans_a, trans_b): batch K <= 32, M >= 256, N >= 256, N % 4 == 0, act == 0; 256 x 256 per workgroup
DW = [G("dw/256x256x1", 256, 256, 1, ta=True, tb=True), G("dw/257x260x5", 257, 260, 5, ta=True, tb=True),
      G("dw/300x324x31", 300, 324, 31, ta=True, tb=True), G("dw/256x260x32", 256, 260, 32, ta=True, tb=True),
      G("dw/300x324x31/beta", 300, 324, 31, ta=True, tb=True, alpha=0.5, beta=1),
      G("dw/257x260x32/beta", 257, 260, 32, ta=True, tb=True, alpha=-2.0, beta=1, odd=(1, 1, 0), off=(1, 1, 0))]
DW_OUTSIDE = [G("dw-out/K33", 256, 256, 33, ta=True, tb=True), G("dw-out/M255", 255, 256, 32, ta=True, tb=True),
              G("dw-out/N258", 256, 258, 32, ta=True, tb=True), G("dw-out/act", 256, 256, 32, ta=True, tb=True, alpha=ACT_ALPHA, act=TANH),
              G("dw-out/act-pin", 256, 256, 32, ta=True, tb=True, alpha=ACT_ALPHA),
              G("dw-out/ldc", 256, 256, 32, ta=True, tb=True, odd=(0, 0, 1), beta=1)]

SKINNY = FWD + DX + DW
OUTSIDE = FWD_OUTSIDE + DX_OUTSIDE + DW_OUTSIDE

# ---- generic kernel: (M, N) -> tile configuration; every transpose combination x trans_c x mode at each K
GENERIC_SHAPES = {"mid": (67, 45),      # 64 x 64 tiles, two block rows, both ragged
                  "narrow": (130, 17),  # N <= 32: 128 x 32 tiles, ragged
                  "swap": (5, 70)}      # M <= 32 < N: the operands change places, then 128 x 32 tiles
GENERIC_K = (1, 31, 33, 100)
MODES = (F32, BF16, F16)


def generic_cases(shape, k):
    m, n = GENERIC_SHAPES[shape]
    out = []
    for i, (ta, tb, tc) in enumerate((ta, tb, tc) for ta in (False, True) for tb in (False, True) for tc in (False, True)):
        for mode in MODES:
            # the epilogue and the buffer layout rotate over the combinations: each appears with every transpose form
            al, be = ((1.0, 0), (0.5, 1), (-2.0, 0), (1.0, 1))[(i + mode) % 4]
            odd = ((0, 0, 0), (1, 1, 1), (1, 0, 1), (0, 1, 0))[(i + 2 * mode + k) % 4]
            off = ((0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 1))[(i // 2 + mode + k) % 4]
            out.append(G(f"gen/{shape}/k{k}/t{int(ta)}{int(tb)}{int(tc)}m{mode}", m, n, k, ta, tb, tc, mode, al, be, NONE, 0, odd, off))
    return out


# explicit split_k = 3 at K = 100: the slice length rounds up to 64, which leaves two slices; zero pass (beta = 0), accumulation onto
# the prior C (beta = 1) and the separate activation pass
SPLIT = [G(f"split3/{tag}m{mode}", 67, 45, 100, ta, tb, tc, mode, al, be, ac, 3, odd=(0, 0, 1), off=(0, 0, 1))
         for mode in MODES
         for tag, ta, tb, tc, al, be, ac in (("nn", False, False, False, 1.0, 0, NONE), ("tt-c", True, True, True, 0.5, 1, NONE),
                                             ("pin", False, True, False, ACT_ALPHA, 0, NONE), ("act", False, True, False, ACT_ALPHA, 0, SIGMOID))
         if not (ac and mode != F32)]
SPLIT += [G("split3/swap", 5, 70, 100, alpha=-2.0, beta=1, split_k=3, odd=(1, 1, 1)), G("split3/narrow", 130, 17, 100, split_k=3, off=(0, 0, 1))]

# 128 x 128 tiles: M * N >= 128 * 128 * 512, both ragged (4100 = 32 * 128 + 4, 2052 = 16 * 128 + 4), K = 40 = one full and one
# quarter K step
BIG = [G("big/nn-f32", 4100, 2052, 40, alpha=0.5, beta=1, odd=(0, 0, 1)), G("big/tt-bf16", 4100, 2052, 40, ta=True, tb=True, mode=BF16, odd=(1, 1, 0), off=(1, 1, 0)),
       G("big/nt-c-f16", 4100, 2052, 40, tb=True, tc=True, mode=F16, alpha=-2.0)]

# deterministic mode: the multi-slice shapes take the workspace path (partial sums + linear_reduce_kernel)
DET = [c._replace(tag="det/" + c.tag) for c in [FWD_MULTI, DX_MULTI] + _with_epilogues(FWD_MULTI) + _with_epilogues(DX_MULTI)]
DET_RANDN = (FWD_MULTI, DX_MULTI)


def forced_generic(c):
    """the same problem with split_k = 1: never a weight-streaming form"""
    return c._replace(tag=c.tag + "/generic", split_k=1)


def ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).float()


def shapes(c):
    """stored shapes of (A, B, C)"""
    return ((c.k, c.m) if c.ta else (c.m, c.k)), ((c.k, c.n) if c.tb else (c.n, c.k)), ((c.n, c.m) if c.tc else (c.m, c.n))


@functools.lru_cache(maxsize=None)
def _inputs(m, n, k, ta, tb, tc, seed):
    gen = torch.Generator().manual_seed(1000 + seed + 7 * m + 13 * n + 31 * k + 2 * ta + tb)
    sa, sb, sc = shapes(G("", m, n, k, ta, tb, tc))
    a = ints(sa, -3, 3, gen) + ints(sa, 0, 255, gen) / 256.0
    b = ints(sb, -3, 3, gen)
    c0 = ints(sc, -100, 100, gen)
    return a, b, c0


def inputs(c):
    """(A, B, prior C) as float32 CPU tensors in their stored shapes; cached, never to be written to"""
    return _inputs(c.m, c.n, c.k, c.ta, c.tb, c.tc, c.seed)


def randn_inputs(c):
    gen = torch.Generator().manual_seed(77 + c.k)
    sa, sb, _ = shapes(c)
    return torch.randn(*sa, generator=gen), torch.randn(*sb, generator=gen)


@functools.lru_cache(maxsize=None)
def _reference(m, n, k, ta, tb, tc, mode, alpha, beta, act, seed):
    a, b, c0 = _inputs(m, n, k, ta, tb, tc, seed)
    return dref.gemm_f64(a, b, ta, tb, alpha, c0 if beta else None, act, mode, tc)


def reference(c):
    """float64 result of the case (independent of split_k, leading dimensions and offsets); cached"""
    return _reference(c.m, c.n, c.k, c.ta, c.tb, c.tc, c.mode, c.alpha, c.beta, c.act, c.seed)


def leading_dim(cols, odd):
    """a leading dimension wider than the row: a multiple of 4 (the weight-streaming forms' condition), or one more"""
    return (cols + 3) // 4 * 4 + 4 + (1 if odd else 0)


def place(t, odd, off, fill, device="cpu"):
    """Embed the 2-D tensor t in a larger buffer filled with `fill`: `off` floats before its first element, leading dimension wider
    than the row, one more row below.  -> (buffer, view of t's shape)."""
    rows, cols = t.shape
    ld = leading_dim(cols, odd)
    buf = torch.full((off + (rows + 1) * ld,), float(fill), dtype=torch.float32)
    view = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t)
    if device != "cpu":
        buf = buf.to(device)
        view = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    return buf, view


def all_exact_cases():
    """every case whose result must equal the reference bit for bit (act == 0) or within the activation tolerance"""
    out = SKINNY + OUTSIDE + SPLIT + BIG + DET
    for s in GENERIC_SHAPES:
        for k in GENERIC_K:
            out = out + generic_cases(s, k)
    return out
