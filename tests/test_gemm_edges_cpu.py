"""What test_gemm_edges_gpu.py relies on, shown on exactly its inputs without a GPU: the float64 reference is the product torch
computes, every case meets the condition under which float32 arithmetic in ANY order is exact, bf16 rounding really changes A (so
a precise path that rounded its operands could not pass), a single dropped or doubled term changes the float32 result, and the
buffers the operands travel in hold NaN everywhere outside the operand."""
import pytest
import torch

import gemm_edges_cases as cs
from oracle import dense_edges_ref as dref

ALL = cs.all_exact_cases()
IDS = [c.tag for c in ALL]


def test_case_tags_are_unique_and_the_lists_cover_what_the_kernels_branch_on():
    assert len(set(IDS)) == len(IDS)
    fwd = [c for c in cs.FWD]
    assert {c.m for c in fwd} == {1, 15, 16, 17, 32} and {c.n for c in fwd} == {512, 516, 640} and {c.k for c in fwd} == {16, 496, 512, 528, 1040}
    assert any((c.m, c.n, c.k) == (17, 516, 528) for c in fwd)
    dx = [c for c in cs.DX]
    assert {c.n for c in dx} == {256, 260, 320} and {c.k for c in dx} == {512, 513, 576, 1030} and {c.m for c in dx} == {1, 15, 16, 17, 32}
    dw = [c for c in cs.DW]
    assert {c.k for c in dw} == {1, 5, 31, 32} and {c.m for c in dw} == {256, 257, 300} and {c.n for c in dw} == {256, 260, 324}
    assert max(c.k for c in ALL) <= 2064
    for c in cs.BIG:
        assert c.m * c.n >= 128 * 128 * 512 and c.m % 128 and c.n % 128
        assert (c.m + 1) * cs.leading_dim(c.n, 1) * 4 < 34 * 2 ** 20      # the largest allocation of the GPU test
    # every form's multi-slice shape really has more than one slice of 512, the single-slice one has one
    assert cs.FWD_MULTI.k > 512 and cs.DX_MULTI.k > 512 and cs.FWD_SINGLE.k <= 512 and cs.DX_SINGLE.k <= 512
    # explicit split_k = 3 at K = 100: slices of 64, hence two of them
    kps = -(-(-(-100 // 3)) // 32) * 32
    assert kps == 64 and -(-100 // kps) == 2


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_exactness_condition_and_reference(c):
    a, b, c0 = cs.inputs(c)
    sa, sb, sc = cs.shapes(c)
    assert tuple(a.shape) == sa and tuple(b.shape) == sb and tuple(c0.shape) == sc
    # the grids: A on multiples of 2^-8 with |A| < 4, B and the prior C integers
    assert torch.equal(a * 256, (a * 256).round()) and float(a.abs().max()) < 4
    assert torch.equal(b, b.round()) and float(b.abs().max()) <= 3
    assert torch.equal(c0, c0.round()) and float(c0.abs().max()) <= 100
    ar, br = dref.round_operand(a, c.mode), dref.round_operand(b, c.mode)
    assert torch.equal(br, b)
    if c.mode == cs.BF16 and a.numel() >= 64:
        assert not torch.equal(ar, a), "bf16 must change A, or the mode's rounding goes unchecked"
    if c.mode == cs.F16:
        assert torch.equal(ar, a)      # 2 + 8 bits fit an IEEE half
    assert torch.equal(ar * 256, (ar * 256).round())      # still on the grid after rounding
    # any partial sum of any output is a multiple of 2^-8 bounded by sum |a||b|; alpha (a power of two or 0.5, -2) moves the grid to
    # 2^-9 at the finest for the values added to the prior C: all of it fits 24 bits
    assert c.alpha in (1.0, 0.5, -2.0, cs.ACT_ALPHA)
    bound = dref.gemm_abs_sum(ar, br, c.ta, c.tb)
    if c.alpha == cs.ACT_ALPHA:
        assert bound * 2 ** 8 < 2 ** 24 and (bound * c.alpha + 100) * 2 ** 14 < 2 ** 24
    else:
        assert (bound * max(1.0, abs(c.alpha)) + 100) * 2 ** 9 < 2 ** 24, bound
    want = cs.reference(c)
    assert tuple(want.shape) == sc and want.dtype == torch.float64
    if c.act == cs.NONE:
        assert torch.equal(want.float().double(), want), "the exact result is a float32 number"
        # torch's own float32 arithmetic (another summation order) gives the same bits
        z = ((ar.t() if c.ta else ar) @ (br if c.tb else br.t())) * c.alpha
        z = z.t() if c.tc else z
        got32 = z + c0 if c.beta else z
        assert torch.equal(got32, want.float())
    else:
        pre = dref.gemm_f64(a, b, c.ta, c.tb, c.alpha, c0 if c.beta else None, cs.NONE, c.mode, c.tc)
        f = torch.tanh if c.act == cs.TANH else torch.sigmoid
        assert torch.equal(want, f(pre))
        z = pre - (c0.double() if c.beta else 0)
        assert 0.25 < float(z.std()) < 3.0 and float(z.abs().max()) > 1.0, "the activation's argument should span its curved part"
        # torch's float32 activation of the exact pre-activation value is inside the tolerance the GPU test applies
        err = (f(pre.float()).double() - want).abs()
        assert bool((err <= cs.ACT_ATOL + cs.ACT_RTOL * want.abs()).all())


@pytest.mark.parametrize("c", [c for c in ALL if c.act == cs.NONE], ids=[c.tag for c in ALL if c.act == cs.NONE])
def test_a_dropped_or_doubled_term_changes_the_float32_result(c):
    a, b, c0 = cs.inputs(c)
    a = dref.round_operand(a, c.mode)
    want = cs.reference(c).float()
    # the non-zero term nearest the last k of the last row and column: what the tails of a kernel are most likely to lose
    nza, nzb = (a.t() if c.ta else a) != 0, (b.t() if c.tb else b) != 0          # [M,K], [N,K]
    k = max(kk for kk in range(c.k) if bool(nza[:, kk].any()) and bool(nzb[:, kk].any()))
    m, n = int(nza[:, k].nonzero().max()), int(nzb[:, k].nonzero().max())
    ia = (k, m) if c.ta else (m, k)
    for factor in (0.0, 2.0):
        a2 = a.clone()
        a2[ia] *= factor
        got = dref.gemm_f64(a2, b, c.ta, c.tb, c.alpha, c0 if c.beta else None, cs.NONE, cs.F32, c.tc).float()
        where = (n, m) if c.tc else (m, n)
        assert float(got[where]) != float(want[where])


def test_buffers_hold_nan_outside_the_operand_and_views_have_the_asked_layout():
    t = torch.arange(15.0).view(3, 5)
    for odd in (0, 1):
        for off in (0, 1):
            buf, view = cs.place(t, odd, off, float("nan"))
            ld = cs.leading_dim(5, odd)
            assert ld > 5 and ld % 4 == odd and view.stride() == (ld, 1) and view.storage_offset() == off
            assert torch.equal(view, t)
            assert buf.numel() == off + 4 * ld and int(torch.isnan(buf).sum()) == buf.numel() - 15
            assert bool(torch.isnan(buf[off + 2 * ld + 5:]).all()) and bool(torch.isnan(buf[:off]).all())
    buf, view = cs.place(t, 1, 1, cs.SENTINEL)
    assert int((buf == cs.SENTINEL).sum()) == buf.numel() - 15


def test_randn_reference_tolerance_is_the_one_of_test_gemm():
    """the deterministic-mode randn runs are compared to float64 at 2e-5 sqrt(K) + 1e-5 (rtol 1e-4): torch's float32 product is inside"""
    for c in cs.DET_RANDN:
        a, b = cs.randn_inputs(c)
        want = dref.gemm_f64(a, b, c.ta, c.tb)
        got = (a @ (b if c.tb else b.t())).double()
        assert bool(((got - want).abs() <= 2e-5 * c.k ** 0.5 + 1e-5 + 1e-4 * want.abs()).all())
