"""maavss_gemm_f32's seven kernels (csrc/gemm.hip: three tile configurations; csrc/linear_skinny.hip: the fwd, dx and dw
weight-streaming forms) on both sides of every condition that chooses among them, against float64.

The inputs (tests/gemm_edges_cases.py) make every product and every partial sum exact in float32 in any order, so the comparison is
torch.equal -- for plain stores, f32 atomics and the ordered deterministic reduction alike; tests/test_gemm_edges_cpu.py asserts the
condition on these very inputs.  Every operand is a view into a buffer whose padding (the columns up to the leading dimension, a
row below, the floats before a misaligned start) holds NaN, and the output a view into a buffer of a finite sentinel: an over-read
that reaches an MFMA poisons the result, and a write outside [M][N] -- by a kernel, a zero pass or an activation pass -- changes the
sentinel.  Activations are compared at test_gemm_epilogues' tolerance; the same case with act = 0 pins the pre-activation value."""
import numpy as np
import pytest
import torch

import gemm_edges_cases as cs
from oracle import dense_edges_ref as dref

pytestmark = pytest.mark.gpu


def run(c, a=None, b=None):
    """One ops.gemm call of case c on padded buffers -> the [M][N] result (device).  Asserts that nothing outside it was written."""
    from maavss_amd import ops
    a0, b0, c0 = cs.inputs(c)
    a, b = (a0 if a is None else a), (b0 if b is None else b)
    nan = float("nan")
    _, av = cs.place(a, c.odd[0], c.off[0], nan, "cuda")
    _, bv = cs.place(b, c.odd[1], c.off[1], nan, "cuda")
    prior = c0 if c.beta else torch.full(c0.shape, cs.SENTINEL)
    cbuf, cv = cs.place(prior, c.odd[2], c.off[2], cs.SENTINEL, "cuda")
    ret = ops.gemm(av, bv, c.ta, c.tb, act=c.act, alpha=c.alpha, out=cv, beta=c.beta, precise=c.mode, split_k=c.split_k, trans_c=c.tc)
    assert ret.data_ptr() == cv.data_ptr()
    got = cv.clone()
    cv.fill_(cs.SENTINEL)
    bad = cbuf != cs.SENTINEL
    assert not bool(bad.any()), f"{c.tag}: {int(bad.sum())} floats outside C[M][N] were written, first at buffer offset {int(bad.nonzero()[0])}"
    return got


def check(c, got=None):
    got = run(c) if got is None else got
    want = cs.reference(c)
    assert not bool(torch.isnan(got).any()), f"{c.tag}: NaN in the result (an operand was read outside its bounds)"
    if c.act == cs.NONE:
        want32 = want.float().cuda()
        if not torch.equal(got, want32):
            bad = got != want32
            idx = tuple(int(i) for i in bad.nonzero()[0])
            raise AssertionError(f"{c.tag}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result, first at {idx}: "
                                 f"got {got[idx].item()!r}, want {want32[idx].item()!r}")
    else:
        np.testing.assert_allclose(got.cpu().double().numpy(), want.numpy(), rtol=cs.ACT_RTOL, atol=cs.ACT_ATOL, err_msg=c.tag)
    return got


@pytest.mark.parametrize("c", cs.SKINNY, ids=[c.tag for c in cs.SKINNY])
def test_weight_streaming_forms_and_the_generic_kernel_on_their_shapes(c):
    """each fwd / dx / dw case as dispatched, and again with split_k = 1 (always the generic kernel): both exact, hence identical"""
    got = check(c)
    got_generic = check(cs.forced_generic(c))
    if c.act == cs.NONE:
        assert torch.equal(got, got_generic)


@pytest.mark.parametrize("c", cs.OUTSIDE, ids=[c.tag for c in cs.OUTSIDE])
def test_just_outside_the_weight_streaming_forms(c):
    """one step past each shape, leading-dimension and alignment condition: whichever kernel takes it returns the same exact result"""
    check(c)


@pytest.mark.parametrize("shape", list(cs.GENERIC_SHAPES))
@pytest.mark.parametrize("k", cs.GENERIC_K)
def test_generic_kernel_transposes_modes_and_ragged_tiles(shape, k):
    for c in cs.generic_cases(shape, k):
        check(c)


@pytest.mark.parametrize("c", cs.SPLIT, ids=[c.tag for c in cs.SPLIT])
def test_explicit_split_k(c):
    check(c)


@pytest.mark.parametrize("c", cs.BIG, ids=[c.tag for c in cs.BIG])
def test_128x128_tiles_with_ragged_edges(c):
    check(c)


@pytest.fixture
def deterministic():
    import maavss_amd
    prev = maavss_amd.set_deterministic(True)
    try:
        yield
    finally:
        maavss_amd.set_deterministic(prev)


@pytest.mark.parametrize("c", cs.DET, ids=[c.tag for c in cs.DET])
def test_deterministic_mode_is_exact(c, deterministic):
    """multi-slice fwd and dx shapes with the workspace: partial sums per slice, added in order by linear_reduce_kernel"""
    check(c)


@pytest.mark.parametrize("c", cs.DET_RANDN, ids=[c.tag for c in cs.DET_RANDN])
def test_deterministic_mode_is_bit_reproducible_on_randn(c, deterministic):
    a, b = cs.randn_inputs(c)
    got1, got2 = run(c, a, b), run(c, a, b)
    assert torch.equal(got1, got2)
    want = dref.gemm_f64(a, b, c.ta, c.tb)
    np.testing.assert_allclose(got1.cpu().double().numpy(), want.numpy(), rtol=1e-4, atol=2e-5 * np.sqrt(c.k) + 1e-5)      # test_gemm's


@pytest.mark.parametrize("c", cs.DET_RANDN, ids=[c.tag for c in cs.DET_RANDN])
def test_deterministic_mode_on_a_second_stream(c, deterministic):
    """the workspace belongs to one stream: on another the library must take a single-slice path, and stay exact"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run(c)
    torch.cuda.current_stream().wait_stream(side)
    side.synchronize()
    check(c, got)
