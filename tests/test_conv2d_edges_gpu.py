"""The STFT encoder's Conv2d(k=(3,9), pad (1,pw), bias=False) kernels at their edges: maps a few rows high where every tap clips
at every border, every stride and input layout, the channel counts the position / row kernels of csrc/conv2d.hip refuse, and the
chunk boundaries of the weight gradient.  Integer-exact like test_conv2d_gen_edges_gpu.py: operands are small integers, every
partial sum is an integer below 2^24 (asserted on these very tensors, here and in test_conv2d_edges_cpu.py), so whichever kernel
serves a shape must return the float64 reference bit for bit -- torch.equal, no tolerance."""
import pytest
import torch

import conv2d_edges_cases as cs

pytestmark = pytest.mark.gpu


def exact(got, want, what):
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: got {got[idx].item()}, "
                             f"want {want[idx].item()}")


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def check_forward_and_input_gradient(name):
    from maavss_amd import ops
    c = cs.case(name)
    assert c["bound"] < cs.EXACT_BELOW
    w = c["wt"].cuda()
    x = c["x"].cuda() if c["nchw"] else nhwc(c["x"])
    y = ops.conv2d_fwd(x, w, c["stride"], c["pw"], c["nchw"])
    exact(y.permute(0, 3, 1, 2), c["y"], f"{name} forward")
    dx = ops.conv2d_dgrad(nhwc(c["dy"]), w, (c["h"], c["w"]), c["stride"], c["pw"])
    exact(dx.permute(0, 3, 1, 2), c["dx"], f"{name} input gradient")


def check_weight_gradient(name, beta):
    from maavss_amd import ops
    c = cs.case(name)
    assert c["bound"] < cs.EXACT_BELOW
    x = c["x"].cuda() if c["nchw"] else nhwc(c["x"])
    dy = nhwc(c["dy"])
    # NaNs in the block the caching allocator is likely to hand out as the partial-sum workspace: an unwritten partial shows
    torch.full((2 * c["wt"].numel(),), float("nan"), device="cuda")
    if beta:
        dw = ops.conv2d_wgrad(x, dy, c["wt"].shape, c["stride"], c["pw"], c["nchw"], dw=c["dw0"].cuda(), beta=1)
        exact(dw, c["dw"] + c["dw0"].double(), f"{name} weight gradient onto a prior dw")
    else:
        exact(ops.conv2d_wgrad(x, dy, c["wt"].shape, c["stride"], c["pw"], c["nchw"]), c["dw"], f"{name} weight gradient")


@pytest.mark.parametrize("name", cs.TUNED_CASES)
def test_tuned_shapes_are_exact(name):
    check_forward_and_input_gradient(name)
    check_weight_gradient(name, 0)


@pytest.mark.parametrize("name", cs.REFUSED_CASES)
def test_shapes_the_tuned_kernels_refuse_are_exact(name):
    check_forward_and_input_gradient(name)
    check_weight_gradient(name, 0)


@pytest.mark.parametrize("beta", (0, 1))
@pytest.mark.parametrize("name", cs.CHUNK_CASES)
def test_weight_gradient_chunk_boundaries_are_exact(name, beta):
    check_weight_gradient(name, beta)


@pytest.mark.parametrize("name", ("tuned_2_4_s22_p3_nchw", "tuned_16_16_s12_p4_nhwc", "refused_3_6_s22_p4", "refused_4_32_s21_p4"))
def test_weight_gradient_onto_a_prior_dw_is_exact(name):
    check_weight_gradient(name, 1)
