"""The generic convolution kernels (csrc/conv2d_gen.hip) where the STFT decoder takes them: 30 taps, the chunk boundaries of the
weight gradient, channel-padded and NCHW maps.  Integer-exact like test_conv3d_edges_gpu.py: operands are small integers, every
partial sum is an integer below 2^24 (asserted on these very tensors, here and in test_conv2d_gen_edges_cpu.py), so the kernels
must return the float64 reference bit for bit -- torch.equal, no tolerance."""
import pytest
import torch

import conv2d_gen_edges_cases as cs

pytestmark = pytest.mark.gpu


def exact(got, want, what):
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: got {got[idx].item()}, "
                             f"want {want[idx].item()}")


def untouched(pad, what):
    assert pad is None or bool((pad == cs.SENTINEL).all()), f"{what}: the padded channels were written"


def maps(c, small, big, fill=0.0):
    """ops.Map of the case's small and big tensors in their storage layouts, on the GPU"""
    from maavss_amd import ops
    st, skw = cs.store(small, c["lay_s"], fill)
    gt, gkw = cs.store(big, c["lay_g"], fill)
    return ops.Map(st.cuda(), **skw), ops.Map(gt.cuda(), **gkw)


def check_forward_and_input_gradient(name):
    from maavss_amd import ops
    c = cs.case(name)
    assert c["bound"] < cs.EXACT_BELOW
    w = c["w"].cuda()
    sm, gm = maps(c, c["s"], torch.full_like(c["g"], cs.SENTINEL), fill=cs.SENTINEL)
    ops.conv_gen_big(sm, w, None, gm, c["stride"], c["pad"])
    got, pad = cs.load(gm.t.cpu(), c["lay_g"], c["cb"])
    exact(got, c["big"], f"{name} forward")
    untouched(pad, f"{name} forward")
    sm, gm = maps(c, torch.full_like(c["s"], cs.SENTINEL), c["g"], fill=cs.SENTINEL)
    ops.conv_gen_small(gm, w, None, sm, c["stride"], c["pad"])
    got, pad = cs.load(sm.t.cpu(), c["lay_s"], c["cs"])
    exact(got, c["small"], f"{name} input gradient")
    untouched(pad, f"{name} input gradient")


def check_weight_gradient(name, beta):
    from maavss_amd import ops
    c = cs.case(name)
    assert c["bound"] < cs.EXACT_BELOW
    sm, gm = maps(c, c["s"], c["g"], fill=cs.SENTINEL)      # padded channels hold junk: they must not be read
    # NaNs in the block the caching allocator is likely to hand out as the partial-sum workspace: an unwritten partial shows
    torch.full((ops.query("maavss_conv2d_gen_wgrad_nchunk", c["b"], c["hs"], c["ws"]) * c["w"].numel(),), float("nan"), device="cuda")
    if beta:
        dw = ops.conv_gen_wgrad(sm, gm, c["w"].shape, c["stride"], c["pad"], dw=c["dw0"].cuda(), beta=1)
        exact(dw, c["dw"] + c["dw0"].double(), f"{name} weight gradient onto a prior dw")
    else:
        exact(ops.conv_gen_wgrad(sm, gm, c["w"].shape, c["stride"], c["pad"]), c["dw"], f"{name} weight gradient")


def test_30_tap_kernel_is_exact():
    """(3,10), pad (1,4), stride (1,2), output_padding (0,1): the decoder layer at the tap limit"""
    check_forward_and_input_gradient("taps30")
    check_weight_gradient("taps30", 0)


@pytest.mark.parametrize("beta", (0, 1))
@pytest.mark.parametrize("name", sorted(cs.CHUNK_CASES))
def test_weight_gradient_chunk_boundaries_are_exact(name, beta):
    check_weight_gradient(name, beta)


@pytest.mark.parametrize("name", cs.LAYOUT_CASES)
def test_decoder_layouts_are_exact_and_leave_padded_channels_alone(name):
    check_forward_and_input_gradient(name)
    check_weight_gradient(name, 0)
    check_weight_gradient(name, 1)
