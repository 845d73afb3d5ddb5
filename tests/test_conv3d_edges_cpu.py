"""CPU checks of everything tests/test_conv3d_edges_gpu.py relies on, on exactly the inputs it uses: the float64 twins of
oracle/conv3d_ref.py against independent formulations, the conditions under which the integer cases are exact in every
arithmetic mode (operands representable in bf16 and IEEE half, every sum of absolute products below 2^24), the share of
bf16-undecided elements of the fused BatchNorm gradient, and the multiply-shift division by 3 of the first-layer kernels."""
import pytest
import torch
import torch.nn.functional as F

import conv3d_edges_cases as cs
from oracle import conv3d_ref as cref

IGEMM_CASES = [(n, ci, co) for n in cs.IGEMM_SHAPES for ci, co in cs.PAIRS]
WGRAD_CASES = [(n, ci, co) for n in cs.WGRAD_SHAPES for ci, co in cs.MODEL_PAIRS]


# ------------------------------------------------------------------------------------------------ the twins
def test_tile_counts_match_the_hand_count():
    for name, (b, t, h, w, pad) in cs.IGEMM_SHAPES.items():
        ho, wo = h + 2 * pad - 4, w + 2 * pad - 4
        assert (ho, wo) == cs.IGEMM_OUT[name]
        assert cref.tile_count(b, t, ho, wo) == cs.IGEMM_TILES[name], name
        # conv3d_igemm's allocation of the partial rows counts 16-row tiles: the same number by construction of tile_h
        assert cref.tile_count(b, t, ho, wo) == b * t * cref.cdiv(ho, 16) * cref.cdiv(wo, 16)
    for name, (b, t, h, w, pad) in cs.WGRAD_SHAPES.items():
        assert cref.tile_count(b, t, h + 2 * pad - 4, w + 2 * pad - 4) == cs.WGRAD_TILES[name], name
    assert [cref.tile_h(ho) for ho in (15, 29, 30, 47, 17, 20, 28, 42, 56, 12, 1)] == [16, 16, 16, 16, 14, 14, 14, 14, 14, 14, 14]
    # which input-gradient planes the table promises
    assert cref.tile_h(34) == 14 and 34 - 2 * 14 == 6 and cref.tile_h(5) == 14


@pytest.mark.parametrize("ci,co", [(16, 32), (64, 16)])
def test_conv3d_f64_and_autograd_against_a_direct_loop(ci, co):
    """F.conv3d and its autograd in float64 against the tap loop, on the smallest shape and on a padded multi-frame one."""
    for name in ("a", "h"):
        c = cs.conv_case("igemm", name, ci, co)
        assert torch.equal(cref.conv3d_direct_f64(c["x"], c["w"], c["pad"]), c["y"])
        gx, gw = cref.conv3d_direct_grads_f64(c["x"], c["w"], c["dy"], c["pad"])
        assert torch.equal(gx, c["gx"]) and torch.equal(gw, c["gw"])
    # real values: equal up to float64 summation order
    c = cs.real_case("igemm", "a", ci, co, 1)
    torch.testing.assert_close(cref.conv3d_direct_f64(c["x"], c["w"], c["pad"]), c["y"], rtol=1e-12, atol=1e-12)


def test_c1_taps_is_the_conv_weight_gradient():
    c = cs.c1_case(2, 2, 31, 15)
    assert torch.equal(cref.c1_taps_f64(c["x"], c["dy"]), c["gw"])


# ------------------------------------------------------------------------------------------------ exactness conditions
def _exactness(c):
    assert cref.representable_16bit(c["x"], c["w"], c["dy"], c["prior"])
    assert all(torch.equal(v, v.round()) for v in (c["x"], c["w"], c["dy"], c["prior"]))
    assert cref.forward_magnitude(c["x"], c["w"], c["pad"]) < cref.EXACT
    gx_mag, gw_mag = cref.grads_magnitude(c["x"], c["w"], c["dy"], c["pad"])
    assert gx_mag < cref.EXACT
    assert 2 * gw_mag + float(c["prior"].abs().max()) < cref.EXACT          # doubled: the accumulate form
    s1, s2, ymax = cref.bn_partial_magnitudes(c["y"])
    assert s1 < cref.EXACT and s2 < cref.EXACT and ymax < 4096, (s1, s2, ymax)
    return s2, ymax


@pytest.mark.parametrize("name,ci,co", IGEMM_CASES)
def test_igemm_integer_cases_are_exact_in_every_mode(name, ci, co):
    c = cs.conv_case("igemm", name, ci, co)
    b, t, h, w = c["dims"]
    ho, wo = cs.IGEMM_OUT[name]
    assert c["y"].shape == (b, co, t, ho, wo) and c["gx"].shape == c["x"].shape and c["gw"].shape == c["w"].shape
    assert c["y"].dtype == c["gx"].dtype == c["gw"].dtype == torch.float64
    _exactness(c)
    # asymmetric data: no flip or transposition of the image axes leaves an operand unchanged
    if h > 1 and w > 1 and (ho, wo) != (1, 1):
        for v in (c["x"], c["dy"]):
            assert not torch.equal(v, v.flip(-1)) and not torch.equal(v, v.flip(-2))
            assert v.shape[-1] != v.shape[-2] or not torch.equal(v, v.transpose(-1, -2))
    wk = c["w"]
    assert not torch.equal(wk, wk.flip(-1)) and not torch.equal(wk, wk.flip(-2)) and not torch.equal(wk, wk.flip(-3))
    assert not torch.equal(wk, wk.transpose(-1, -2))


@pytest.mark.parametrize("name,ci,co", WGRAD_CASES)
def test_wgrad_integer_cases_are_exact_in_every_mode(name, ci, co):
    c = cs.conv_case("wgrad", name, ci, co)
    _exactness(c)
    assert bool((c["gw"] != 0).any())


def test_largest_case_magnitudes():
    """64 -> 64 at 2 x 2 x 30 x 17: the case nearest the limits (sum y^2 about 8.4e6 of 1.68e7, max |y| in the hundreds of 4096)."""
    s2, ymax = _exactness(cs.conv_case("igemm", "c", 64, 64))
    assert 2e6 < s2 < cref.EXACT and 100 < ymax < 4096, (s2, ymax)


@pytest.mark.parametrize("b,t,h,w", cs.C1_SHAPES)
def test_c1_integer_cases_are_exact(b, t, h, w):
    c = cs.c1_case(b, t, h, w)
    assert cref.representable_16bit(c["x"], c["w"], c["dy"], c["prior"])
    assert float(c["x"].min()) >= 0
    x5 = c["x"][:, None]
    assert cref.forward_magnitude(x5, c["w"], 2) < cref.EXACT
    _, gw_mag = cref.grads_magnitude(x5, c["w"], c["dy_ncdhw"], 2)
    assert 2 * gw_mag + 3 < cref.EXACT
    s1, s2, ymax = cref.bn_partial_magnitudes(c["y_ncdhw"])
    assert s1 < cref.EXACT and s2 < cref.EXACT and ymax < 4096
    assert torch.equal(cs.from_cl(c["y"]), c["y_ncdhw"])


# ------------------------------------------------------------------------------------------------ fused BatchNorm twin
def test_fused_twin_against_autograd():
    """conv -> train-mode BatchNorm -> max pool -> LeakyReLU in float64 autograd gives the weight gradient the twin forms from the
    chain's intermediate tensors (pool 2 with a dropped row and column, and pool 3)."""
    for b, t, h, w, pool in ((2, 2, 31, 15, 2), (1, 2, 17, 22, 3)):
        x, wgt, gamma, beta, dout = cs.c1_bn_inputs(b, t, h, w, pool)
        wd = wgt.double().requires_grad_(True)
        y = F.conv3d(x.double()[:, None], wd, padding=(1, 2, 2))
        z = F.batch_norm(y, None, None, gamma.double(), beta.double(), training=True, eps=1e-5)
        o = F.leaky_relu(F.max_pool3d(z, (1, pool, pool)), 0.01)
        want, = torch.autograd.grad(o, wd, cs.from_cl(dout.double()))
        ch = cref.c1_chain_f64(x, wgt, gamma, beta, dout, pool)
        torch.testing.assert_close(cs.from_cl(ch["out"]), o.detach(), rtol=1e-12, atol=1e-12)
        dy, bound = cref.c1_fused_dy_f64(ch["y"], dout, ch["out"], ch["arg"], ch["mean"], ch["invstd"], ch["coef"], pool)
        got = cref.c1_taps_f64(x, dy)
        torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-12 * float(want.abs().max()))
        # the strip the pool drops carries no pooled gradient
        g = cref.c1_pool_route_f64(dout, ch["out"], ch["arg"], pool, h, w)
        assert float(g[:, :, (h // pool) * pool:].abs().max() if h % pool else 0) == 0
        assert float(g[:, :, :, (w // pool) * pool:].abs().max() if w % pool else 0) == 0
        assert int((g != 0).sum()) == dout.numel()
        assert bool((bound > 0).all()) and float((bound / dy.abs().clamp_min(1e-30)).median()) < 1e-5


@pytest.mark.parametrize("b,t,h,w,pool", cs.C1_BN_CASES)
def test_undecided_share_of_the_twin(b, t, h, w, pool):
    """Elements of the twin's dy within their f32 evaluation bound of a bf16 rounding boundary: below 1 % on these inputs, for the
    conv output of the f32 operands and of the IEEE-half operands (what the recompute kernel sees)."""
    x, wgt, gamma, beta, dout = cs.c1_bn_inputs(b, t, h, w, pool)
    for xo, wo in ((x, wgt), (x.half().float(), wgt.half().float())):
        ch = cref.c1_chain_f64(xo, wo, gamma, beta, dout, pool)
        f32 = {k: (v.float().double() if v.dtype == torch.float64 else v) for k, v in ch.items()}      # as the kernels receive them
        dy, bound = cref.c1_fused_dy_f64(f32["y"], dout, f32["out"], f32["arg"], f32["mean"], f32["invstd"], f32["coef"], pool)
        share = float(cref.bf16_undecided(dy, bound).double().mean())
        print(f"[undecided {b}x{t}x{h}x{w} pool {pool}] share {share:.5f}")
        assert share < cs.UNDECIDED_MAX_SHARE


def test_bf16_ulp_and_boundaries():
    v = torch.tensor([1.0, 1.5, 1.9999, 2.0, 0.75, -3.0, 0.0, 2.0 ** -10], dtype=torch.float64)
    assert cref.bf16_ulp(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6, 0.0, 2.0 ** -17]
    # agrees with the spacing of torch's bfloat16: the next bf16 value above a bf16 value r > 0 is r + ulp(r)
    r = torch.randn(4096, generator=torch.Generator().manual_seed(3)).abs().bfloat16().float()
    r = r[r > 0]
    nxt = (r.view(torch.int32) + 0x10000).view(torch.float32)
    assert torch.equal(nxt.double() - r.double(), cref.bf16_ulp(r.double()))
    mid = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 1e-6, 1.0 + 2.0 ** -9, -(3.0 + 2.0 ** -7)], dtype=torch.float64)
    tol = torch.full_like(mid, 1e-7)
    assert cref.bf16_undecided(mid, tol).tolist() == [True, False, False, True]
    assert cref.bf16_undecided(mid, torch.full_like(mid, 2e-6)).tolist() == [True, True, False, True]


# ------------------------------------------------------------------------------------------------ division by 3
def test_c1_pdiv_multiply_shift_is_division_by_three():
    """(x * 43691) >> 17 == x // 3 for every x the entry points admit (H, W < 98304), in 32-bit unsigned arithmetic."""
    x = torch.arange(98304, dtype=torch.int64)
    prod = x * 43691
    assert int(prod.max()) < 2 ** 32
    assert torch.equal(prod >> 17, x // 3)
    assert 98304 * 43691 >= 2 ** 32      # the admitted range is all the 32-bit product allows
