"""tests/rounding.py has teeth: on synthetic outputs of the ViT kernels' operations (the shapes and data of the GPU tests), a correct
f32-accumulated result -- summed in another order than the float64 reference -- passes assert_one_rounding at the committed
MIN_IDENTICAL fractions, and each of the kernel defects below is rejected.  Each defect's line also records whether the tolerance
the GPU tests applied before (np.allclose at the (rtol, atol) quoted) would have accepted it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rounding import (MIN_IDENTICAL, U24, assert_one_rounding, attention64, gelu_as64, gelu_as_budget, gelu_poly_budget, gemm_budget,
                      layernorm64, layernorm_err, midpoint_slack, round16)

DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _gemm(dt, m=1000, n=1152, k=384):
    """test_vit_gemm_epilogues' operands; the f32 product summed over K in reverse order (another summation order than the reference)"""
    a, w, bias = rnd(m, k, seed=1).to(dt), rnd(n, k, seed=2, scale=k ** -0.5).to(dt), rnd(n, seed=3, scale=0.1)
    acc32 = a.float().flip(-1) @ w.float().flip(-1).t()
    return a, w, bias, acc32, a.double() @ w.double().t() + bias.double(), gemm_budget(a, w, bias)


def _gelu_as32(v):
    """vit_gemm.hip gelu_erf evaluated in f32 (as the kernel does)"""
    x = v.abs() * 0.70710678118654752
    t = 1.0 / (1.0 + 0.3275911 * x)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    erf_abs = 1.0 - poly * torch.exp(-x * x)
    return 0.5 * v * (1.0 + torch.where(v < 0, -erf_abs, erf_abs))


def _ln32(x, g, b, unbiased=False):
    mu = x.mean(-1, keepdim=True)
    var = x.var(-1, unbiased=unbiased, keepdim=True)
    return (x - mu) * (var + 1e-6).rsqrt() * g + b


def _attn(dt, ntok=785, frames=2):
    """test_vit_attention_and_cls' operands: q pre-scaled to log2 units, 6 heads of 64"""
    qkv = rnd(frames * ntok, 1152, seed=1)
    qkv[:, :384] *= 0.125 * 3 * 1.4426950408889634
    qkv = qkv.to(dt)
    return [t.view(frames, ntok, 6, 64).transpose(1, 2) for t in qkv.float().split(384, 1)]


def _trunc16(v32, dt):
    """f32 -> 16 bits toward zero (a store that truncates)"""
    r = v32.to(dt)
    over = r.float().abs() > v32.abs()
    return torch.where(over, (r.view(torch.int16) - 1).view(dt), r)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_correct_f32_results_pass(fmt):
    from oracle import vit_ref_cpu as vref
    dt = DT[fmt]
    a, w, bias, acc32, v64, pb = _gemm(dt)
    qs = torch.where(torch.arange(v64.shape[1]) < 384, 0.125, 1.0)
    v32 = acc32 + bias
    assert_one_rounding((v32 * qs).to(dt), v64 * qs.double(), dt, budget64=(pb + U24 * v64.abs()) * qs.double(),
                        min_identical=MIN_IDENTICAL["gemm"], label=f"sim gemm epi 0 {fmt}")
    assert_one_rounding(_gelu_as32(v32).to(dt), gelu_as64(v64), dt, budget64=gelu_as_budget(v64, pb), min_identical=MIN_IDENTICAL["gelu_as"],
                        label=f"sim gemm A-S GELU {fmt}")
    assert_one_rounding(vref.gelu_poly(v32).to(dt), vref.gelu_poly(v64), dt, budget64=gelu_poly_budget(v64, pb),
                        min_identical=MIN_IDENTICAL["gelu_poly"], label=f"sim gemm poly GELU {fmt}")
    # LayerNorm (vit_layernorm's data) and a LayerNorm-fed product (vit_panel_gemm's): LN in f32, rounded, f32 product
    x, g, b = rnd(1003, 384, seed=1, scale=2.0) + 0.3, 1 + 0.1 * rnd(384, seed=2), 0.1 * rnd(384, seed=3)
    y64, lerr = layernorm64(x, g, b)[0], layernorm_err(x, g, b)
    xn = _ln32(x, g, b).to(dt)
    assert_one_rounding(xn, y64, dt, budget64=lerr, min_identical=MIN_IDENTICAL["ln_out"], label=f"sim layernorm {fmt}")
    slack = midpoint_slack(y64, dt, lerr)
    xr = round16(y64, dt)
    z64 = xr.double() @ w.double().t() + bias.double()
    zb = gemm_budget(xr, w, bias) + (slack.float() @ w.float().abs().t()).double()
    z32 = xn.float().flip(-1) @ w.float().flip(-1).t() + bias
    assert_one_rounding(z32.to(dt), z64, dt, budget64=zb + U24 * z64.abs(), min_identical=MIN_IDENTICAL["ln_gemm"], label=f"sim LN gemm {fmt}")
    # attention: the flash recurrence in f32 (P rounded to the format), O rounded
    q, k, v = _attn(dt)
    o32 = vref.flash_attention_emulated(q, k, v, lambda p: p.to(dt).float())
    o64, ob = attention64(q, k, v, dt)
    assert_one_rounding(o32.to(dt), o64, dt, budget64=ob, min_identical=MIN_IDENTICAL["attn"], label=f"sim attention {fmt}")


def _defect(name):
    """(got, exact64, budget64, dtype, min_identical, what the old tolerance compared it with, old (rtol, atol))"""
    from oracle import vit_ref_cpu as vref
    if name in ("truncating store", "f16 through bf16", "bias after a 16-bit rounding"):
        dt = torch.float16
        a, w, bias, acc32, v64, pb = _gemm(dt)
        if name == "truncating store":
            got = _trunc16(acc32 + bias, dt)
        elif name == "f16 through bf16":
            got = (acc32 + bias).to(torch.bfloat16).to(dt)
        else:
            got = (acc32.to(dt).float() + bias).to(dt)
        return got, v64, pb + U24 * v64.abs(), dt, MIN_IDENTICAL["gemm"], (acc32 + bias), (1e-2, 1e-2)
    if name == "tanh GELU":
        dt = torch.float16
        a, w, bias, acc32, v64, pb = _gemm(dt)
        v32 = acc32 + bias
        return F.gelu(v32, approximate="tanh").to(dt), gelu_as64(v64), gelu_as_budget(v64, pb), dt, MIN_IDENTICAL["gelu_as"], F.gelu(v32), (1e-2, 1e-2)
    if name == "unbiased LayerNorm variance":
        dt = torch.bfloat16
        x, g, b = rnd(1003, 384, seed=1, scale=2.0) + 0.3, 1 + 0.1 * rnd(384, seed=2), 0.1 * rnd(384, seed=3)
        return (_ln32(x, g, b, unbiased=True).to(dt), layernorm64(x, g, b)[0], layernorm_err(x, g, b), dt, MIN_IDENTICAL["ln_out"],
                F.layer_norm(x, (384,), g, b, 1e-6), (8e-3, 8e-3))
    if name == "f16 attention with bf16 P and O":
        dt = torch.float16
        q, k, v = _attn(dt)
        got = vref.flash_attention_emulated(q, k, v, lambda p: p.to(torch.bfloat16).float()).to(torch.bfloat16).to(dt)
        o64, ob = attention64(q, k, v, dt)
        want = ((q @ k.transpose(-1, -2)) * 0.6931471805599453).softmax(-1) @ v
        return got, o64, ob, dt, MIN_IDENTICAL["attn"], want, (2e-2, 1.2e-2)
    raise ValueError(name)


@pytest.mark.parametrize("name", ["truncating store", "f16 through bf16", "bias after a 16-bit rounding", "tanh GELU",
                                  "unbiased LayerNorm variance", "f16 attention with bf16 P and O"])
def test_kernel_defects_are_rejected(name):
    got, exact64, budget, dt, need, old_want, (rtol, atol) = _defect(name)
    old_ok = np.allclose(got.float().numpy(), old_want.numpy(), rtol=rtol, atol=atol)
    print(f"[defect] {name}: the previous tolerance (rtol {rtol}, atol {atol}) {'ACCEPTS' if old_ok else 'rejects'} it")
    with pytest.raises(AssertionError):
        assert_one_rounding(got, exact64, dt, budget64=budget, min_identical=need, label=f"defect: {name}")


def test_round16_rounds_once():
    """torch's float64 -> 16-bit conversion rounds twice (through f32); round16 once"""
    x = torch.tensor([1 + 2 ** -11 + 2 ** -30, -(1 + 2 ** -11 + 2 ** -30), 1 + 2 ** -11, 3.0, 2 ** -25 + 2 ** -40], dtype=torch.float64)
    assert round16(x, torch.float16).tolist() == [1 + 2 ** -10, -(1 + 2 ** -10), 1.0, 3.0, 2 ** -24]
    assert x[:1].to(torch.float16).item() == 1.0                     # the double rounding round16 avoids
    y = torch.tensor([1 + 2 ** -8 + 2 ** -30, 1 + 2 ** -8], dtype=torch.float64)
    assert round16(y, torch.bfloat16).tolist() == [1 + 2 ** -7, 1.0]
    r = torch.randn(100000, dtype=torch.float64)
    for dt in (torch.float16, torch.bfloat16):      # away from f32-level midpoints both agree
        assert (round16(r, dt) == r.to(dt)).double().mean().item() > 0.999
