"""One rounding of the exact result: the check the ViT kernel tests apply to their 16-bit outputs.

A kernel that accumulates in f32 and rounds once on its way out stores, for nearly every element, the 16-bit value nearest to the
exact result; where its f32 value lies within its own (small) error of a rounding midpoint it may land on the other neighbour, never
further.  `assert_one_rounding` holds a kernel to exactly that:

  (a) |got - exact| <= 1/2 ulp(max(|got|, |exact|)) + budget     for every element, where `budget` bounds the kernel's error BEFORE
      its final store (f32 accumulation, documented approximations of a function): catches wrong precision and wrong functions;
  (b) at least `min_identical` of the elements are bit-identical to the correctly rounded exact result: catches truncation and
      double rounding, which stay within one ulp and so pass (a).

`exact` is the same operation in float64 on the same 16-bit operands, rounding only where the kernel rounds before its final store.
Imported by the tests like dino_twin (tests/ is on sys.path under pytest); not a conftest.
"""
import math

import torch

U24 = 2.0 ** -24        # f32 unit roundoff

# Bit-identical fractions required of the 16-bit outputs, per kernel family: the lowest fraction the first MI355X run of the tests
# printed (the "[one rounding]" lines) over the family's parametrisations and both formats, less at most one percentage point, never
# below 0.95.  (CPU simulation of a correct f32 kernel: 99.7-99.99 %; a truncating store: 50 %, f16 through bf16: 13 %.)
MIN_IDENTICAL = {
    "gemm": 0.99,          # vit_gemm / vit_ws_gemm epilogue 0 (incl. ViT-B qkv): lowest 99.885 % (vit_gemm, f16)
    "gelu_as": 0.99,       # vit_gemm epilogue 1, A-S erf (incl. ViT-B fc1): lowest 99.859 % (f16)
    "gelu_poly": 0.99,     # vit_ws_gemm epilogue 1, pg_gelu1: lowest 99.758 % (f16)
    "ln_gemm": 0.985,      # LayerNorm-fed products (vit_panel_gemm, vit_ws_gemm_ln, folded weights, _ln_post): lowest 99.287 % (ws_gemm_ln, f16)
    "ln_out": 0.99,        # LayerNorm outputs (vit_layernorm, vit_ws_gemm epilogue 2's xn): lowest 99.922 % (xn, f16)
    "attn": 0.985,         # vit_attn against the float64 flash emulation: lowest 99.377 % (2305 tokens, f16)
}


def ulp(x, dtype):
    """Spacing of the 16-bit format `dtype` at |x| (float64), down to its subnormal spacing."""
    fi = torch.finfo(dtype)
    a = x.double().abs().clamp_min(fi.tiny)
    return fi.eps * torch.exp2(torch.floor(torch.log2(a)))


def round16(x64, dtype):
    """float64 -> `dtype`, rounded ONCE to nearest-even.  torch's own float64 -> 16-bit conversion goes through f32 and so rounds
    twice (1 + 2^-11 + 2^-30 becomes half 1.0 instead of 1 + 2^-10); rounding to f32 by round-to-odd first makes the second rounding
    exact (f32 keeps more than two bits beyond either 16-bit format)."""
    x64 = x64.double()
    f = x64.float()
    fd = f.double()
    inexact = (fd != x64) & torch.isfinite(fd)
    toward_zero = torch.where(fd.abs() > x64.abs(), torch.nextafter(f, torch.zeros_like(f)), f)
    odd = (toward_zero.view(torch.int32) | 1).view(torch.float32)
    return torch.where(inexact, odd, f).to(dtype)


def gemm_budget(a, w, bias=None):
    """Bound on the pre-store error of an f32-accumulated product a @ w^T (+ bias) of 16-bit operands: the products are exact in f32,
    the K-deep sum makes independent roundings of at most 2^-24 of the running magnitude -- 4 sqrt(K) of them bound the sum's error
    by 4 sqrt(K) 2^-24 (|a| @ |w|^T + |bias|) at a margin of four standard deviations of that random walk.  float32 is exact enough for
    a bound (its own error is 1e-7 of it)."""
    k = a.shape[-1]
    mag = a.float().abs() @ w.float().abs().t()
    if bias is not None:
        mag = mag + bias.float().abs()
    return (4.0 * math.sqrt(k) * U24) * mag.double()


def midpoint_slack(x64, dtype, err):
    """Where a kernel rounds an f32 value that may differ from x64 by up to `err` (elementwise), the stored value can be either
    neighbour of x64 if x64 lies within `err` of a rounding midpoint: the spacing of the two neighbours there, 0 elsewhere.  Used for
    operands the kernel rounds INSIDE the operation (LayerNorm output before a product, P before P.V) -- what the exact reference
    cannot know.  The spacing is ulp(x64), not ulp of the rounded value: just below a power of two x64 rounds UP to it, and the
    midpoint it may cross lies half the lower binade's ulp away."""
    x64 = x64.double()
    r = round16(x64, dtype).double()
    u = ulp(x64, dtype)
    gap = 0.5 * u - (x64 - r).abs()                    # distance to the nearest midpoint
    return torch.where(gap <= err, u, torch.zeros_like(u))


def assert_one_rounding(got, exact64, dtype, *, budget64, min_identical, label):
    """Assert (a) and (b) above; print the identical fraction and the worst (|d| - budget) / ulp (at most 0.5 under (a))."""
    assert got.dtype == dtype, (got.dtype, dtype)
    got = got.detach().cpu()
    exact64 = exact64.detach().cpu().double()
    assert got.shape == exact64.shape, (got.shape, exact64.shape)
    g64 = got.double()
    assert torch.isfinite(g64).all(), f"[{label}] non-finite outputs"
    budget64 = torch.as_tensor(budget64, dtype=torch.float64).expand_as(exact64)
    u = ulp(torch.maximum(g64.abs(), exact64.abs()), dtype)
    excess = ((g64 - exact64).abs() - budget64) / u
    worst = excess.max().item()
    same = (got.view(torch.int16) == round16(exact64, dtype).view(torch.int16)).double().mean().item()
    print(f"[one rounding] {label}: {same * 100:.3f} % of {got.numel()} bit-identical (need {min_identical * 100:.1f} %); "
          f"worst (|d| - budget) / ulp {worst:+.3f} (limit +0.5)")
    bad = excess > 0.5
    if bad.any():
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"[{label}] {int(bad.sum())} of {got.numel()} elements beyond half an ulp + budget; first at flat index {i}: "
                             f"got {g64.flatten()[i].item()!r} exact {exact64.flatten()[i].item()!r} budget {budget64.flatten()[i].item():.3e}")
    assert same >= min_identical, f"[{label}] only {same * 100:.3f} % bit-identical to the correctly rounded result (need {min_identical * 100:.1f} %)"
    return same, worst


# ---- float64 references and budgets of the ViT kernels' operations ------------------------------------------------------------------

def stat_err(k):
    """Relative error bound of f32 row statistics over k values (means, sums of squared deviations, merged partials): the same
    4 sqrt(k) 2^-24 random-walk bound as a k-deep product."""
    return 4.0 * math.sqrt(k) * U24


def layernorm64(x, gamma=None, beta=None, eps=1e-6):
    """LayerNorm over the last dim in float64; returns (y, xhat, rstd)."""
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    rstd = ((x - mu).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xhat = (x - mu) * rstd
    y = xhat
    if gamma is not None:
        y = y * gamma.double()
    if beta is not None:
        y = y + beta.double()
    return y, xhat, rstd


def layernorm_err(x, gamma=None, beta=None, eps=1e-6):
    """Bound on |f32 LayerNorm - LN64| elementwise (before any 16-bit rounding): the f32 mean is off by stat_err(K) mean|x| (moves
    every output by |gamma| rstd that much), the f32 variance by stat_err(K) relative (rstd by half of it, + 1 ulp for rsqrt), and the
    normalise / scale / shift make three more roundings of the result."""
    k = x.shape[-1]
    _, xhat, rstd = layernorm64(x, None, None, eps)
    g = gamma.double().abs() if gamma is not None else torch.ones(k, dtype=torch.float64)
    b = beta.double().abs() if beta is not None else torch.zeros(k, dtype=torch.float64)
    dmu = stat_err(k) * x.double().abs().mean(-1, keepdim=True)
    drstd = (0.5 * stat_err(k) + 2 * U24)
    return g * (rstd * dmu + xhat.abs() * drstd) + 3 * U24 * (xhat.abs() * g + b)


def gelu_as64(v):
    """vit_gemm.hip gelu_erf in float64: 0.5 v (1 + erf(v / sqrt 2)) with erf from Abramowitz-Stegun 7.1.26."""
    v = v.double()
    x = v.abs() * 0.70710678118654752
    t = 1.0 / (1.0 + 0.3275911 * x)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    erf_abs = 1.0 - poly * torch.exp(-x * x)
    return 0.5 * v * (1.0 + torch.where(v < 0, -erf_abs, erf_abs))


def gelu_as_budget(v, product_budget):
    """Pre-store error of gelu_erf in f32 on an f32 pre-activation: GELU's slope is at most 1.13 (x 1.2 on the product's budget, +1
    ulp for the bias add); erf(|v|/sqrt 2) is rounded to f32 (<= 2^-24) before 1 + erf cancels, and 1 + erf rounds once more (the
    0.5 |v| 2^-23 term); A-S's poly * exp(-x^2) (= erfc, at most 1) carries __expf's argument and result roundings, the reciprocal and
    the Horner chain -- 8 ulp of erfc, times 0.5 |v|; the products 0.5 v (1 + erf) round twice more."""
    v = v.double()
    erfc = torch.special.erfc(v.abs() * 0.70710678118654752)
    return (1.2 * (product_budget + U24 * v.abs()) + 0.5 * v.abs() * (2.0 ** -23 + 8 * U24 * erfc)
            + 2 * U24 * gelu_as64(v).abs())


def gelu_poly_budget(v, product_budget):
    """Pre-store error of pg_gelu1 (vit_epilogue.h) in f32: the slope of GELU (<= 1.13, x 1.2) on the pre-activation's error; the
    f32 Horner chain and the cancellation in c q + 1/2 cost 2^-23 |v|."""
    return 1.2 * (product_budget + U24 * v.double().abs()) + 2.0 ** -23 * v.double().abs()


def attention64(q, k, v, dtype):
    """The flash kernel's O = softmax2(q k^T) v in float64 (oracle.vit_ref_cpu.flash_attention_emulated, P rounded to `dtype` for
    P.V), and the bound on the kernel's pre-store error of O.  q, k, v: [b, heads, n, 64] holding `dtype` values.

    The kernel's scores are 64-deep f32 products started from -m (the running maximum): off by ds = 4 sqrt(64) 2^-24 (|q| |k|^T + |m|)
    plus the f32 sums of the maximum (2^-24 |m| per tile).  So each exponentiated P_j (hardware exp2: +2 ulp) is off by
    E_j = ln2 (ds_j + max ds) + 3 2^-24 relative (its own score, and the tile maximum it is taken against) -- and where P64_j lies
    within E_j P64_j of a rounding midpoint the kernel's 16-bit P_j may be the other neighbour: ulp_j |v_j| in the numerator
    (midpoint_slack).  The numerator sum, the row sum l and the rescales add 4 sqrt(n) 2^-24 of sum |P| |v| and of l, the final
    1 / l and product two more ulps, and l's relative error (at most max E) moves O by that much.  Tile t's P are taken against
    that tile's running maximum m_t; by the end they carry the weight 2^(m_t - m_final), which the bound applies."""
    from oracle import vit_ref_cpu as vref
    shp = q.shape
    q, k, v = [t.double().reshape(-1, 1, *t.shape[-2:]) for t in (q, k, v)]
    outs = [_attention64_one(q[i:i + 1], k[i:i + 1], v[i:i + 1], dtype, vref) for i in range(q.shape[0])]      # one (frame, head) at a time: n^2 memory
    return torch.cat([o for o, _ in outs]).reshape(shp), torch.cat([b for _, b in outs]).reshape(shp)


def _attention64_one(q, k, v, dtype, vref):
    ps = []

    def r(p):
        ps.append(p)
        return round16(p, dtype).double()
    o = vref.flash_attention_emulated(q, k, v, r)
    assert o.dtype == torch.float64
    n, kt = k.shape[-2], vref.ATT_KT
    s = q @ k.transpose(-2, -1)
    m, ms = torch.zeros(s.shape[:-1] + (1,), dtype=torch.float64), []
    for t0 in range(0, n, kt):                  # the emulation's running maximum after each tile
        mx = (s[..., t0:t0 + kt] - m).amax(-1, keepdim=True)
        m = m + (torch.where(mx > vref.ATT_THR, mx, torch.zeros_like(mx)) if t0 else mx)
        ms.append(m.expand(*m.shape[:-1], min(kt, n - t0)))
    w = torch.exp2(torch.cat(ms, -1) - m)       # 2^(m_t - m_final) per key
    p64 = torch.cat(ps, -1)
    smax = s.abs().amax(-1, keepdim=True) + vref.ATT_THR
    ds = 32 * U24 * ((q.abs() @ k.abs().transpose(-2, -1)) + smax) + (n // kt + 1) * U24 * smax
    e = math.log(2.0) * (ds + ds.amax(-1, keepdim=True)) + 3 * U24
    emax = e.amax(-1, keepdim=True)
    slack = midpoint_slack(p64, dtype, e * p64) * w
    pr = round16(p64, dtype).double().abs() * w
    l = (p64 * w).sum(-1, keepdim=True)
    acc = 4 * math.sqrt(n) * U24
    budget = (slack @ v.abs() + (acc + emax) * (pr @ v.abs())) / l + o.abs() * (acc + emax + 4 * U24)
    return o, budget


def cls_attention64(q, k):
    """vit_cls_attn's f32 CLS rows in float64: 2^(s - max) / sum over the keys (without the CLS column), and the elementwise
    RELATIVE bound on the kernel's error.  The kernel's score is a 64-long f32 fma chain: off by ds = 4 sqrt(64) 2^-24 |q| |k|^T,
    its 2^(s - max) by ln2 (ds + 2^-24 |s - max|) + 2 ulp (exp2f) relative; the row sum is the P-weighted mean of those relative
    errors + 4 sqrt(n) 2^-24 (f32 sum of n terms); 1 / sum and the product add two ulps.  q: [b, h, 64], k: [b, h, n, 64]."""
    q, k = q.double(), k.double()
    s = (k @ q[..., None])[..., 0]
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    ep = math.log(2.0) * (32 * U24 * (k.abs() @ q.abs()[..., None])[..., 0] + U24 * (s - s.amax(-1, keepdim=True)).abs()) + 2 * U24
    rel = ep + (p * ep).sum(-1, keepdim=True) / l + 4 * math.sqrt(s.shape[-1]) * U24 + 2 * U24
    return (p / l)[..., 1:], rel[..., 1:]


# ---- the attention checks shared by tests/test_vit_gpu.py and tests/test_vit_base_gpu.py ------------------------------------------

def assert_attention_one_rounding(out, q, k, v, dt16, min_identical, label):
    """vit_attn's O against flash_attention_emulated in float64 on the same operands (P rounded to the format), rounded once.
    q, k, v: [frames, heads, ntok, 64] holding the kernel's 16-bit operands; out: [rows, heads * 64]."""
    o64, budget = attention64(q, k, v, dt16)
    f, h, n, _ = q.shape
    perm = lambda t: t.transpose(1, 2).reshape(f * n, h * 64)         # noqa: E731
    assert_one_rounding(out.cpu(), perm(o64), dt16, budget64=perm(budget), min_identical=min_identical, label=label)


def assert_cls_rows(att, q, k, label):
    """vit_cls_attn's f32 CLS rows against the float64 exp2-softmax, elementwise relative (derivation: rounding.cls_attention64)."""
    want, rel = cls_attention64(q[:, :, 0], k)
    d = (att.cpu().double() - want).abs()
    ratio = (d / (rel * want + 1e-38)).max().item()
    print(f"[cls rows] {label}: relative bound median {rel.median().item():.1e} max {rel.max().item():.1e}; worst |d| / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
