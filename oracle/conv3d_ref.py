"""TEST INFRASTRUCTURE ONLY -- float64 twins, exactness conditions and derived error bounds for the Conv3d(3,5,5) kernels
(implicit GEMM forward / input gradient, weight gradient, the C_in = 1 first layer and its fused BatchNorm weight gradient).
Plain torch on the CPU; tests/test_conv3d_edges_cpu.py checks each of them before the GPU tests rely on them.

Integer-exact method: with small-integer operands every product and every partial sum of a convolution is an integer, and as
long as sum |a||b| per result stays below 2^24 every such integer is a float32 (and the operands are bf16 / IEEE-half values),
whatever the summation order.  The f32, bf16 and IEEE-half kernels must then return the float64 result bit for bit."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of float32
EXACT = 2.0 ** 24       # integers of magnitude up to here are float32 values
NSLOPE = 0.01           # LeakyReLU


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------- tiles
def tile_h(ho):
    """Rows of the 16-wide output tiles: 14 when that covers the plane with as many tiles as 16 would, else 16."""
    return 14 if cdiv(ho, 14) == cdiv(ho, 16) else 16


def tile_count(b, t, ho, wo):
    """Output tiles (= BatchNorm partial rows) of conv3d_igemm and the weight-gradient kernels."""
    return b * t * cdiv(ho, tile_h(ho)) * cdiv(wo, 16)


def c1_tiles(b, t, h, w):
    return b * t * cdiv(h, 16) * cdiv(w, 16)


# The MFMA first layer's workgroups walk 8 tiles each and write one partial row per workgroup: `#define C1_TPW 8` in
# csrc/conv3d_c1.hip, restated by hand (the check that matters is the exact sum of the partial rows, not this count).
C1_TILES_PER_WG = 8


# ---------------------------------------------------------------------------------------------- convolution twins
def conv3d_f64(x, w, pad):
    """x [B,Ci,T,H,W], w [Co,Ci,3,5,5] -> [B,Co,T,H+2p-4,W+2p-4], float64."""
    return F.conv3d(x.double(), w.double(), padding=(1, pad, pad))


def conv3d_grads_f64(x, w, dy, pad):
    """float64 autograd of conv3d_f64: (input gradient, weight gradient)."""
    x = x.double().clone().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    return torch.autograd.grad(F.conv3d(x, w, padding=(1, pad, pad)), (x, w), dy.double())


def conv3d_direct_f64(x, w, pad):
    """conv3d_f64 spelled out tap by tap, without a library convolution."""
    x, w = x.double(), w.double()
    b, ci, t, h, wd = x.shape
    ho, wo = h + 2 * pad - 4, wd + 2 * pad - 4
    xp = F.pad(x, (pad, pad, pad, pad, 1, 1))
    y = x.new_zeros(b, w.shape[0], t, ho, wo)
    for kd in range(3):
        for kh in range(5):
            for kw in range(5):
                y += torch.einsum("bcthw,oc->bothw", xp[:, :, kd:kd + t, kh:kh + ho, kw:kw + wo], w[:, :, kd, kh, kw])
    return y


def conv3d_direct_grads_f64(x, w, dy, pad):
    """conv3d_grads_f64 spelled out tap by tap, without autograd."""
    x, w, dy = x.double(), w.double(), dy.double()
    b, ci, t, h, wd = x.shape
    ho, wo = h + 2 * pad - 4, wd + 2 * pad - 4
    xp = F.pad(x, (pad, pad, pad, pad, 1, 1))
    gxp, gw = torch.zeros_like(xp), torch.zeros_like(w)
    for kd in range(3):
        for kh in range(5):
            for kw in range(5):
                win = (slice(None), slice(None), slice(kd, kd + t), slice(kh, kh + ho), slice(kw, kw + wo))
                gw[:, :, kd, kh, kw] = torch.einsum("bcthw,bothw->oc", xp[win], dy)
                gxp[win] += torch.einsum("bothw,oc->bcthw", dy, w[:, :, kd, kh, kw])
    return gxp[:, :, 1:1 + t, pad:pad + h, pad:pad + wd], gw


# ---------------------------------------------------------------------------------------------- exactness conditions
def representable_16bit(*tensors):
    """every value survives a round trip through bf16 and through IEEE half"""
    return all(torch.equal(t.float().bfloat16().double(), t.double()) and torch.equal(t.float().half().double(), t.double())
               for t in tensors)


def forward_magnitude(x, w, pad):
    """max over outputs of sum |x||w|"""
    return float(conv3d_f64(x.abs(), w.abs(), pad).max())


def grads_magnitude(x, w, dy, pad):
    """(max over input elements of sum |dy||w|, max over weight elements of sum |x||dy|)"""
    gx, gw = conv3d_grads_f64(x.abs(), w.abs(), dy.abs(), pad)
    return float(gx.max()), float(gw.max())


def bn_partial_magnitudes(y):
    """y [B,C,T,H,W] -> (max over channels of sum |y|, of sum y^2, max |y|)"""
    y = y.double()
    return float(y.abs().sum((0, 2, 3, 4)).max()), float((y * y).sum((0, 2, 3, 4)).max()), float(y.abs().max())


# ---------------------------------------------------------------------------------------------- first layer, fused BatchNorm backward
def c1_taps_f64(x, dy):
    """dW[c][0][kd][kh][kw] = sum over positions of x[pos + tap] * dy[pos][c].  x [B,T,H,W], dy [B,T,H,W,16] -> [16,1,3,5,5]."""
    x, dy = x.double(), dy.double()
    b, t, h, w = x.shape
    xp = F.pad(x, (2, 2, 2, 2, 1, 1))
    dw = x.new_zeros(dy.shape[-1], 1, 3, 5, 5)
    for kd in range(3):
        for kh in range(5):
            for kw in range(5):
                dw[:, 0, kd, kh, kw] = torch.einsum("bthw,bthwc->c", xp[:, kd:kd + t, kh:kh + h, kw:kw + w], dy)
    return dw


def c1_pool_route_f64(dout, out, arg, pool, h, w):
    """g [B,T,H,W,C]: dout * (out > 0 ? 1 : 0.01) at the argmax position (window index a = row * pool + column) of its pool
    window, zero elsewhere and in the strip the pool drops."""
    b, t, hp, wp, c = dout.shape
    gp = dout.double()
    gp = torch.where(out.double() > 0, gp, NSLOPE * gp)
    a = arg.long()
    g = gp.new_zeros(b, t, h, w, c)
    win = g[:, :, :hp * pool, :wp * pool].view(b, t, hp, pool, wp, pool, c)
    for r in range(pool):
        for s in range(pool):
            win[:, :, :, r, :, s] = torch.where(a == r * pool + s, gp, torch.zeros_like(gp))
    return g


def c1_fused_dy_f64(y, dout, out, arg, mean, invstd, coef, pool):
    """The conv-output gradient the fused weight-gradient kernels form in their loader, in float64 from their own inputs:
    dy = k0 (g - k1 - (y - mean) invstd k2), coef = [k0 = gamma invstd, k1 = mean(g), k2 = mean(g xhat)].
    Returns (dy, bound): bound >= |f32 evaluation - dy| = 8 u |k0| (|g| + |k1| + |xhat k2|) -- at most eight roundings of
    partial results, each bounded by that sum."""
    y = y.double()
    g = c1_pool_route_f64(dout, out, arg, pool, y.shape[2], y.shape[3])
    k0, k1, k2 = coef.double().view(3, -1)
    xhat = (y - mean.double()) * invstd.double()
    dy = k0 * (g - k1 - xhat * k2)
    bound = 8 * U * k0.abs() * (g.abs() + k1.abs() + (xhat * k2).abs())
    return dy, bound


def c1_wgrad_bn_f32_bound(x, dy, dy_bound):
    """bound [16,1,3,5,5] on the exact-f32 fused kernel: the dy errors through the products, plus P u sum |x||dy| for the
    product sum over the P positions in any order."""
    p = x.numel()
    return c1_taps_f64(x.abs(), dy_bound) + p * U * c1_taps_f64(x.abs(), dy.abs())


def bf16_ulp(v):
    """spacing of bf16 (8 significant bits) at |v|, float64; 0 at 0"""
    m, e = torch.frexp(v.double().abs())
    return torch.where(v == 0, torch.zeros_like(m), torch.ldexp(torch.ones_like(m), e - 8))


def bf16_undecided(dy, dy_bound):
    """elements whose float64 value lies within their own f32 evaluation bound of a bf16 rounding boundary (the midpoint of two
    neighbouring bf16 values): two correct f32 evaluations may round them to different bf16 values"""
    ulp = bf16_ulp(dy)
    scaled = dy.double().abs() / torch.where(ulp > 0, ulp, torch.ones_like(ulp))
    dist = (scaled - scaled.floor() - 0.5).abs() * ulp
    return (ulp > 0) & (dist <= dy_bound)


def c1_wgrad_bn_bf16_bound(x16, dy16, undecided):
    """x16, dy16: the bf16 operands as float64.  Only f32 accumulation remains: P u sum |x||dy|; an undecided dy element may sit
    one bf16 step away: |x| ulp(dy) for those alone."""
    p = x16.numel()
    slack = torch.where(undecided, bf16_ulp(dy16), torch.zeros_like(dy16.double()))
    return p * U * c1_taps_f64(x16.abs(), dy16.abs()) + c1_taps_f64(x16.abs(), slack)


def c1_chain_f64(x, w, gamma, beta, dout, pool, eps=1e-5):
    """The producers of the fused kernels' inputs, restated in float64: conv -> train-mode BatchNorm -> MaxPool(1,p,p) ->
    LeakyReLU(0.01) and the BatchNorm backward coefficients.  x [B,T,H,W], w [16,1,3,5,5], dout [B,T,H//p,W//p,16].
    Returns dict(y [B,T,H,W,16], mean, invstd, out, arg (window index row * p + column), coef [3,16]) in float64."""
    x, w, gamma, beta, dout = x.double(), w.double(), gamma.double(), beta.double(), dout.double()
    b, t, h, wd = x.shape
    hp, wp = h // pool, wd // pool
    y = conv3d_f64(x[:, None], w, 2).permute(0, 2, 3, 4, 1).contiguous()
    mean = y.mean((0, 1, 2, 3))
    invstd = (y.var((0, 1, 2, 3), unbiased=False) + eps).rsqrt()
    xhat = (y - mean) * invstd
    z = xhat * gamma + beta
    zw = z[:, :, :hp * pool, :wp * pool].reshape(b, t, hp, pool, wp, pool, 16).permute(0, 1, 2, 4, 6, 3, 5).reshape(b, t, hp, wp, 16, pool * pool)
    pooled, arg = zw.max(-1)
    out = torch.where(pooled > 0, pooled, NSLOPE * pooled)
    g = c1_pool_route_f64(dout, out, arg, pool, h, wd)
    coef = torch.stack([gamma * invstd, g.mean((0, 1, 2, 3)), (g * xhat).mean((0, 1, 2, 3))])
    return dict(y=y, mean=mean, invstd=invstd, out=out, arg=arg, coef=coef)
