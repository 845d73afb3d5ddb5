"""TEST INFRASTRUCTURE ONLY -- float64 references of the GEMM family (csrc/gemm.hip, linear_skinny.hip) and of the BatchNorm /
max-pool / activation family (csrc/bn_pool.hip), written from the definition of each operation and not from the kernels.
Plain torch on the CPU; tests/test_gemm_edges_cpu.py and tests/test_bn_pool_edges_cpu.py check them against torch's own
operators before the GPU tests rely on them."""
import torch
import torch.nn.functional as F

ACT_NONE, ACT_TANH, ACT_SIGMOID = 0, 1, 2      # gemm epilogues
BN_LEAKY, BN_TANH = 0, 1                        # bn_pool_act activations
LEAKY_SLOPE = 0.01


# ---------------------------------------------------------------------------------------------- GEMM
def round_operand(x, mode):
    """what the MFMA operand arithmetic of `mode` does to a float32 operand: 0 bf16, 1 nothing, 2 IEEE half"""
    if mode == 1:
        return x
    return x.to(torch.float16 if mode == 2 else torch.bfloat16).to(torch.float32)


def gemm_f64(a, b, trans_a, trans_b, alpha=1.0, c0=None, act=ACT_NONE, mode=1, trans_c=False):
    """float64 act(alpha * op(a) @ op(b)^T (+ c0)): a [M,K] (or [K,M] if trans_a), b [N,K] (or [K,N] if trans_b), c0 / result [M,N]
    (or [N,M] if trans_c)."""
    a, b = round_operand(a, mode).double(), round_operand(b, mode).double()
    z = (a.t() if trans_a else a) @ (b if trans_b else b.t()) * float(alpha)
    if trans_c:
        z = z.t()
    if c0 is not None:
        z = z + c0.double()
    if act == ACT_TANH:
        z = torch.tanh(z)
    elif act == ACT_SIGMOID:
        z = torch.sigmoid(z)
    return z.contiguous()


def gemm_abs_sum(a, b, trans_a, trans_b):
    """max over outputs of sum_k |a||b| (float64): with operands on a grid of 2^-g, every partial sum of every output, in any
    order, is a multiple of 2^-g no larger than this."""
    a, b = a.double().abs(), b.double().abs()
    return float(((a.t() if trans_a else a) @ (b if trans_b else b.t())).max())


# ---------------------------------------------------------------------------------------------- BatchNorm statistics
def bn_sums_f64(y2d):
    """y [rows, C] -> per-channel (sum, sum of squares) in float64"""
    y = y2d.double()
    return y.sum(0), (y * y).sum(0)


def bn_finalize_f64(s1, s2, count, eps, momentum, running_mean=None, running_var=None):
    """Per-channel sums -> (mean, invstd, running_mean, running_var) of a train-mode BatchNorm, all float64: biased variance for the
    normalisation, unbiased for the running estimate.  eps and momentum are used at their float32 values (the kernels take them as
    floats); the caller rounds the results to float32 once."""
    eps, momentum = float(torch.tensor(eps, dtype=torch.float32)), float(torch.tensor(momentum, dtype=torch.float32))
    s1, s2 = s1.double(), s2.double()
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    rm = rv = None
    if running_mean is not None:
        unbiased = var * count / (count - 1.0) if count > 1 else var
        rm = (1.0 - momentum) * running_mean.double() + momentum * mean
        rv = (1.0 - momentum) * running_var.double() + momentum * unbiased
    return mean, invstd, rm, rv


def ulp_distance(got, want):
    """number of float32 values between two float32 tensors of the same sign pattern (0 = equal)"""
    assert got.dtype == torch.float32 and want.dtype == torch.float32
    gi, wi = got.contiguous().view(torch.int32).long(), want.contiguous().view(torch.int32).long()
    gi = torch.where(gi < 0, -(gi & 0x7FFFFFFF), gi)
    wi = torch.where(wi < 0, -(wi & 0x7FFFFFFF), wi)
    return (gi - wi).abs()


# ---------------------------------------------------------------------------------------------- BatchNorm + pool + activation
def to_ncdhw(x):      # channels-last [B,T,H,W,C] -> [B,C,T,H,W]
    return x.permute(0, 4, 1, 2, 3).contiguous()


def to_cl(x):         # [B,C,T,H,W] -> channels-last
    return x.permute(0, 2, 3, 4, 1).contiguous()


def bn_normalise_f64(y_cl, mean, invstd, gamma, beta):
    """z = gamma * (y - mean) * invstd + beta in float64 from the float32 parameters; channels-last in and out"""
    return gamma.double() * ((y_cl.double() - mean.double()) * invstd.double()) + beta.double()


def _act(z, act):
    return torch.tanh(z) if act == BN_TANH else F.leaky_relu(z, LEAKY_SLOPE)


def bn_pool_act_fwd_f64(y_cl, mean, invstd, gamma, beta, pool, act):
    """-> (out float64 channels-last [B,T,H//p,W//p,C], arg uint8 or None): arg is the window offset dy * p + dx of the element
    F.max_pool3d (float64, CPU) reports as the maximum."""
    z = to_ncdhw(bn_normalise_f64(y_cl, mean, invstd, gamma, beta))
    if pool == 1:
        return to_cl(_act(z, act)), None
    b, c, t, h, w = z.shape
    zp, idx = F.max_pool3d(z, (1, pool, pool), return_indices=True)
    hp, wp = h // pool, w // pool
    it, rem = idx // (h * w), idx % (h * w)
    iy, ix = rem // w, rem % w
    py = torch.arange(hp).view(1, 1, 1, hp, 1)
    px = torch.arange(wp).view(1, 1, 1, 1, wp)
    assert bool((it == torch.arange(t).view(1, 1, t, 1, 1)).all())
    dy, dx = iy - py * pool, ix - px * pool
    assert bool(((dy >= 0) & (dy < pool) & (dx >= 0) & (dx < pool)).all())
    return to_cl(_act(zp, act)), to_cl((dy * pool + dx).to(torch.uint8))


def first_max_offsets(z_cl, pool):
    """The argmax convention written out: offset dy * p + dx of the FIRST maximum of each window in that order.  z channels-last
    float64 -> uint8 [B,T,Hp,Wp,C]."""
    b, t, h, w, c = z_cl.shape
    hp, wp = h // pool, w // pool
    win = z_cl[:, :, :hp * pool, :wp * pool].reshape(b, t, hp, pool, wp, pool, c).permute(0, 1, 2, 4, 6, 3, 5).reshape(b, t, hp, wp, c, pool * pool)
    is_max = win == win.max(-1, keepdim=True).values
    order = torch.arange(pool * pool).expand_as(win)
    return torch.where(is_max, order, torch.full_like(order, pool * pool)).min(-1).values.to(torch.uint8)


def max_ties(z_cl, pool):
    """share of windows whose maximum is attained more than once"""
    b, t, h, w, c = z_cl.shape
    hp, wp = h // pool, w // pool
    win = z_cl[:, :, :hp * pool, :wp * pool].reshape(b, t, hp, pool, wp, pool, c).permute(0, 1, 2, 4, 6, 3, 5).reshape(-1, pool * pool)
    return float(((win == win.max(-1, keepdim=True).values).sum(-1) > 1).double().mean())


def scatter_from_pool(g_pooled_cl, arg, shape_cl, pool):
    """pooled gradient [B,T,Hp,Wp,C] -> full resolution [B,T,H,W,C], each value at the window offset arg (dy * p + dx) of its window,
    zero elsewhere (rows / columns the pool drops included)"""
    b, t, h, w, c = shape_cl
    if pool == 1:
        return g_pooled_cl.clone()
    hp, wp = h // pool, w // pool
    full = g_pooled_cl.new_zeros(b, t, h, w, c)
    a = arg.long()
    for q in range(pool * pool):
        dy, dx = q // pool, q % pool
        full[:, :, dy:hp * pool:pool, dx:wp * pool:pool] = torch.where(a == q, g_pooled_cl, torch.zeros_like(g_pooled_cl))
    return full


def bn_pool_act_bwd_f64(dout_cl, y_cl, mean, invstd, gamma, beta, pool, act, arg):
    """The backward pass of train-mode BatchNorm -> MaxPool(1,p,p) -> activation, written out for GIVEN batch statistics and a given
    argmax (the kernels' convention), all float64:
        g      = dout * act'(z at the argmax), routed to the argmax position
        dbeta  = sum g,  dgamma = sum g * xhat
        dy     = gamma * invstd * (g - dbeta / N - xhat * dgamma / N),   N = B T H W
    -> dict(dy, dgamma, dbeta, g_full, dense, k0, k1, k2): dense = dy - k0 * g_full, the part every position receives."""
    b, t, h, w, c = y_cl.shape
    xhat = (y_cl.double() - mean.double()) * invstd.double()
    z = gamma.double() * xhat + beta.double()
    if pool > 1:
        hp, wp = h // pool, w // pool
        win = z[:, :, :hp * pool, :wp * pool].reshape(b, t, hp, pool, wp, pool, c).permute(0, 1, 2, 4, 6, 3, 5).reshape(b, t, hp, wp, c, pool * pool)
        zp = win.gather(-1, arg.long().unsqueeze(-1)).squeeze(-1)
    else:
        zp = z
    dact = 1.0 - torch.tanh(zp) ** 2 if act == BN_TANH else torch.where(zp > 0, torch.ones_like(zp), torch.full_like(zp, LEAKY_SLOPE))
    g_full = scatter_from_pool(dout_cl.double() * dact, arg, y_cl.shape, pool)
    n = float(b * t * h * w)
    dbeta, dgamma = g_full.sum((0, 1, 2, 3)), (g_full * xhat).sum((0, 1, 2, 3))
    k0, k1, k2 = gamma.double() * invstd.double(), dbeta / n, dgamma / n
    dense = k0 * (-k1 - xhat * k2)
    return dict(dy=k0 * g_full + dense, dgamma=dgamma, dbeta=dbeta, g_full=g_full, dense=dense, k0=k0, k1=k1, k2=k2, zp=zp)


def bn_pool_act_autograd_f64(dout_cl, y_cl, gamma, beta, pool, act, eps):
    """float64 autograd of F.batch_norm(training=True) -> F.max_pool3d -> activation -> (out, dy, dgamma, dbeta, mean, invstd), the
    statistics being the batch's own (biased variance)."""
    y = to_ncdhw(y_cl.double()).requires_grad_(True)
    ga, be = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    z = F.batch_norm(y, None, None, ga, be, training=True, eps=eps)
    if pool > 1:
        z = F.max_pool3d(z, (1, pool, pool))
    out = _act(z, act)
    gy, gg, gb = torch.autograd.grad(out, (y, ga, be), to_ncdhw(dout_cl.double()))
    yd = y.detach()
    mean = yd.mean((0, 2, 3, 4))
    var = (yd * yd).mean((0, 2, 3, 4)) - mean * mean
    return to_cl(out.detach()), to_cl(gy), gg, gb, mean, 1.0 / torch.sqrt(var + eps)
