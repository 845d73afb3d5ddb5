"""The definition of maavss_adamw_ema_step (include/maavss.h, csrc/optim.hip) in numpy -- the contract the kernel is held to.

Per element, with the host scalars below:

    gr = g * gscale
    m  = b1 * m + (1 - b1) * gr
    v  = b2 * v + ((1 - b2) * gr) * gr
    p  = p * decay_s                                  decay_s of the element's segment
    p  = p - (lr_bc1 * m) / (sqrt(v) * inv_sqrt_bc2 + eps)
    e  = d * e + one_m_d * p                          only with an average

Two modes:
* "f32": what the kernel computes, bit for bit.  Every array operation is one numpy float32 ufunc call, i.e. one IEEE single
  operation per element, rounded on its own, in the order written above (numpy fuses nothing across calls; float32 sqrt and divide are
  correctly rounded).  The host scalars are formed in double from the f32 ARGUMENTS of the entry point and rounded once, as optim.hip
  forms them: lr_bc1 = f32(lr / (1 - b1^step)), inv_sqrt_bc2 = f32(1 / sqrt(1 - b2^step)), decay_s = f32(1 - lr * wd_s),
  one_m_d = f32(1 - d), while 1 - b1 and 1 - b2 are f32 subtractions (as adam_body of elementwise.hip writes them).
* "f64": the same expressions in double from the Python floats -- the arithmetic torch.optim.AdamW and lerp(ema, p, 1 - d) perform
  up to rounding; tests/test_optim_cpu.py holds it against torch on double tensors.
"""
import math

import numpy as np

U24 = 2.0 ** -24
U53 = 2.0 ** -53


def host_scalars(lr, beta1, beta2, eps, step, grad_scale, ema_decay, mode):
    """-> dict of the scalars the kernel is launched with (numpy scalars of the mode's type)."""
    if step < 1:
        raise ValueError("step counts from 1")
    if mode == "f32":
        f = np.float32
        lr, b1, b2 = float(f(lr)), f(beta1), f(beta2)                 # the entry point's float arguments
        bc1, bc2 = 1.0 - math.pow(float(b1), step), 1.0 - math.pow(float(b2), step)
        d = f(0.0 if ema_decay is None else ema_decay)
        return dict(lr=lr, lr_bc1=f(lr / bc1), inv_sqrt_bc2=f(1.0 / math.sqrt(bc2)), b1=b1, b2=b2, omb1=f(1.0) - b1, omb2=f(1.0) - b2,
                    eps=f(eps), gscale=f(grad_scale), d=d, one_m_d=f(1.0 - float(d)))
    if mode == "f64":
        f = np.float64
        bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
        d = 0.0 if ema_decay is None else float(ema_decay)
        return dict(lr=float(lr), lr_bc1=f(lr / bc1), inv_sqrt_bc2=f(1.0 / math.sqrt(bc2)), b1=f(beta1), b2=f(beta2), omb1=f(1.0 - beta1),
                    omb2=f(1.0 - beta2), eps=f(eps), gscale=f(grad_scale), d=f(d), one_m_d=f(1.0 - d))
    raise ValueError("mode must be 'f32' or 'f64'")


def decay_vector(n, seg_ends, seg_wd, lr, mode):
    """decay_s per element of a run of n elements: seg_ends ascending, relative to the run, the last >= n.  `lr` as host_scalars()['lr']."""
    f = np.float32 if mode == "f32" else np.float64
    out = np.empty(n, dtype=f)
    lo = 0
    for e, wd in zip(seg_ends, seg_wd):
        wd = float(np.float32(wd)) if mode == "f32" else float(wd)
        out[lo:min(e, n)] = f(1.0 - lr * wd)
        lo = min(e, n)
    assert lo == n, "the decay table does not cover the run"
    return out


def ema_warmup_decay(d, t):
    """the decay of average update number t (from 0) under ema_warmup"""
    return min(d, (1.0 + t) / (10.0 + t))


class Twin:
    """State of one run: p, m, v (and e with `ema`), stepped by step().  Arrays are copied in and never alias the caller's."""

    def __init__(self, p, mode="f32", ema=False, betas=(0.9, 0.999), eps=1e-8, m=None, v=None, e=None):
        self.mode = mode
        self.f = np.float32 if mode == "f32" else np.float64
        self.p = np.array(p, dtype=self.f)
        self.m = np.zeros_like(self.p) if m is None else np.array(m, dtype=self.f)
        self.v = np.zeros_like(self.p) if v is None else np.array(v, dtype=self.f)
        self.e = None if not ema else (self.p.copy() if e is None else np.array(e, dtype=self.f))
        self.betas, self.eps = betas, eps

    def step(self, g, lr, step, seg_ends=None, seg_wd=None, grad_scale=1.0, ema_decay=None, sel=None):
        """One update with gradient `g`; `sel` (a slice) restricts it to a contiguous run, `seg_ends` relative to the run's start."""
        sel = slice(None) if sel is None else sel
        p, m, v = self.p[sel], self.m[sel], self.v[sel]
        g = np.asarray(g, dtype=self.f)[sel]
        n = p.size
        c = host_scalars(lr, self.betas[0], self.betas[1], self.eps, step, grad_scale, ema_decay, self.mode)
        dec = decay_vector(n, [n] if seg_ends is None else seg_ends, [0.0] if seg_wd is None else seg_wd, c["lr"], self.mode)
        gr = g * c["gscale"]
        t1 = c["omb1"] * gr
        m[:] = c["b1"] * m + t1
        t2 = (c["omb2"] * gr) * gr
        v[:] = c["b2"] * v + t2
        pd = p * dec
        num = c["lr_bc1"] * m
        den = np.sqrt(v) * c["inv_sqrt_bc2"] + c["eps"]
        p[:] = pd - num / den
        assert p.dtype == self.f and gr.dtype == self.f and den.dtype == self.f
        if self.e is not None and ema_decay is not None:
            e = self.e[sel]
            t3 = c["one_m_d"] * p
            e[:] = c["d"] * e + t3


def make_case(n, seed, zeros=True):
    """p, g [3 steps] for a flat-kernel case, all in the normal range: |p| in [0.01, 2], |g| in [1e-4, 10] log-uniform with random signs
    and (with `zeros`) every 7th gradient an exact zero, so that no value the kernel forms is subnormal."""
    rng = np.random.default_rng(seed)
    p = (rng.uniform(0.01, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    gs = []
    for _ in range(3):
        g = (10.0 ** rng.uniform(-4.0, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        if zeros:
            g[rng.integers(0, 7)::7] = 0.0
        gs.append(g)
    return p, gs
