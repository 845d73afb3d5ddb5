"""Shapes, inputs and float64 references shared by test_conv2d_edges_cpu.py (which checks the references and the exactness
conditions) and test_conv2d_edges_gpu.py (which holds the STFT encoder's Conv2d(k=(3,9), pad (1,pw), bias=False) kernels -- the
position / row kernels of csrc/conv2d.hip and the generic kernels that serve the shapes those refuse -- to them).

Operands are small integers (|x|, |dy| <= 2, |w| <= 1, a prior dw with |dw| <= 3), so every product and every partial sum is an
integer far below 2^24 in any summation order and the f32 kernels must return the float64 result bit for bit.  Maps are a few
rows high and an odd number of columns wide, so every tap clips at every border.  Logical tensors are NCHW."""
import functools

import torch
import torch.nn.functional as F

EXACT_BELOW = float(1 << 24)
STRIDES = ((1, 1), (2, 2), (1, 2), (2, 1))

# name: B, C_in, H, W, C_out, stride, pw, input stored NCHW
CASES = {}
# the channel pairs of the STFT encoder, which the tuned kernels take: every stride, both paddings, both input layouts where the
# first layer allows it (the network input is NCHW with C_in = 2)
for _n, (_ci, _co) in enumerate(((2, 4), (4, 8), (8, 16), (16, 16))):
    for _s, _st in enumerate(STRIDES):
        for _pw in (3, 4):
            # an odd height under a row stride of 2, so that the last output row still reaches the bottom padding
            _h, _w = (3 + (_n + _s) % 3) if _st[0] == 1 else (3, 5)[(_n + _s) % 2], 17 + (2 * _s + _pw + _n) % 5
            for _nchw in ((False, True) if _ci == 2 else (False,)):
                CASES[f"tuned_{_ci}_{_co}_s{_st[0]}{_st[1]}_p{_pw}_{'nchw' if _nchw else 'nhwc'}"] = (2, _ci, _h, _w, _co, _st, _pw, _nchw)
TUNED_CASES = tuple(CASES)
# shapes the tuned kernels refuse: C_out = 6 (no tuned kernel at all), C_in = 32 (forward and input gradient: the LDS weight image
# holds 16 input channels), C_out = 32 (input gradient and weight gradient)
for _ci, _co in ((3, 6), (32, 16), (4, 32)):
    for _s, _st in enumerate(STRIDES):
        CASES[f"refused_{_ci}_{_co}_s{_st[0]}{_st[1]}_p{3 + _s % 2}"] = (2, _ci, (3, 5, 4, 5)[_s], 17 + 2 * (_s % 3), _co, _st, 3 + _s % 2, False)
REFUSED_CASES = tuple(n for n in CASES if n.startswith("refused"))
# weight-gradient chunks of the tuned kernel: one per 1024 output positions, split evenly -- 1024 = one chunk; 1025 = 513 + 512
CASES.update({
    "tuned_pos1024": (2, 4, 4, 128, 8, (1, 1), 4, False),
    "tuned_pos1025": (5, 4, 5, 41, 8, (1, 1), 4, False),
    "refused_pos1024": (2, 3, 4, 128, 6, (1, 1), 4, False),
    "refused_pos1025": (5, 3, 5, 41, 6, (1, 1), 4, False),
})
CHUNK_CASES = ("tuned_pos1024", "tuned_pos1025", "refused_pos1024", "refused_pos1025")
del _n, _ci, _co, _s, _st, _pw, _h, _w, _nchw


def ints(shape, lo, hi, seed):
    """integers lo..hi (inclusive) as float32"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=torch.Generator().manual_seed(seed)).float()


def out_size(h, w, stride, pw):
    return (h + 2 - 3) // stride[0] + 1, (w + 2 * pw - 9) // stride[1] + 1


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs (float32) and float64 references of a case, computed once; `bound` = the largest sum |a||b| over every result"""
    b, ci, h, w, co, stride, pw, nchw = CASES[name]
    ho, wo = out_size(h, w, stride, pw)
    seed = 1000 + sorted(CASES).index(name) * 10
    x, dy = ints((b, ci, h, w), -2, 2, seed), ints((b, co, ho, wo), -2, 2, seed + 1)
    wt, dw0 = ints((co, ci, 3, 9), -1, 1, seed + 2), ints((co, ci, 3, 9), -3, 3, seed + 3)
    x64, dy64, w64 = x.double(), dy.double(), wt.double()

    def fwd(xv, wv):
        return F.conv2d(xv, wv, stride=stride, padding=(1, pw))

    def dgrad(dv, wv):
        return torch.nn.grad.conv2d_input((b, ci, h, w), wv, dv, stride=stride, padding=(1, pw))

    def wgrad(xv, dv):
        return torch.nn.grad.conv2d_weight(xv, (co, ci, 3, 9), dv, stride=stride, padding=(1, pw))

    bound = max(float(fwd(x64.abs(), w64.abs()).max()), float(dgrad(dy64.abs(), w64.abs()).max()),
                float((wgrad(x64.abs(), dy64.abs()) + dw0.double().abs()).max()))
    return dict(b=b, ci=ci, h=h, w=w, co=co, ho=ho, wo=wo, stride=stride, pw=pw, nchw=nchw, x=x, dy=dy, wt=wt, dw0=dw0,
                y=fwd(x64, w64), dx=dgrad(dy64, w64), dw=wgrad(x64, dy64), bound=bound)
