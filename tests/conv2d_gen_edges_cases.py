"""Shapes, inputs and float64 references shared by test_conv2d_gen_edges_cpu.py (which checks the references and the exactness
conditions) and test_conv2d_gen_edges_gpu.py (which holds the generic convolution kernels of csrc/conv2d_gen.hip to them).

Operands are small integers (|S|, |G| <= 2, |w| <= 1, a prior dw with |dw| <= 3), so every product and every partial sum is an
integer far below 2^24 in any summation order and the f32 kernels must return the float64 result bit for bit.  Logical tensors
are NCHW; `store` / `load` move them into and out of the storage layouts the kernels address through ops.Map."""
import functools

import torch
import torch.nn.functional as F

SENTINEL = 7.0      # what written maps hold beforehand: the padded channels must still hold it afterwards
EXACT_BELOW = float(1 << 24)

# name: B, Cs, Hs, Ws, Cb, kernel, stride, pad, output_padding, small layout, big layout
# layouts: "nhwc", "nchw", "pad4" = channels-last with 4 channels allocated (what the BatchNorm kernels take for c = 2)
CASES = {
    # the tap limit: the STFT decoder's (3,10) layer
    "taps30": (2, 3, 5, 7, 2, (3, 10), (1, 2), (1, 4), (0, 1), "nhwc", "nhwc"),
    # weight-gradient chunks: one per 4096 small-map positions, split evenly -- 4096 = one chunk; 4097 = 2049 + 2048, the last
    # position of the map closing the second chunk; 4160 = 2080 + 2080, both ending in a pass with 32 of the 256 threads at work;
    # 200 = one chunk shorter than a single pass of the 256 threads
    "pos200": (1, 2, 10, 20, 2, (3, 9), (1, 1), (1, 4), (0, 0), "nhwc", "nhwc"),
    "pos4096": (1, 2, 64, 64, 2, (3, 9), (1, 1), (1, 4), (0, 0), "nhwc", "nhwc"),
    "pos4097": (1, 2, 17, 241, 2, (3, 9), (1, 1), (1, 4), (0, 0), "nhwc", "nhwc"),
    "pos4160": (1, 2, 64, 65, 2, (3, 9), (1, 1), (1, 4), (0, 0), "nhwc", "nhwc"),
    # the decoder's layouts: a channel-padded activation into the network's NCHW output (last layer), a dense activation into a
    # channel-padded one (the 2-channel BatchNorm layer), one channel each way
    "pad_to_nchw": (2, 2, 4, 6, 2, (3, 9), (2, 2), (1, 4), (1, 1), "pad4", "nchw"),
    "nhwc_to_pad": (2, 4, 3, 5, 2, (3, 10), (1, 2), (1, 4), (0, 1), "nhwc", "pad4"),
    "one_channel": (3, 1, 4, 5, 1, (3, 9), (2, 1), (1, 4), (1, 0), "pad4", "nchw"),
}
CHUNK_CASES = {"pos200": 1, "pos4096": 1, "pos4097": 2, "pos4160": 2}      # expected maavss_conv2d_gen_wgrad_nchunk
LAYOUT_CASES = ("pad_to_nchw", "nhwc_to_pad", "one_channel")


def ints(shape, lo, hi, seed):
    """integers lo..hi (inclusive) as float32"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=torch.Generator().manual_seed(seed)).float()


def big_size(hs, ws, kernel, stride, pad, opad):
    return tuple((n - 1) * s - 2 * p + k + o for n, k, s, p, o in zip((hs, ws), kernel, stride, pad, opad))


def store(x, layout, fill=0.0):
    """logical NCHW tensor -> (storage tensor, keyword arguments of ops.Map)"""
    if layout == "nchw":
        return x.contiguous(), dict(nchw=True)
    x = x.permute(0, 2, 3, 1)
    if layout == "nhwc":
        return x.contiguous(), {}
    c = x.shape[-1]
    t = torch.full((*x.shape[:3], 4), fill, dtype=x.dtype)
    t[..., :c] = x
    return t, dict(c=c)


def load(t, layout, c):
    """storage tensor -> (logical NCHW tensor, the padded channels or None)"""
    if layout == "nchw":
        return t, None
    return t[..., :c].permute(0, 3, 1, 2), (t[..., c:] if layout == "pad4" else None)


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs (float32) and float64 references of a case, computed once; `bound` = the largest sum |a||b| over every result"""
    b, cs, hs, ws, cb, kernel, stride, pad, opad, lay_s, lay_g = CASES[name]
    hb, wb = big_size(hs, ws, kernel, stride, pad, opad)
    seed = sorted(CASES).index(name) * 10
    s, g = ints((b, cs, hs, ws), -2, 2, seed), ints((b, cb, hb, wb), -2, 2, seed + 1)
    w, dw0 = ints((cs, cb, *kernel), -1, 1, seed + 2), ints((cs, cb, *kernel), -3, 3, seed + 3)
    s64, g64, w64 = s.double(), g.double(), w.double()

    def big(sv, wv):
        return F.conv_transpose2d(sv, wv, stride=stride, padding=pad, output_padding=opad)

    def small(gv, wv):
        return F.conv2d(gv, wv, stride=stride, padding=pad)

    def wgrad(sv, gv):
        return torch.nn.grad.conv2d_weight(gv, (cs, cb, *kernel), sv, stride=stride, padding=pad)

    bound = max(float(big(s64.abs(), w64.abs()).max()), float(small(g64.abs(), w64.abs()).max()),
                float((wgrad(s64.abs(), g64.abs()) + dw0.double().abs()).max()))
    return dict(b=b, cs=cs, cb=cb, kernel=kernel, stride=stride, pad=pad, opad=opad, lay_s=lay_s, lay_g=lay_g, hs=hs, ws=ws, hb=hb, wb=wb,
                s=s, g=g, w=w, dw0=dw0, big=big(s64, w64), small=small(g64, w64), dw=wgrad(s64, g64), bound=bound)
