"""CPU side of test_conv2d_edges_gpu.py: the float64 references of conv2d_edges_cases.py are right, the integer inputs meet the
condition under which an f32 kernel must reproduce them bit for bit, and the cases cover what their names say."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv2d_edges_cases as cs
from maavss_amd import _lib


@pytest.mark.parametrize("name", sorted(cs.CASES))
def test_references_and_exactness_conditions(name):
    c = cs.case(name)
    assert c["bound"] < cs.EXACT_BELOW, (name, c["bound"])
    assert c["bound"] <= 4 * 1025 + 3                   # what the module's docstring promises: "far below 2^24"
    for t in (c["x"], c["dy"], c["wt"], c["dw0"], c["y"], c["dx"], c["dw"]):
        assert torch.equal(t, t.round())
    assert c["x"].abs().max() <= 2 and c["dy"].abs().max() <= 2 and c["wt"].abs().max() <= 1 and c["dw0"].abs().max() <= 3
    assert c["y"].shape == c["dy"].shape and c["dx"].shape == c["x"].shape and c["dw"].shape == c["wt"].shape
    # the two gradients by another route: autograd through the convolution, which is linear in both operands
    x, w = c["x"].double().requires_grad_(), c["wt"].double().requires_grad_()
    (F.conv2d(x, w, stride=c["stride"], padding=(1, c["pw"])) * c["dy"].double()).sum().backward()
    assert torch.equal(x.grad, c["dx"]) and torch.equal(w.grad, c["dw"])
    # ... and the forward from its definition  y[b, co, oy, ox] = sum x[b, ci, oy*sh - 1 + kh, ox*sw - pw + kw] * w[co, ci, kh, kw]
    (sh, sw), pw = c["stride"], c["pw"]
    xp = torch.zeros(c["b"], c["ci"], c["h"] + 2 + sh, c["w"] + 2 * pw + sw, dtype=torch.float64)
    xp[:, :, 1:1 + c["h"], pw:pw + c["w"]] = c["x"].double()
    want = torch.zeros_like(c["y"])
    for kh in range(3):
        for kw in range(9):
            want += torch.einsum("bihw,oi->bohw", xp[:, :, kh:kh + sh * c["ho"]:sh, kw:kw + sw * c["wo"]:sw], c["wt"][:, :, kh, kw].double())
    assert torch.equal(want, c["y"])


def test_every_tap_clips_at_every_border():
    """maps of 3-5 rows and 17-21 columns: the first and last output positions lose taps on each side, at every stride"""
    for name in cs.TUNED_CASES + cs.REFUSED_CASES:
        c = cs.case(name)
        assert c["b"] == 2 and 3 <= c["h"] <= 5 and 17 <= c["w"] <= 21, name
        (sh, sw), pw = c["stride"], c["pw"]
        assert (c["ho"] - 1) * sh + 1 >= c["h"] and (c["wo"] - 1) * sw - pw + 8 >= c["w"], name      # the last row / column reaches the padding


def test_cases_cover_the_tuned_and_the_refused_shapes():
    tuned = {(c["ci"], c["co"], c["stride"], c["pw"], c["nchw"]) for c in map(cs.case, cs.TUNED_CASES)}
    for ci, co in ((2, 4), (4, 8), (8, 16), (16, 16)):
        for st in cs.STRIDES:
            for pw in (3, 4):
                assert (ci, co, st, pw, False) in tuned and ((ci, co, st, pw, True) in tuned) == (ci == 2)
    assert {(c["ci"], c["co"]) for c in map(cs.case, cs.REFUSED_CASES)} == {(3, 6), (32, 16), (4, 32)}


def test_chunk_counts_are_the_ones_the_cases_are_named_for():
    """the row kernel's weight gradient: one partial per 1024 positions, 1025 positions = 2 chunks of 513 + 512; a shape it refuses runs the
    generic kernel, whose chunks hold 4096 positions (test_conv2d_gen_edges_cpu.py pins those boundaries).  Read off the size of the
    workspace, which holds one partial dw per chunk of whichever kernel the call launches."""
    def nhwc(h, w, c_alloc):
        return (ctypes.c_int64 * 4)(h * w * c_alloc, w * c_alloc, c_alloc, 1)

    for name in cs.CHUNK_CASES:
        c = cs.case(name)
        npos = c["b"] * c["ho"] * c["wo"]
        assert npos == int(name.split("pos")[1])
        y, x = nhwc(c["ho"], c["wo"], c["co"]), nhwc(c["h"], c["w"], c["ci"])
        nbytes = _lib.query("maavss_conv2d_gen_wgrad_ws_bytes", c["b"], c["co"], c["ho"], c["wo"], c["ci"], c["h"], c["w"], 3, 9, *c["stride"], 1, c["pw"],
                            y, x)
        tuned = name.startswith("tuned")
        assert nbytes == (2 if tuned and npos == 1025 else 1) * c["wt"].numel() * 4, name
        assert _lib.query("maavss_conv2d_gen_wgrad_nchunk", c["b"], c["ho"], c["wo"]) == 1
        # the same geometry with a channel-padded input is not the row kernel's: the generic kernel's single chunk
        assert _lib.query("maavss_conv2d_gen_wgrad_ws_bytes", c["b"], c["co"], c["ho"], c["wo"], c["ci"], c["h"], c["w"], 3, 9, *c["stride"], 1, c["pw"],
                          y, nhwc(c["h"], c["w"], c["ci"] + 4)) == c["wt"].numel() * 4, name
