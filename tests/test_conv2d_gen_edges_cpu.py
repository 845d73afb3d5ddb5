"""CPU side of test_conv2d_gen_edges_gpu.py: the float64 references of conv2d_gen_edges_cases.py are right, and the integer
inputs meet the condition under which an f32 kernel must reproduce them bit for bit."""
import pytest
import torch
import torch.nn.functional as F

import conv2d_gen_edges_cases as cs
from maavss_amd import _lib


@pytest.mark.parametrize("name", sorted(cs.CASES))
def test_references_and_exactness_conditions(name):
    c = cs.case(name)
    assert c["bound"] < cs.EXACT_BELOW, (name, c["bound"])
    assert c["bound"] <= 4 * 4160 + 3                   # what the module's docstring promises: "far below 2^24"
    for t in (c["s"], c["g"], c["w"], c["dw0"], c["big"], c["small"], c["dw"]):
        assert torch.equal(t, t.round())
    assert c["s"].abs().max() <= 2 and c["g"].abs().max() <= 2 and c["w"].abs().max() <= 1
    assert c["big"].shape == c["g"].shape and c["small"].shape == c["s"].shape and c["dw"].shape == c["w"].shape
    # the same three results by another route: autograd through the transposed convolution, which is linear in both operands
    s, w = c["s"].double().requires_grad_(), c["w"].double().requires_grad_()
    (F.conv_transpose2d(s, w, stride=c["stride"], padding=c["pad"], output_padding=c["opad"]) * c["g"].double()).sum().backward()
    assert torch.equal(s.grad, c["small"]) and torch.equal(w.grad, c["dw"])
    # ... and the forward from its definition  G[b, cb, sy*sh - ph + kh, sx*sw - pw + kw] += S[b, cs, sy, sx] * w[cs, cb, kh, kw]
    (ph, pw), (sh, sw) = c["pad"], c["stride"]
    want = torch.zeros(c["b"], c["cb"], c["hb"] + 2 * ph + sh, c["wb"] + 2 * pw + sw, dtype=torch.float64)
    for kh in range(c["kernel"][0]):
        for kw in range(c["kernel"][1]):
            want[:, :, kh:kh + sh * c["hs"]:sh, kw:kw + sw * c["ws"]:sw] += torch.einsum("bshw,sc->bchw", c["s"].double(), c["w"][:, :, kh, kw].double())
    assert torch.equal(want[:, :, ph:ph + c["hb"], pw:pw + c["wb"]], c["big"])


def test_chunk_counts_are_the_ones_the_cases_are_named_for():
    for name, nchunk in cs.CHUNK_CASES.items():
        c = cs.case(name)
        assert c["b"] * c["hs"] * c["ws"] == int(name[3:])
        assert _lib.query("maavss_conv2d_gen_wgrad_nchunk", c["b"], c["hs"], c["ws"]) == nchunk
