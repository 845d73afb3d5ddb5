"""The Conv3d(3,5,5) kernels (csrc/conv3d_igemm.hip, conv3d_wgrad.hip, conv3d_wgrad_wide.hip, conv3d_c1.hip) at their tile edges, against float64 references.

Most cases are integer-exact: operands are small integers, so every product and partial sum is an integer below 2^24 in any
summation order and the f32, bf16 and IEEE-half paths must all return the float64 result bit for bit (torch.equal, no
tolerance; tests/test_conv3d_edges_cpu.py asserts the conditions on these very inputs).  Branches reached here for the first
time: 16-row tiles with rows below the image, three full 14-row tiles, a 14-row tile with work for one wave only, pad 0 and its
pad-4 input gradient, the wide weight-gradient kernel's half-width K walk for every shape / tile height / operand form and at
exactly 8 and 9 columns, empty chunks, one tile per chunk, one chunk over all tiles, the first layer's pool 3 and its fused
BatchNorm weight gradient against an independent twin with a derived bound.

The fused and real-valued cases print their worst error as a fraction of the bound (`pytest -s`); profiles/conv3d_edges_gpu.txt
keeps that."""
import pytest
import torch

import conv3d_edges_cases as cs
from oracle import conv3d_ref as cref

pytestmark = pytest.mark.gpu

BF16, F32, F16 = 0, 1, 2                                   # ops.MODE_*
MODES = (F32, BF16, F16)
STORE = {BF16: torch.bfloat16, F16: torch.float16}         # 16-bit operand storage of a mode
IGEMM_CASES = [(n, ci, co) for n in cs.IGEMM_SHAPES for ci, co in cs.PAIRS]
DGRAD_CASES = [(n, ci, co) for n in cs.IGEMM_SHAPES for ci, co in cs.MODEL_PAIRS]
WGRAD_CASES = [(n, ci, co) for n in cs.WGRAD_SHAPES for ci, co in cs.MODEL_PAIRS]


def exact(got, want, what):
    """bit-for-bit agreement of a kernel result with the float64 reference"""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: got {got[idx].item()}, "
                             f"want {want[idx].item()}")


def frac(got, want, atol, rtol=0.0):
    """worst |got - want| / (atol + rtol |want|); <= 1 is np.testing.assert_allclose's criterion.  atol: number or tensor."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all())
    return float(((got - want).abs() / (atol + rtol * want.abs())).max())


def report(tag, **fracs):
    print(f"[{tag}] " + " ".join(f"{k} {v:.3f}" for k, v in fracs.items()) + " of bound", flush=True)
    bad = {k: v for k, v in fracs.items() if not v <= 1.0}
    assert not bad, f"[{tag}] exceeds its bound: {bad}"


def poison(numel):
    """Leave NaNs in the block the caching allocator hands to the next torch.empty of this size (the kernels' workspaces): a
    partial sum that is read without having been written shows.  Best effort: it relies on torch's caching allocator reusing the
    freed block and on the sizes below matching what ops.py allocates; nothing asserts that the poison landed, and without it
    the cases still check every written partial."""
    torch.full((int(numel),), float("nan"), device="cuda", dtype=torch.float32)


def mode_name(mode):
    return {F32: "f32", BF16: "bf16", F16: "f16"}[mode]


# ------------------------------------------------------------------------------------------------ 1. implicit GEMM
def _stats_exact(part, y_ref, tiles, what):
    """the fused BatchNorm partial rows: one per tile, summing (in float64) to sum y and sum y^2 per channel"""
    assert part.shape[0] == tiles, (what, part.shape, tiles)
    s = part.double().sum(0).cpu()
    exact(s[0], y_ref.sum((0, 2, 3, 4)), what + " sum y")
    exact(s[1], (y_ref * y_ref).sum((0, 2, 3, 4)), what + " sum y^2")


@pytest.mark.parametrize("name,ci,co", IGEMM_CASES)
def test_igemm_forward_is_exact(name, ci, co):
    from maavss_amd import ops
    c = cs.conv_case("igemm", name, ci, co)
    pad = c["pad"]
    x_cl, w = cs.to_cl(c["x"]).cuda(), c["w"].cuda()
    for mode in MODES:
        wt = ops.conv3d_prep(w, 0, mode)
        for xin in [x_cl] + ([x_cl.to(STORE[mode])] if mode != F32 else []):
            what = f"igemm fwd {name} {ci}->{co} {mode_name(mode)} x {str(xin.dtype)[6:]}"
            y, part = ops.conv3d_igemm(xin, wt, co, pad, mode, want_stats=True)
            exact(cs.from_cl(y), c["y"], what)
            _stats_exact(part, c["y"], cs.IGEMM_TILES[name], what)


@pytest.mark.parametrize("name,ci,co", DGRAD_CASES)
def test_igemm_input_gradient_is_exact(name, ci, co):
    """the same kernel on the flipped / transposed weight image with pad 4 - p, over the forward's output plane"""
    from maavss_amd import ops
    c = cs.conv_case("igemm", name, ci, co)
    pad = c["pad"]
    dy_cl, w = cs.to_cl(c["dy"]).cuda(), c["w"].cuda()
    for mode in MODES:
        wtd = ops.conv3d_prep(w, 1, mode)
        for din in [dy_cl] + ([dy_cl.to(STORE[mode])] if mode != F32 else []):
            dx, _ = ops.conv3d_igemm(din, wtd, ci, 4 - pad, mode)
            exact(cs.from_cl(dx), c["gx"], f"igemm dgrad {name} {ci}->{co} {mode_name(mode)} dy {str(din.dtype)[6:]}")


@pytest.mark.parametrize("ci,co", cs.PAIRS)
def test_igemm_real_valued(ci, co):
    """randn operands on the ragged 16-row-tile shape: a wrong operand conversion on a staging path that integers cannot see.
    Reference: float64 from operands rounded as the mode rounds them; tolerances of test_conv3d_igemm_fwd_dgrad_wgrad."""
    from maavss_amd import ops
    name = cs.REAL_SHAPE
    for mode in MODES:
        c = cs.real_case("igemm", name, ci, co, mode)
        pad = c["pad"]
        x_cl, w = cs.to_cl(c["x"]).cuda(), c["w"].cuda()
        wt = ops.conv3d_prep(w, 0, mode)
        fr = {}
        for xin in [x_cl] + ([x_cl.to(STORE[mode])] if mode != F32 else []):
            y, part = ops.conv3d_igemm(xin, wt, co, pad, mode, want_stats=True)
            s = part.double().sum(0)
            k = str(xin.dtype)[6:]
            fr["y_" + k] = frac(cs.from_cl(y), c["y"], 2e-4, 2e-4)
            fr["sum_" + k] = frac(s[0], c["y"].sum((0, 2, 3, 4)), 1e-2, 1e-3)
            fr["sumsq_" + k] = frac(s[1], (c["y"] * c["y"]).sum((0, 2, 3, 4)), 1e-2, 1e-3)
        if (ci, co) in cs.MODEL_PAIRS:
            wtd = ops.conv3d_prep(w, 1, mode)
            dy_cl = cs.to_cl(c["dy"]).cuda()
            for din in [dy_cl] + ([dy_cl.to(STORE[mode])] if mode != F32 else []):
                dx, _ = ops.conv3d_igemm(din, wtd, ci, 4 - pad, mode)
                fr["dx_" + str(din.dtype)[6:]] = frac(cs.from_cl(dx), c["gx"], 2e-4, 2e-4)
        report(f"igemm real {name} {ci}->{co} {mode_name(mode)}", **fr)


# ------------------------------------------------------------------------------------------------ 2. weight gradient
def _wgrad_forms(ops, ci, co, x_cl, dy_cl):
    """(label, mode, x, dy): f32, IEEE half, bf16, bf16 with a bf16 dy, and -- where the kernel takes it -- a bf16 x as well"""
    forms = [("f32", F32, x_cl, dy_cl), ("f16", F16, x_cl, dy_cl), ("bf16", BF16, x_cl, dy_cl),
             ("bf16 dy16", BF16, x_cl, dy_cl.bfloat16())]
    if (ci, co) in ops.WGRAD_X16_SHAPES:
        forms.append(("bf16 dy16 x16", BF16, x_cl.bfloat16(), dy_cl.bfloat16()))
    return forms


def _wgrad_ws(ops, c, ci, co, nchunk):
    b, t, h, w = c["dims"]
    ho, wo = h + 2 * c["pad"] - 4, w + 2 * c["pad"] - 4
    n = ops.wgrad_chunks(b, t, ho, wo, ci, co) if nchunk is None else nchunk
    return n, 75 * ci * co * n


@pytest.mark.parametrize("name,ci,co", WGRAD_CASES)
def test_wgrad_is_exact(name, ci, co):
    from maavss_amd import ops
    c = cs.conv_case("wgrad", name, ci, co)
    pad = c["pad"]
    x_cl, dy_cl = cs.to_cl(c["x"]).cuda(), cs.to_cl(c["dy"]).cuda()
    for label, mode, xin, din in _wgrad_forms(ops, ci, co, x_cl, dy_cl):
        for nchunk in cs.WGRAD_NCHUNK[name]:
            n, ws = _wgrad_ws(ops, c, ci, co, nchunk)
            poison(ws)
            dw = ops.conv3d_wgrad(xin, din, pad, mode, nchunk=nchunk)
            exact(dw, c["gw"], f"wgrad {name} {ci}->{co} {label} nchunk {nchunk} (= {n})")
        n, ws = _wgrad_ws(ops, c, ci, co, None)
        poison(ws)
        acc = ops.conv3d_wgrad(xin, din, pad, mode, dw=c["prior"].cuda(), beta=1)
        exact(acc, c["prior"].double() + c["gw"], f"wgrad {name} {ci}->{co} {label} accumulate")


def test_wgrad_default_chunks_leave_an_empty_chunk():
    """what the 11-tile shape is for: 5 chunks of 3 tiles, the fifth without a tile"""
    from maavss_amd import ops
    b, t, h, w, pad = cs.WGRAD_SHAPES["t11"]
    for ci, co in ((16, 32), (32, 64)):
        n = ops.wgrad_chunks(b, t, h + 2 * pad - 4, w + 2 * pad - 4, ci, co)
        assert n == 5 and cref.cdiv(11, n) * (n - 1) >= 11


@pytest.mark.parametrize("ci,co", cs.MODEL_PAIRS)
def test_wgrad_real_valued(ci, co):
    """randn operands on the 12-tile shape (half-width walk at exactly 8 columns, 14-row tiles), every operand form;
    tolerances of test_conv3d_igemm_fwd_dgrad_wgrad."""
    from maavss_amd import ops
    name = cs.WGRAD_REAL_SHAPE
    for mode in MODES:
        c = cs.real_case("wgrad", name, ci, co, mode)
        pad = c["pad"]
        x_cl, dy_cl = cs.to_cl(c["x"]).cuda(), cs.to_cl(c["dy"]).cuda()
        scale = float(c["gw"].abs().max())
        fr = {}
        for label, fmode, xin, din in _wgrad_forms(ops, ci, co, x_cl, dy_cl):
            if fmode != mode:
                continue
            dw = ops.conv3d_wgrad(xin, din, pad, mode)
            fr[label.replace(" ", "_")] = frac(dw, c["gw"], 2e-4 * scale + 1e-5, 2e-4)
            dw2 = ops.conv3d_wgrad(xin, din, pad, mode, dw=dw.clone(), beta=1, nchunk=3)
            fr[label.replace(" ", "_") + "_acc"] = frac(dw2, 2 * c["gw"], 4e-4 * scale + 1e-5, 2e-4)
        report(f"wgrad real {name} {ci}->{co} {mode_name(mode)}", **fr)


# ------------------------------------------------------------------------------------------------ 3. first layer
@pytest.mark.parametrize("b,t,h,w", cs.C1_SHAPES)
def test_c1_forward_and_weight_gradient_are_exact(b, t, h, w):
    from maavss_amd import ops
    from maavss_amd._lib import query
    c = cs.c1_case(b, t, h, w)
    x, wgt = c["x"].cuda(), c["w"].cuda()
    y_ref = c["y_ncdhw"]
    tiles = cref.c1_tiles(b, t, h, w)
    for mode, rows in ((F32, tiles), (F16, cref.cdiv(tiles, cref.C1_TILES_PER_WG))):
        what = f"c1 fwd {b}x{t}x{h}x{w} {mode_name(mode)}"
        assert query("maavss_conv3d_c1_fwd_nparts", b, t, h, w, mode) == rows, what
        y, part = ops.conv3d_c1_fwd(x, wgt, want_stats=True, precise=mode)
        exact(y, c["y"], what)
        _stats_exact(part, y_ref, rows, what)
    dy = c["dy"].cuda()
    for nchunk in (1, None, tiles + 1):
        poison(1200 * (nchunk or max(1, min(1024, tiles // 2))))
        dw = ops.conv3d_c1_wgrad(x, dy, nchunk=nchunk)
        exact(dw, c["gw"], f"c1 wgrad {b}x{t}x{h}x{w} nchunk {nchunk}")
    acc = ops.conv3d_c1_wgrad(x, dy, dw=c["prior"].cuda(), beta=1)
    exact(acc, c["prior"].double() + c["gw"], f"c1 wgrad {b}x{t}x{h}x{w} accumulate")


def _fused_inputs(ops, b, t, h, w, pool, conv_mode):
    """The producer chain on the GPU, as the trainer runs it: conv (f32 VALU or IEEE-half MFMA) -> BatchNorm statistics -> pool ->
    LeakyReLU -> backward coefficients; and the float64 twin of the conv-output gradient from those very tensors."""
    x, wgt, gamma, beta, dout = (v.cuda() for v in cs.c1_bn_inputs(b, t, h, w, pool))
    y, part = ops.conv3d_c1_fwd(x, wgt, want_stats=True, precise=conv_mode)
    mean, invstd = ops.bn_finalize(part, b * t * h * w)
    out, arg = ops.bn_pool_act_fwd(y, mean, invstd, gamma, beta, pool, ops.BN_LEAKY)
    dg, db = torch.zeros(16, device="cuda"), torch.zeros(16, device="cuda")
    coef = ops.bn_pool_act_bwd(dout, out, arg, y, mean, invstd, gamma, pool, ops.BN_LEAKY, dgamma=dg, dbeta=db, beta=beta,
                               coef_only=True).clone()
    dg, db = torch.zeros(16, device="cuda"), torch.zeros(16, device="cuda")
    dy16 = ops.bn_pool_act_bwd(dout, out, arg, y, mean, invstd, gamma, pool, ops.BN_LEAKY, dgamma=dg, dbeta=db, beta=beta, dy_bf16=True)
    dy64, dy_bound = cref.c1_fused_dy_f64(y.cpu(), dout.cpu(), out.cpu(), arg.cpu(), mean.cpu(), invstd.cpu(), coef.cpu(), pool)
    return dict(x=x, w=wgt, gamma=gamma, beta=beta, dout=dout, y=y, mean=mean, invstd=invstd, out=out, arg=arg, coef=coef,
                dy16=dy16.double().cpu(), dy64=dy64, dy_bound=dy_bound)


def _bf16_reference(f):
    """operands fixed first: x rounded to bf16, dy the bf16 tensor bn_pool_act_bwd writes for the same inputs; then only f32
    accumulation remains, plus one bf16 step for the (few) undecided elements"""
    und = cref.bf16_undecided(f["dy64"], f["dy_bound"])
    share = float(und.double().mean())
    assert share <= cs.UNDECIDED_MAX_SHARE, share
    # the producer's bf16 dy is a rounding of the twin's dy
    slack = f["dy_bound"] + 0.5 * torch.maximum(cref.bf16_ulp(f["dy64"]), cref.bf16_ulp(f["dy16"]))
    assert bool(((f["dy16"] - f["dy64"]).abs() <= slack).all())
    x16 = f["x"].bfloat16().double().cpu()
    return cref.c1_taps_f64(x16, f["dy16"]), cref.c1_wgrad_bn_bf16_bound(x16, f["dy16"], und), share


@pytest.mark.parametrize("b,t,h,w,pool", cs.C1_BN_CASES)
def test_c1_fused_bn_weight_gradient(b, t, h, w, pool):
    """conv3d_c1_wgrad_bn (exact f32 and bf16 MFMA) and conv3d_c1_wgrad_bn_recompute against the float64 twin of the formula in
    their loaders, within bounds derived from the float32 / bf16 formats (oracle/conv3d_ref.py); several chunkings and the
    accumulate form."""
    from maavss_amd import ops
    tiles = cref.c1_tiles(b, t, h, w)
    tag = f"c1 fused bn {b}x{t}x{h}x{w} pool {pool}"
    prior = cs.randn((16, 1, 3, 5, 5), 77)

    # --- conv output of the f32 kernel: the f32 form and the bf16 MFMA form
    f = _fused_inputs(ops, b, t, h, w, pool, F32)
    args = (f["x"], f["y"], f["dout"], f["out"], f["arg"], f["mean"], f["invstd"], f["coef"], pool)
    want = cref.c1_taps_f64(f["x"].cpu(), f["dy64"])
    bound = cref.c1_wgrad_bn_f32_bound(f["x"].cpu(), f["dy64"], f["dy_bound"])
    fr = {}
    for nchunk in (None, 1, 5, tiles + 1):
        poison(1200 * (nchunk or max(1, min(1024, tiles // 2))))
        fr[f"f32_n{nchunk}"] = frac(ops.conv3d_c1_wgrad_bn(*args, nchunk=nchunk), want, bound)
    acc = ops.conv3d_c1_wgrad_bn(*args, dw=prior.cuda(), beta=1)
    fr["f32_acc"] = frac(acc, want + prior.double(), bound + cref.U * (want + prior.double()).abs())
    want16, bound16, share = _bf16_reference(f)
    for nchunk in (None, 1, 5, tiles + 1):
        poison(1200 * (nchunk or max(1, min(1024, tiles // 2))))
        fr[f"bf16_n{nchunk}"] = frac(ops.conv3d_c1_wgrad_bn(*args, nchunk=nchunk, precise=BF16), want16, bound16)
    acc = ops.conv3d_c1_wgrad_bn(*args, dw=prior.cuda(), beta=1, precise=BF16)
    fr["bf16_acc"] = frac(acc, want16 + prior.double(), bound16 + cref.U * (want16 + prior.double()).abs())
    report(tag + f" (f32 conv output, undecided {share:.4f})", **fr)

    # --- conv output of the IEEE-half MFMA kernel: the bf16 MFMA form again and the form that recomputes that output per tile
    f = _fused_inputs(ops, b, t, h, w, pool, F16)
    args = (f["x"], f["y"], f["dout"], f["out"], f["arg"], f["mean"], f["invstd"], f["coef"], pool)
    rargs = (f["x"], f["w"], f["dout"], f["arg"], f["mean"], f["invstd"], f["beta"], f["coef"], pool)
    want16, bound16, share = _bf16_reference(f)
    fr = {}
    for nchunk in (None, 1, 5, tiles + 1):
        poison(1200 * (nchunk or max(1, min(1024, tiles // 2))))
        fr[f"bf16_n{nchunk}"] = frac(ops.conv3d_c1_wgrad_bn(*args, nchunk=nchunk, precise=BF16), want16, bound16)
        poison(1200 * (nchunk or max(1, min(1024, tiles // 2))))
        fr[f"recompute_n{nchunk}"] = frac(ops.conv3d_c1_wgrad_bn_recompute(*rargs, nchunk=nchunk), want16, bound16)
    acc = ops.conv3d_c1_wgrad_bn_recompute(*rargs, dw=prior.cuda(), beta=1)
    fr["recompute_acc"] = frac(acc, want16 + prior.double(), bound16 + cref.U * (want16 + prior.double()).abs())
    report(tag + f" (f16 conv output, undecided {share:.4f})", **fr)


@pytest.mark.parametrize("b,t,h,w,pool", cs.C1_BN_CASES)
def test_c1_fused_bn_weight_gradient_from_the_stored_and_the_recomputed_output_is_bit_identical(b, t, h, w, pool):
    """The two instantiations of conv3d_c1_wgrad_mfma_kernel -- y read from memory, y recomputed per tile -- form the same product
    in the same order: on the IEEE-half MFMA forward's y (what the recompute reproduces; the sign of `out` and of the recomputed
    pre-activation agree through bn_act.h) they return the same bits.  Partial tiles in both directions, a pool window cut off at
    the border, pool 3, and an empty chunk (tiles + 1 chunks) on poisoned workspaces."""
    from maavss_amd import ops
    tiles = cref.c1_tiles(b, t, h, w)
    f = _fused_inputs(ops, b, t, h, w, pool, F16)
    args = (f["x"], f["y"], f["dout"], f["out"], f["arg"], f["mean"], f["invstd"], f["coef"], pool)
    rargs = (f["x"], f["w"], f["dout"], f["arg"], f["mean"], f["invstd"], f["beta"], f["coef"], pool)
    for nchunk in (None, 1, tiles + 1):
        poison(1200 * (nchunk or max(1, min(1024, tiles // 2))))
        stored = ops.conv3d_c1_wgrad_bn(*args, nchunk=nchunk, precise=BF16)
        poison(1200 * (nchunk or max(1, min(1024, tiles // 2))))
        recomputed = ops.conv3d_c1_wgrad_bn_recompute(*rargs, nchunk=nchunk)
        assert bool(torch.isfinite(stored).all()), f"c1 fused bn {b}x{t}x{h}x{w} pool {pool} nchunk {nchunk}: not finite"
        assert torch.equal(stored, recomputed), (f"c1 fused bn {b}x{t}x{h}x{w} pool {pool} nchunk {nchunk}: "
                                                 f"{int((stored != recomputed).sum())} of 1200 elements differ")


def test_c1_fused_bn_rejects_other_pools():
    """the entry points admit pool 2 and 3 only (c1_pdiv divides by nothing else)"""
    from maavss_amd import ops
    from maavss_amd._lib import MaavssError
    b, t, h, w, pool = cs.C1_BN_CASES[0]
    f = _fused_inputs(ops, b, t, h, w, pool, F32)
    for bad in (1, 4):
        with pytest.raises(MaavssError, match="pool must be 2 or 3"):
            ops.conv3d_c1_wgrad_bn(f["x"], f["y"], f["dout"], f["out"], f["arg"], f["mean"], f["invstd"], f["coef"], bad)
        with pytest.raises(MaavssError, match="pool must be 2 or 3"):
            ops.conv3d_c1_wgrad_bn_recompute(f["x"], f["w"], f["dout"], f["arg"], f["mean"], f["invstd"], f["beta"], f["coef"], bad)
