"""What test_bn_pool_edges_gpu.py relies on, shown on exactly its inputs without a GPU: the statistics' partial sums are exact
integers, a dropped or doubled row moves the mean by far more than the accepted ulp, the tie-rich pool inputs cannot collide after
normalisation in float32, the reference argmax (float64 F.max_pool3d) is the first maximum in dy * P + dx order, the written-out
backward pass agrees with float64 autograd, and a dropped pooled position moves dgamma and dbeta beyond their tolerances."""
import pytest
import torch
import torch.nn.functional as F

import bn_pool_edges_cases as cs
from oracle import dense_edges_ref as dref


def beyond(delta, want, tol):
    """|delta| exceeds what assert_allclose(rtol, atol) accepts around `want`"""
    return delta.abs() > tol[1] + tol[0] * want.abs()


# ---------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("rows,c", cs.STATS_CASES)
def test_statistics_sums_are_exact_integers_and_the_reference_is_torchs(rows, c):
    y, rm0, rv0 = cs.stats_input(rows, c)
    assert torch.equal(y, y.round()) and float(y.min()) >= -4 and float(y.max()) <= 6
    nblk = cs.stats_nblk(rows)
    rpb = -(-rows // nblk)
    # whatever order a workgroup adds its rows in, no partial sum or sum of squares leaves the exact integers of float32
    assert rpb * 36 < 2 ** 24
    for blk in (0, nblk - 1):
        rows_of = y[blk * rpb:min(rows, (blk + 1) * rpb)]
        assert float((rows_of * rows_of).sum(0).max()) < 2 ** 24 and float(rows_of.abs().sum(0).max()) < 2 ** 24
    s1, s2 = dref.bn_sums_f64(y)
    assert float(s2.max()) < 2 ** 53
    assert torch.equal(y.sum(0, dtype=torch.float64), s1)
    mean, invstd, rm, rv = cs.stats_reference(rows, c)
    if rows > 1:
        rm_t, rv_t = rm0.double(), rv0.double()
        F.batch_norm(y.double(), rm_t, rv_t, training=True, momentum=cs.MOMENTUM, eps=cs.EPS)      # torch's own running update
        torch.testing.assert_close(rm.double(), rm_t, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(rv.double(), rv_t, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(mean.double(), y.double().mean(0), rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(invstd.double(), 1 / torch.sqrt(y.double().var(0, unbiased=False) + cs.EPS), rtol=1e-6, atol=0)
    else:
        assert torch.equal(mean, y[0]) and torch.equal(invstd, torch.full((c,), float(1 / torch.tensor(cs.EPS, dtype=torch.float32).double().sqrt())).float())


@pytest.mark.parametrize("rows,c", cs.STATS_CASES)
def test_a_dropped_or_doubled_row_moves_the_mean_by_many_ulp(rows, c):
    y, rm0, rv0 = cs.stats_input(rows, c)
    mean = cs.stats_reference(rows, c)[0]
    seen = (y != 0).any(0)                # channels in which some row has a non-zero entry: all of them, unless there is one row
    assert bool(seen.all()) if rows > 1 else bool(seen.any())
    s1, s2 = dref.bn_sums_f64(y)
    for v in (-1.0, 1.0):      # the smallest non-zero entry a lost (-) or repeated (+) row can hold
        m2 = dref.bn_finalize_f64(s1 + v, s2 + v * v, float(rows), cs.EPS, cs.MOMENTUM)[0].float()
        assert int(dref.ulp_distance(m2, mean)[seen].min()) >= 4 * (cs.MAX_ULP + 1), (rows, c)


@pytest.mark.parametrize("nblk,c", cs.TWO_LEVEL_CASES)
def test_two_level_partials_stay_exact(nblk, c):
    part = cs.two_level_partials(nblk, c)
    assert nblk > 512 and tuple(part.shape) == (nblk, 2, c) and torch.equal(part, part.round())
    assert float(part.abs().sum(0).max()) < 2 ** 24          # every subtotal of the first level is a float32 integer
    mean, invstd, rm, rv = cs.two_level_reference(nblk, c)
    var = part[:, 1].double().sum(0) / cs.TWO_LEVEL_COUNT - mean.double() ** 2
    assert float(var.min()) > 1.0
    # one dropped partial row shows
    s1, s2 = part[:, 0].double().sum(0), part[:, 1].double().sum(0)
    inv2 = dref.bn_finalize_f64(s1 - part[-1, 0].double(), s2 - part[-1, 1].double(), float(cs.TWO_LEVEL_COUNT), cs.EPS, cs.MOMENTUM)[1].float()
    assert int(dref.ulp_distance(inv2, invstd).min()) >= 4 * (cs.MAX_ULP + 1)


def test_ulp_distance():
    a = torch.tensor([1.0, -1.0, 0.0, 3.5], dtype=torch.float32)
    b = torch.nextafter(a, torch.tensor([2.0, -2.0, 1.0, 0.0]))
    assert dref.ulp_distance(a, a).tolist() == [0, 0, 0, 0] and dref.ulp_distance(a, b).tolist() == [1, 1, 1, 1]
    assert dref.ulp_distance(torch.tensor([-0.0]), torch.tensor([0.0])).item() == 0


# ---------------------------------------------------------------------------------------------- forward
FWD_VARIANTS = [(p, sg, bs) for p in cs.POOL_CASES for sg, bs in ((False, False), (False, True), (True, True))]


@pytest.mark.parametrize("p,small_gamma,batch_stats", FWD_VARIANTS, ids=[f"{p.tag}-{int(sg)}{int(bs)}" for p, sg, bs in FWD_VARIANTS])
def test_pool_inputs_tie_often_and_cannot_collide_in_float32(p, small_gamma, batch_stats):
    d = cs.pool_input(p, small_gamma, batch_stats)
    y, gamma = d["y"], d["gamma"]
    assert torch.equal(y * 8, (y * 8).round()) and float(y.abs().max()) <= 2
    assert bool((gamma > 0).any()) and bool((gamma < 0).any())
    assert float(gamma.abs().min()) >= (1e-3 if small_gamma else 0.5)
    if small_gamma:
        assert float(gamma[1].abs()) < 1e-2
    # distinct grid values stay strictly ordered after the kernel's float32 normalisation, in the direction of gamma's sign: with
    # two roundings (v * sc + sh) and with one (fused multiply-add); equal values tie exactly by construction
    g = cs.grid_values()
    sc = d["gamma"] * d["invstd"]
    sh = d["beta"] - d["mean"] * sc
    two = g[:, None] * sc[None, :] + sh[None, :]
    one = (g.double()[:, None] * sc.double()[None, :] + sh.double()[None, :]).float()
    for v in (two, one):
        step = (v[1:] - v[:-1]) * torch.sign(sc)[None, :]
        assert bool((step > 0).all())
    if p.pool > 1:
        z = dref.bn_normalise_f64(y, d["mean"], d["invstd"], d["gamma"], d["beta"])
        share = dref.max_ties(z, p.pool)
        assert share >= (1.0 if p.blocks else 0.25 if p.pool == 2 else 0.5), share
        # the reference argmax (float64 F.max_pool3d) is the first maximum in dy * P + dx order
        out, arg = cs.fwd_reference(p, small_gamma, batch_stats)
        assert arg.dtype == torch.uint8 and torch.equal(arg, dref.first_max_offsets(z, p.pool))
        if p.blocks:
            assert int(arg.max()) == 0
        else:
            assert len(arg.unique()) > 2
    else:
        out, arg = cs.fwd_reference(p, small_gamma, batch_stats)
        assert arg is None
    assert tuple(out.shape) == (p.b, p.t, p.h // p.pool, p.w // p.pool, p.c)


def test_the_wrap_case_wraps_both_row_walks():
    p = cs.POOL_CASES[-1]
    assert p.b * p.t == 33 and p.b * p.t * (p.h // p.pool) > 4096 and p.b * p.t * p.h > 4096


# ---------------------------------------------------------------------------------------------- backward
BWD_VARIANTS = [(p, sg) for p in cs.POOL_CASES + (cs.STRIDED,) for sg in (False, True)]


@pytest.mark.parametrize("p,small_gamma", BWD_VARIANTS, ids=[f"{p.tag}-{int(sg)}" for p, sg in BWD_VARIANTS])
def test_written_out_backward_agrees_with_autograd_and_a_dropped_position_shows(p, small_gamma):
    d = cs.pool_input(p, small_gamma, True)
    ref = cs.bwd_reference(p, small_gamma)
    out64, arg = cs.fwd_reference(p, small_gamma, True)
    # LeakyReLU's kink: no pre-activation value close enough to zero for float32 and float64 to disagree about its side
    if p.act == cs.LEAKY:
        assert float(ref["zp"].abs().min()) > cs.MIN_Z
    out_a, gy, gg, gb, mean64, invstd64 = dref.bn_pool_act_autograd_f64(d["dout"], d["y"], d["gamma"], d["beta"], p.pool, p.act, cs.EPS)
    # the statistics handed to the kernels are the batch's own, rounded to float32
    torch.testing.assert_close(d["mean"].double(), mean64, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(d["invstd"].double(), invstd64, rtol=1e-6, atol=0)
    # the same formula on the unrounded statistics is autograd's result to double rounding ...
    exact = dref.bn_pool_act_bwd_f64(d["dout"], d["y"], mean64, invstd64, d["gamma"], d["beta"], p.pool, p.act, arg)
    torch.testing.assert_close(exact["dy"], gy, rtol=1e-9, atol=1e-10)
    torch.testing.assert_close(exact["dgamma"], gg, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(exact["dbeta"], gb, rtol=1e-9, atol=1e-9)
    # ... and rounding them to float32 moves it by a small part of the tolerances of test_bn_pool_act
    assert not bool(beyond(4 * (ref["dy"] - gy), gy, cs.DY_TOL).any())
    assert not bool(beyond(4 * (ref["dgamma"] - gg), gg, cs.DPARAM_TOL).any())
    assert not bool(beyond(4 * (ref["dbeta"] - gb), gb, cs.DPARAM_TOL).any())
    assert not bool(beyond(4 * (out64 - out_a), out_a, cs.OUT_TOL).any())
    # one dropped pooled position (the one whose gradient weighs most) moves dgamma and dbeta beyond their tolerances
    xhat = (d["y"].double() - d["mean"].double()) * d["invstd"].double()
    g = ref["g_full"]
    assert bool(beyond(g.abs().amax((0, 1, 2, 3)), ref["dbeta"], cs.DPARAM_TOL).all())
    assert bool(beyond((g * xhat).abs().amax((0, 1, 2, 3)), ref["dgamma"], cs.DPARAM_TOL).all())


@pytest.mark.parametrize("p", cs.ROUTING_CASES, ids=[p.tag for p in cs.ROUTING_CASES])
def test_single_position_gradient_lands_on_one_input_per_channel(p):
    ref = cs.routing_reference(p)
    _, arg = cs.fwd_reference(p, False, True)
    routed = ref["dy"] - ref["dense"]
    hit = routed != 0
    assert int(hit.sum()) == p.c and tuple(hit.sum((0, 1, 2, 3)).tolist()) == (1,) * p.c
    # ... and it is the argmax position of the last window
    hp, wp = p.h // p.pool, p.w // p.pool
    for ch in range(p.c):
        a = int(arg[-1, -1, -1, -1, ch])
        assert bool(hit[-1, -1, (hp - 1) * p.pool + a // p.pool, (wp - 1) * p.pool + a % p.pool, ch])
    # the routed value stands far above what float32 rounding leaves elsewhere (dy's tolerance)
    assert bool((routed[hit].abs() > 100 * (cs.DY_TOL[1] + cs.DY_TOL[0] * ref["dy"][hit].abs())).all())
    # the last window's maximum is tied in some channel: routing to another of the tied positions would show
    d = cs.pool_input(p, False, True)
    z = dref.bn_normalise_f64(d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"])
    win = z[-1, -1, (hp - 1) * p.pool:hp * p.pool, (wp - 1) * p.pool:wp * p.pool].reshape(p.pool * p.pool, p.c)
    assert bool(((win == win.max(0, keepdim=True).values).sum(0) > 1).any())


def test_sequence_buffer_layout():
    p = cs.STRIDED
    pooled = torch.arange(p.b * p.t * 2 * 2 * p.c).float().view(p.b, p.t, 2, 2, p.c)
    seq = cs.to_seq(pooled, float("nan"))
    sb, st, sp, sc = cs.seq_strides(p)
    flat = seq.view(-1)
    for b, t, pos, ch in ((0, 0, 0, 0), (1, 3, 3, 15), (1, 2, 1, 7)):
        assert flat[b * sb + t * st + pos * sp + ch * sc] == pooled[b, t, pos // 2, pos % 2, ch]
    assert int(torch.isnan(seq).sum()) == seq.numel() // 2
