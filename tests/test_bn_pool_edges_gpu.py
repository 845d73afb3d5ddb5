"""csrc/bn_pool.hip -- BatchNorm statistics, BatchNorm + max-pool + activation forward and backward -- at the edges of its row
walks, channel blocks and reductions, against float64 (tests/bn_pool_edges_cases.py, oracle/dense_edges_ref.py).

Statistics: integer inputs make every partial sum exact, so mean, invstd and the running estimates must be the float64 result rounded
once -- or its neighbour, one float32 ulp away (the compiler may contract s2 / count - m * m in double); a dropped or doubled row
would be many ulp.  Forward: pooling windows whose maximum is attained several times; the argmax bytes must be the first maximum in
dy * P + dx order, which is what float64 F.max_pool3d reports.  Backward: the same tie-rich inputs against the written-out formula
(shown equal to float64 autograd in tests/test_bn_pool_edges_cpu.py), the strided pooled layout against the contiguous call bit
for bit, and a single pooled gradient that must land on exactly one input position per channel."""
import numpy as np
import pytest
import torch

import bn_pool_edges_cases as cs
from oracle import dense_edges_ref as dref

pytestmark = pytest.mark.gpu


def close(got, want, tol, msg=""):
    np.testing.assert_allclose(got.detach().cpu().double().numpy(), want.detach().double().numpy(), rtol=tol[0], atol=tol[1], err_msg=msg)


def within_one_ulp(got, want, what):
    d = dref.ulp_distance(got.detach().cpu(), want)
    assert int(d.max()) <= cs.MAX_ULP, f"{what}: {int(d.max())} ulp from the float64 result at channel {int(d.argmax())}: got {got.cpu()[int(d.argmax())].item()!r}, want {want[int(d.argmax())].item()!r}"


def check_finalize(part, count, c, want, tag):
    """bn_finalize and bn_finalize_synced (identity reduce_fn) on the same partials: both the reference, and equal to each other"""
    from maavss_amd import ops
    results = []
    for synced in (False, True):
        rm, rv = want["rm0"].cuda(), want["rv0"].cuda()
        nbt = torch.full((), 41, dtype=torch.long, device="cuda")
        if synced:
            calls = []
            mean, invstd = ops.bn_finalize_synced(part, count, lambda sums: calls.append(tuple(sums.shape)), rm, rv, nbt)
            assert calls == [(2 * c + 1,)]
        else:
            mean, invstd = ops.bn_finalize(part, count, rm, rv, nbt)
        assert nbt.item() == 42, f"{tag}: num_batches_tracked must advance once"
        for got, name in ((mean, "mean"), (invstd, "invstd"), (rm, "running_mean"), (rv, "running_var")):
            within_one_ulp(got, want[name], f"{tag} {'synced ' if synced else ''}{name}")
        results.append((mean, invstd, rm, rv))
    for a, b in zip(*results):
        assert torch.equal(a, b), f"{tag}: bn_finalize_synced differs from bn_finalize"


@pytest.mark.parametrize("rows,c", cs.STATS_CASES)
def test_statistics_are_the_float64_result(rows, c):
    from maavss_amd import ops
    y, rm0, rv0 = cs.stats_input(rows, c)
    mean, invstd, rm, rv = cs.stats_reference(rows, c)
    part = ops.bn_stats(y.cuda(), c)
    assert tuple(part.shape) == (cs.stats_nblk(rows), 2, c)
    # the partial sums themselves: exact integers whose totals are the float64 sums
    s1, s2 = dref.bn_sums_f64(y)
    tot = part.double().sum(0).cpu()
    assert torch.equal(tot[0], s1) and torch.equal(tot[1], s2), "bn_stats: a row was dropped or counted twice"
    check_finalize(part, rows, c, dict(mean=mean, invstd=invstd, running_mean=rm, running_var=rv, rm0=rm0, rv0=rv0), f"stats {rows}x{c}")


@pytest.mark.parametrize("nblk,c", cs.TWO_LEVEL_CASES)
def test_two_level_finalize(nblk, c):
    part = cs.two_level_partials(nblk, c)
    _, rm0, rv0 = cs.stats_input(1, c)
    mean, invstd, rm, rv = cs.two_level_reference(nblk, c)
    check_finalize(part.cuda(), cs.TWO_LEVEL_COUNT, c, dict(mean=mean, invstd=invstd, running_mean=rm, running_var=rv, rm0=rm0, rv0=rv0), f"two-level {nblk}x{c}")


def dev(d):
    return {k: v.cuda() for k, v in d.items()}


@pytest.mark.parametrize("small_gamma,batch_stats", [(False, False), (True, True)])
@pytest.mark.parametrize("p", cs.POOL_CASES, ids=cs.POOL_IDS)
def test_forward_argmax_bytes_and_values(p, small_gamma, batch_stats):
    from maavss_amd import ops
    d = dev(cs.pool_input(p, small_gamma, batch_stats))
    want_out, want_arg = cs.fwd_reference(p, small_gamma, batch_stats)
    out, arg = ops.bn_pool_act_fwd(d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"], p.pool, p.act)
    if p.pool > 1:
        assert arg.dtype == torch.uint8
        bad = arg.cpu() != want_arg
        assert not bool(bad.any()), (f"{p.tag}: {int(bad.sum())} of {bad.numel()} argmax bytes differ, first at {tuple(int(i) for i in bad.nonzero()[0])}: "
                                     f"got {int(arg.cpu()[bad][0])}, want {int(want_arg[bad][0])}")
    else:
        assert arg is None
    close(out, want_out, cs.OUT_TOL, p.tag)


def test_forward_16bit_copies_at_c4():
    from maavss_amd import ops
    p = cs.C4_CASE
    d = dev(cs.pool_input(p))
    out, arg, out16, outb = ops.bn_pool_act_fwd(d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"], p.pool, p.act, want16=True, want_bf16=True)
    plain, plain_arg = ops.bn_pool_act_fwd(d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"], p.pool, p.act)
    assert torch.equal(out, plain) and torch.equal(arg, plain_arg)
    assert out16.dtype == torch.float16 and torch.equal(out16, out.half())
    assert outb.dtype == torch.bfloat16 and torch.equal(outb, out.bfloat16())


def forward(ops, p, d):
    out, arg = ops.bn_pool_act_fwd(d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"], p.pool, p.act)
    return out, arg


def backward(ops, p, d, out, arg, with_beta, dout=None, **kw):
    c = p.c
    dg, db = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    dy = ops.bn_pool_act_bwd(d["dout"] if dout is None else dout, out, arg, d["y"], d["mean"], d["invstd"], d["gamma"], p.pool, p.act,
                             dgamma=dg, dbeta=db, beta=d["beta"] if with_beta else None, **kw)
    return dy, dg, db


@pytest.mark.parametrize("small_gamma", [False, True])
@pytest.mark.parametrize("with_beta", [False, True])
@pytest.mark.parametrize("p", cs.POOL_CASES, ids=cs.POOL_IDS)
def test_backward_against_float64(p, with_beta, small_gamma):
    """with_beta: LeakyReLU layers recover xhat from the pooled output (a channel below 1e-2 in |gamma| keeps the gather from y)"""
    from maavss_amd import ops
    d = dev(cs.pool_input(p, small_gamma, True))
    ref = cs.bwd_reference(p, small_gamma)
    out, arg = forward(ops, p, d)
    if p.pool > 1:
        assert torch.equal(arg.cpu(), cs.fwd_reference(p, small_gamma, True)[1])
    dy, dg, db = backward(ops, p, d, out, arg, with_beta)
    close(dy, ref["dy"], cs.DY_TOL, p.tag + " dy")
    close(dg, ref["dgamma"], cs.DPARAM_TOL, p.tag + " dgamma")
    close(db, ref["dbeta"], cs.DPARAM_TOL, p.tag + " dbeta")
    # the other forms of the same call: bit-identical sums and coefficients, dy rounded once
    dy16, dg2, db2 = backward(ops, p, d, out, arg, with_beta, dy_bf16=True)
    assert dy16.dtype == torch.bfloat16 and torch.equal(dy16, dy.bfloat16()) and torch.equal(dg2, dg) and torch.equal(db2, db)
    dy_s, dg_s, db_s = backward(ops, p, d, out, arg, with_beta, reduce_fn=lambda sums: None)
    assert torch.equal(dy_s, dy) and torch.equal(dg_s, dg) and torch.equal(db_s, db), "the split form differs from the single call"
    coef, dg3, db3 = backward(ops, p, d, out, arg, with_beta, coef_only=True)
    assert torch.equal(dg3, dg) and torch.equal(db3, db)
    n = float(p.b * p.t * p.h * p.w)
    close(coef[0], ref["k0"], (1e-6, 0.0), p.tag + " coef[0]")
    close(coef[1], ref["k1"], (cs.DPARAM_TOL[0], cs.DPARAM_TOL[1] / n), p.tag + " coef[1]")      # dbeta / N and dgamma / N at their tolerances / N
    close(coef[2], ref["k2"], (cs.DPARAM_TOL[0], cs.DPARAM_TOL[1] / n), p.tag + " coef[2]")
    # accumulate onto prior gradients
    prior_g, prior_b = torch.arange(p.c).float() - 3, 2 - torch.arange(p.c).float() / 4
    dg4, db4 = prior_g.cuda(), prior_b.cuda()
    ops.bn_pool_act_bwd(d["dout"], out, arg, d["y"], d["mean"], d["invstd"], d["gamma"], p.pool, p.act, dgamma=dg4, dbeta=db4,
                        accumulate=True, beta=d["beta"] if with_beta else None)
    assert torch.equal(dg4, prior_g.cuda() + dg) and torch.equal(db4, prior_b.cuda() + db)


@pytest.mark.parametrize("with_beta", [False, True])
@pytest.mark.parametrize("p", cs.ROUTING_CASES, ids=[p.tag for p in cs.ROUTING_CASES])
def test_single_pooled_gradient_lands_on_the_argmax_input(p, with_beta):
    from maavss_amd import ops
    d = dev(cs.pool_input(p, False, True))
    ref = cs.routing_reference(p)
    out, arg = forward(ops, p, d)
    dy, _, _ = backward(ops, p, d, out, arg, with_beta, dout=cs.routing_dout(p).cuda())
    close(dy, ref["dy"], cs.DY_TOL, p.tag)
    routed = dy.cpu().double() - ref["dense"]
    hit = routed.abs() > 50 * (cs.DY_TOL[1] + cs.DY_TOL[0] * ref["dy"].abs())      # the routed value is beyond 100 of these (CPU test)
    assert torch.equal(hit, ref["g_full"] != 0), f"{p.tag}: the gradient reached {int(hit.sum())} inputs, not the {p.c} argmax positions"


@pytest.mark.parametrize("small_gamma", [False, True])
@pytest.mark.parametrize("with_beta", [False, True])
def test_backward_reads_a_strided_pooled_tensor(with_beta, small_gamma):
    """dout and out inside the LSTM sequence buffer (the layout of test_bn_pool_strided_output): the same kernel, other addresses --
    the same bits as the contiguous call.  The other half of the buffer holds NaN."""
    from maavss_amd import ops
    p = cs.STRIDED
    d = dev(cs.pool_input(p, small_gamma, True))
    ref = cs.bwd_reference(p, small_gamma)
    out, arg = forward(ops, p, d)
    dy, dg, db = backward(ops, p, d, out, arg, with_beta)
    close(dy, ref["dy"], cs.DY_TOL)
    close(dg, ref["dgamma"], cs.DPARAM_TOL)
    close(db, ref["dbeta"], cs.DPARAM_TOL)
    strides = cs.seq_strides(p)
    half = p.t * (p.h // p.pool) * (p.w // p.pool)      # the pooled tensor fills the first half of each [2 * T * S] sequence row
    out_seq = torch.full((p.b, p.c, 2 * half), float("nan"), device="cuda")
    _, arg_s = ops.bn_pool_act_fwd(d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"], p.pool, p.act, out=out_seq, strides=strides)
    assert torch.equal(arg_s, arg)
    assert torch.equal(out_seq[:, :, :half], cs.to_seq(out, 0.0)[:, :, :half]) and bool(torch.isnan(out_seq[:, :, half:]).all())
    dout_seq = cs.to_seq(d["dout"], float("nan"))
    for kw in ({}, {"reduce_fn": lambda sums: None}):
        dg_s, db_s = torch.zeros(p.c, device="cuda"), torch.zeros(p.c, device="cuda")
        dy_s = ops.bn_pool_act_bwd(dout_seq, out_seq, arg, d["y"], d["mean"], d["invstd"], d["gamma"], p.pool, p.act, strides=strides,
                                   dgamma=dg_s, dbeta=db_s, beta=d["beta"] if with_beta else None, **kw)
        assert torch.equal(dy_s, dy) and torch.equal(dg_s, dg) and torch.equal(db_s, db)
