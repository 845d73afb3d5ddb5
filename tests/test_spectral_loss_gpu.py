"""The power-law compressed spectral loss on the GPU (csrc/spectral_loss.hip, maavss_amd.SpectralLoss, ops.spectral_loss_pair,
TrainStep(audio_loss=...), Validator(audio_loss=...)) against tests/spectral_loss_twin.py, which states the definition, the cases and the
bounds.  Figures measured on an MI355X (scripts/spectral_loss_parity.py, profiles/spectral_loss_parity.json): every one of the 2 299 540
finite gradient elements of the cases was bit-identical to the twin rounded once to f32, and the largest row-sum excess was 3.09 in units
of 2^-53 of the no-cancellation magnitude."""
import functools
import os

import numpy as np
import pytest
import torch

import maavss_amd
import spectral_loss_twin as tw
from maavss_amd import _lib, ops
from maavss_amd._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    return tw.make_case(shape, kind)


@functools.lru_cache(maxsize=None)
def _twin(shape, kind, params):
    pred, tgt = _case(shape, kind)
    return tw.loss_and_grad(pred, tgt, *params, grad_scale=1.0 / pred.size)


def _row_bound(r, n_terms, k=tw.K_SUM):
    with np.errstate(all="ignore"):
        return (n_terms - 1) * tw.U53 * r["rows"] + k * tw.U53 * r["Bsum"]


# ---- 1, 2: the gradient and the row sums against the twin ------------------------------------------------------------------------------

@pytest.mark.parametrize("params", tw.PARAMS, ids=lambda p: "c%g-mix%g-eps%g" % p)
@pytest.mark.parametrize("shape", tw.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gradient_and_row_sums_equal_the_twin(shape, params):
    b, t, f = shape
    loss = maavss_amd.SpectralLoss(*params)
    for kind in tw.KINDS:
        pred, tgt = _case(shape, kind)
        r = _twin(shape, kind, params)
        res = loss(torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda(), grad_scale=1.0 / pred.size)
        got, rows, a_loss = res["grad"].cpu().numpy(), res["rows"].cpu().numpy(), float(res["loss"].cpu())
        with np.errstate(all="ignore"):
            want32 = r["grad"].astype(np.float32)
        fin = np.isfinite(r["grad"])
        # (c) the non-finite elements sit where the twin's do, NaN for NaN and each infinity for itself
        assert np.array_equal(np.isnan(got), np.isnan(want32)), (kind, "NaN positions")
        assert np.array_equal(got[np.isinf(want32)], want32[np.isinf(want32)]) and np.array_equal(np.isinf(got), np.isinf(want32)), kind
        if kind in tw.FINITE_KINDS:
            assert fin.all()
        # (a) every finite element within half an f32 ulp plus K_GRAD 2^-53 A
        ex = tw.grad_excess(got, r["grad"], r["A"])
        same = (_bits(got) == _bits(want32))[fin]
        print(f"{kind}: gradient excess {ex.max():.3g} (gate {tw.K_GRAD:g}), bit-identical {same.mean() * 100 if same.size else 100:.4f} % of {same.size}")
        assert ex.max() <= tw.K_GRAD, (kind, float(ex.max()))
        # (b) a condition: f32-internal arithmetic reaches 14 to 25 %
        assert same.size == 0 or same.mean() >= tw.IDENTICAL_MIN, (kind, float(same.mean()))
        if kind == "equal":
            assert not got.any() and not rows.any() and a_loss == 0.0
        if kind == "zero_both":
            hole = np.broadcast_to(((pred == 0) & (tgt == 0)).all(axis=1, keepdims=True), pred.shape)
            assert hole.any() and not got[hole].any()
        # 2: the row sums
        fin_rows = np.isfinite(r["rows"])
        assert np.array_equal(np.isfinite(rows), fin_rows), (kind, "a non-finite input makes its row's sums non-finite, and no other row's")
        sx = tw.sum_excess(rows, r["rows"], r["Bsum"], t * f)
        print(f"{kind}: row-sum excess {sx.max():.3g} (gate {tw.K_SUM:g})")
        assert sx.max() <= tw.K_SUM, (kind, float(sx.max()))
        if fin_rows.all():
            bound = float(((1.0 - params[1]) * _row_bound(r, t * f)[:, 0] + params[1] * _row_bound(r, t * f)[:, 1]).sum()) / pred.size
            assert abs(a_loss - r["loss"]) <= bound + 4 * (b + 1) * tw.U53 * r["loss"], kind


# ---- 3: buffer discipline and determinism -------------------------------------------------------------------------------------------

def _raw_call(pred, tgt, params, grad_scale, d_pred, rows):
    b, _, t, f = pred.shape
    nbytes = int(_lib.query("maavss_spectral_loss_ws_bytes", b, t))
    ws = _lib.workspace(nbytes, pred.device)
    _lib.call("maavss_spectral_loss", ptr(pred), ptr(tgt), b, t, f, *params, grad_scale, ptr(d_pred), ptr(rows), ptr(ws), nbytes, stream_ptr())


@pytest.mark.parametrize("shape", [(3, 5, 257), (1, 1, 1), (1, 70, 257)], ids=lambda s: "x".join(map(str, s)))
def test_nothing_is_written_outside_the_gradient_and_the_rows(shape):
    b, t, f = shape
    pred, tgt = (torch.from_numpy(x).cuda() for x in _case(shape, "scale_0.3"))
    n, pad = pred.numel(), 1031
    gbuf = torch.full((pad + n + pad,), 12345.0, dtype=torch.float32, device="cuda")
    rbuf = torch.full((pad + 1 + 2 * b + pad,), 12345.0, dtype=torch.float64, device="cuda")
    d_pred, rows = gbuf[pad:pad + n], rbuf[pad + 1:pad + 1 + 2 * b]              # odd element offsets: 4- and 8-byte alignment only
    _raw_call(pred, tgt, tw.PARAMS[0], 1.0 / n, d_pred, rows)
    assert (gbuf[:pad] == 12345.0).all() and (gbuf[pad + n:] == 12345.0).all()
    assert (rbuf[:pad + 1] == 12345.0).all() and (rbuf[pad + 1 + 2 * b:] == 12345.0).all()
    want = maavss_amd.SpectralLoss(*tw.PARAMS[0])(pred, tgt, grad_scale=1.0 / n)
    assert torch.equal(d_pred.view_as(pred), want["grad"]) and torch.equal(rows.view(b, 2), want["rows"])
    # the forward-only form: no gradient, the same sums
    rbuf.fill_(12345.0)
    _raw_call(pred, tgt, tw.PARAMS[0], 1.0 / n, None, rows)
    assert torch.equal(rows.view(b, 2), want["rows"]) and (rbuf[:pad + 1] == 12345.0).all() and (rbuf[pad + 1 + 2 * b:] == 12345.0).all()
    fwd = maavss_amd.SpectralLoss(*tw.PARAMS[0])(pred, tgt)
    assert fwd["grad"] is None and torch.equal(fwd["rows"], want["rows"]) and torch.equal(fwd["loss"], want["loss"])


@pytest.mark.parametrize("params", [tw.PARAMS[0], tw.PARAMS[2]], ids=lambda p: "c%g-mix%g" % p[:2])
def test_two_runs_and_a_row_of_its_own_give_identical_bytes(params):
    shape = (3, 5, 257)
    loss = maavss_amd.SpectralLoss(*params)
    for kind in ("scale_0.3", "zero_pred", "nan"):
        pred, tgt = (torch.from_numpy(x).cuda() for x in _case(shape, kind))
        gs = 1.0 / pred.numel()
        first, second = loss(pred, tgt, grad_scale=gs), loss(pred, tgt, grad_scale=gs)
        for key in ("grad", "rows", "loss"):
            assert np.array_equal(_bits(first[key].cpu().numpy().reshape(-1)), _bits(second[key].cpu().numpy().reshape(-1))), (kind, key)
        for i in range(shape[0]):
            own = loss(pred[i:i + 1], tgt[i:i + 1], grad_scale=gs)
            assert np.array_equal(_bits(own["grad"].cpu().numpy()), _bits(first["grad"][i:i + 1].cpu().numpy())), (kind, i)
            assert np.array_equal(_bits(own["rows"].cpu().numpy()), _bits(first["rows"][i:i + 1].cpu().numpy())), (kind, i)


# ---- 4: the pair entry --------------------------------------------------------------------------------------------------------------

def _attention_operands(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g).cuda(), torch.rand(shape, generator=g).cuda()


@pytest.mark.parametrize("shape,v_shape,num_seq", [((3, 5, 257), (3, 1, 16, 16), 1), ((2, 8, 256), (2, 1, 67, 67), 3), ((1, 1, 1), (1, 1, 1, 1), 2)],
                         ids=["3x5x257", "2x8x256", "1x1x1"])
@pytest.mark.parametrize("params", tw.PARAMS, ids=lambda p: "c%g-mix%g-eps%g" % p)
def test_pair_entry(shape, v_shape, num_seq, params):
    b, t, f = shape
    coeff = 0.001
    a_pred, a_tgt = (torch.from_numpy(x).cuda() for x in _case(shape, "scale_0.3"))
    v_pred, v_tgt = _attention_operands(v_shape, 7)
    n = a_pred.numel()
    loss = maavss_amd.SpectralLoss(*params)
    losses, d_a, d_v, parts = ops.spectral_loss_pair(a_pred, a_tgt, v_pred, v_tgt, coeff, loss, num_seq=num_seq)
    m_losses, m_d_a, m_d_v = ops.mse_pair(a_pred, a_tgt, v_pred, v_tgt, coeff, num_seq=num_seq)
    # the attention term is mse_pair's, bit for bit
    assert torch.equal(d_v, m_d_v) and _bits(losses[1:2].cpu().numpy()) == _bits(m_losses[1:2].cpu().numpy())
    # the audio gradient is the single entry's at grad_scale = (1 / num_seq) / n, bit for bit
    inv = float(np.float32(1.0 / num_seq))
    single = loss(a_pred, a_tgt, grad_scale=inv / n)
    assert torch.equal(d_a, single["grad"])
    # losses[0] and parts against the twin: the row bounds, the sums over the rows, and for losses[0] its rounding to f32
    r = _twin(shape, "scale_0.3", params)
    rb = _row_bound(r, t * f)
    la, lv, lt = (float(x) for x in losses.cpu())
    mag, cplx = (float(x) for x in parts.cpu())
    slack = 4 * (b + 1) * tw.U53
    assert abs(mag - r["mag_mean"]) <= rb[:, 0].sum() / n + slack * r["mag_mean"]
    assert abs(cplx - r["cplx_mean"]) <= rb[:, 1].sum() / n + slack * r["cplx_mean"]
    bound = ((1.0 - params[1]) * rb[:, 0].sum() + params[1] * rb[:, 1].sum()) / n + slack * r["loss"]
    assert abs(la - r["loss"]) <= float(tw.ulp32(r["loss"])) + bound
    total = (r["loss"] + float(np.float32(coeff)) * lv) * inv
    assert abs(lt - total) <= float(tw.ulp32(total)) + bound + 2 * tw.U24 * coeff * lv
    # want_grads=False: the same losses, no gradient
    l2, a2, v2, p2 = ops.spectral_loss_pair(a_pred, a_tgt, v_pred, v_tgt, coeff, loss, num_seq=num_seq, want_grads=False)
    assert a2 is None and v2 is None and torch.equal(l2, losses) and torch.equal(p2, parts)
    if params[:2] == (1.0, 1.0):
        # the MSE again: mse_pair's own f32 error bound on the loss, 2 f32 ulps on the gradient
        ma = float(m_losses[0].cpu())
        print(f"compress 1, mix 1: losses[0] {la!r}, mse_pair {ma!r}, bound {tw.mse_pair_bound(n):.3g} relative")
        assert abs(la - ma) <= tw.mse_pair_bound(n) * ma
        got, want = d_a.cpu().numpy().astype(np.float64), m_d_a.cpu().numpy().astype(np.float64)
        ulps = np.abs(got - want) / tw.ulp32(np.maximum(np.abs(got), np.abs(want)))
        print(f"compress 1, mix 1: d_a within {ulps.max():.3g} f32 ulps of mse_pair's")
        assert ulps.max() <= 2.0


# ---- 5: TrainStep and Validator on the avse_S golden shape ---------------------------------------------------------------------------

S = 3


@pytest.fixture(scope="module")
def small(golden_dir):
    from oracle import avse_ref_cpu as orc
    z = np.load(os.path.join(golden_dir, "avse_S.npz"), allow_pickle=False)
    m = {k[5:]: z[k].item() for k in z.files if k.startswith("meta_")}
    n_bins, t_a = m["fft_len"] // 2 + 1, m["hops_per_frame"] * m["frames"]
    shapes = ([m["batch"], 2, t_a, n_bins], [m["batch"], 1, m["frames"], m["width"], m["width"]], m["hops_per_frame"])

    def model(train):
        net = maavss_amd.AV_Fusion_Model_Frames(*shapes, precise=True)
        net.load_state_dict(orc.seeded_state_dict(orc.AVFusionFramesRef(*shapes), m["seed"]), strict=True)
        return net.to("cuda").train(train)

    batch = [x.cuda() for x in orc.synthetic_batch(m["batch"], m["frames"], m["width"], t_a, n_bins, m["hops_per_frame"], m["seed"] + 1)]
    prev = maavss_amd.set_deterministic(True)
    yield dict(m=m, model=model, batch=batch)
    maavss_amd.set_deterministic(prev)


def test_sliding_window_step_is_the_three_windows_driven_by_hand(small):
    from maavss_amd.trainer import FlatParams, sliding_windows
    m, (x_a, x_v, y_a, y_v) = small["m"], small["batch"]
    hpf, frames, coeff = m["hops_per_frame"], m["frames"], m["loss_coeff"]
    clip_a = torch.cat([x_a, x_a[:, :, :hpf * (S - 1)]], dim=2)
    clip_y = torch.cat([y_a.repeat(1, 1, frames, 1), y_a.repeat(1, 1, S - 1, 1)], dim=2)
    clip_v = torch.cat([x_v, x_v[:, :, :S - 1]], dim=2)
    loss = maavss_amd.SpectralLoss()
    step = maavss_amd.TrainStep(small["model"](True), lr=m["lr"], loss_coeff=coeff, num_seq=S, audio_loss=loss)
    got = step.sliding_window_step(clip_a, clip_y, clip_v, clip_v, frames, hpf)
    by_hand = small["model"](True)
    flat = FlatParams(by_hand)
    need = {n: bool(p.requires_grad) for n, p in by_hand.named_parameters()}
    for j, xa, xv, ya, yv in sliding_windows(clip_a, clip_y, clip_v, clip_v, frames, hpf, S):
        (a, v, _), sv = by_hand._engine_forward(xa, xv, train=True)
        losses, d_a, d_v, parts = ops.spectral_loss_pair(a, ya.contiguous(), v, yv.contiguous(), coeff, loss, num_seq=S)
        by_hand._engine_backward(sv, d_a, d_v, None, need, grads=flat.grad_views, accumulate=j > 0)
    assert step.flat.grads.abs().max().item() > 0
    assert torch.equal(step.flat.grads, flat.grads)
    assert torch.equal(got, losses) and torch.equal(step.losses, losses) and torch.equal(step.loss_parts, parts)


def test_compress_1_mix_1_trains_as_the_default_step(small):
    m, batch = small["m"], small["batch"]
    plain = maavss_amd.TrainStep(small["model"](True), lr=m["lr"], loss_coeff=m["loss_coeff"])
    as_mse = maavss_amd.TrainStep(small["model"](True), lr=m["lr"], loss_coeff=m["loss_coeff"], audio_loss=maavss_amd.SpectralLoss(1.0, 1.0))
    l0, l1 = plain(*batch, optimizer_step=False), as_mse(*batch, optimizer_step=False)
    assert plain.loss_parts is None and as_mse.loss_parts is not None
    assert abs(float(l1[0]) - float(l0[0])) <= tw.mse_pair_bound(batch[2].numel()) * float(l0[0]) and torch.equal(l0[1], l1[1])
    worst = 0.0
    for name, g0 in plain.flat.grad_views.items():
        g1 = as_mse.flat.grad_views[name]
        if not g0.any():                               # a tensor the step gives no gradient: none here either
            assert not g1.any(), name
            continue
        rel = float((g1.double() - g0.double()).norm() / g0.double().norm())
        worst = max(worst, rel)
        assert rel <= tw.TRAIN_REL_L2, (name, rel)
    print(f"compress 1, mix 1 against the default step: the largest relative L2 over the gradient tensors is {worst:.3g} (gate {tw.TRAIN_REL_L2:g})")


def test_twenty_steps_on_one_batch_lower_the_loss(small):
    batch = small["batch"]
    step = maavss_amd.TrainStep(small["model"](True), lr=1e-3, loss_coeff=small["m"]["loss_coeff"], audio_loss=maavss_amd.SpectralLoss())
    history = [step(*batch)[0] for _ in range(20)]
    history = [float(x) for x in torch.stack(history).cpu()]
    print(f"losses[0] over twenty steps: first {history[0]!r}, last {history[-1]!r}, parts {step.loss_parts.cpu().tolist()}")
    assert history[-1] < history[0]


def test_validator_reports_the_twins_loss_and_never_waits(small):
    m, (x_a, x_v, y_a, y_v) = small["m"], small["batch"]
    model, coeff = small["model"](False), m["loss_coeff"]
    loss = maavss_amd.SpectralLoss()
    g = torch.Generator().manual_seed(3)
    x_a1, y_a1 = (x_a[:1] * 3).contiguous(), (y_a[:1] + torch.randn(y_a[:1].shape, generator=g).cuda()).contiguous()      # a worse batch of one
    x_v1, y_v1 = x_v[:1].contiguous(), y_v[:1].contiguous()
    val = maavss_amd.Validator(model, loss_coeff=coeff, audio_loss=loss)
    plain = maavss_amd.Validator(model, loss_coeff=coeff)
    val._acc(x_a.device)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")              # any blocking call of torch's before result() raises
    try:
        val.add_windows(x_a, x_v, y_a, y_v)
        val.add_windows(x_a1, x_v1, y_a1, y_v1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    res = val.result()
    plain.add_windows(x_a, x_v, y_a, y_v)
    plain.add_windows(x_a1, x_v1, y_a1, y_v1)
    base = plain.result()
    new = {"val_loss_spectral_mag", "val_loss_spectral_cplx", "val_loss_spectral", "val_objective"}
    assert set(res) - set(base) == new
    assert all(res[k] == base[k] or res[k] != res[k] and base[k] != base[k] for k in base)          # NaN: a quantity nothing was added to
    assert val._buf.numel() == plain._buf.numel() + 3
    # the twin on the model's outputs: sums of both batches over the elements of both
    sums, bounds, elems, means = np.zeros(2), np.zeros(2), 0, []
    with torch.no_grad():
        for xa, xv, ya in ((x_a, x_v, y_a), (x_a1, x_v1, y_a1)):
            a = model(xa, xv)[0]
            r = tw.loss_and_grad(a.cpu().numpy(), ya.cpu().numpy(), loss.compress, loss.mix, loss.eps)
            sums += r["rows"].sum(0)
            bounds += _row_bound(r, a.shape[2] * a.shape[3]).sum(0)
            elems += a.numel()
            means.append(r["rows"].sum(0) / a.numel())
    slack = 16 * tw.U53
    for k, key in enumerate(("val_loss_spectral_mag", "val_loss_spectral_cplx")):
        weighted = sums[k] / elems
        print(f"{key} {res[key]!r}, twin {weighted!r}, bound {bounds[k] / elems + slack * weighted:.3g}")
        assert abs(res[key] - weighted) <= bounds[k] / elems + slack * weighted, key
        assert abs(weighted - 0.5 * (means[0][k] + means[1][k])) > 1e-3 * weighted, "the two means must differ for the check to see the weighting"
    mixed = (1.0 - loss.mix) * sums[0] / elems + loss.mix * sums[1] / elems
    assert abs(res["val_loss_spectral"] - mixed) <= ((1.0 - loss.mix) * bounds[0] + loss.mix * bounds[1]) / elems + slack * mixed
    assert res["val_objective"] == res["val_loss_spectral"] + coeff * res["val_loss_attn"]
    assert val.improved(res, key="val_objective") and val.best == res["val_objective"]
