"""CPU-only part of the power-law compressed spectral loss (maavss_amd/spectral_loss.py, csrc/spectral_loss.hip): the float64 twin
against torch.autograd and against the MSE it contains, its exact zeros, the teeth of the GPU gate (three plausible mistakes move the
gradient far beyond it, a correct float64 evaluation stays inside it), and the refusals of SpectralLoss and of the C entries (every call
below fails before any launch)."""
import inspect
import math
import types

import numpy as np
import pytest
import torch

import spectral_loss_twin as tw
from maavss_amd import _lib


def _mixed_case():
    """[3, 2, 5, 257]: rows of scale 0.3, 1e-3 and 1e-5, with bins zeroed in pred, in tgt and in both."""
    rng = np.random.default_rng(11)
    scale = np.array([0.3, 1e-3, 1e-5]).reshape(3, 1, 1, 1)
    tgt = (scale * rng.standard_normal((3, 2, 5, 257))).astype(np.float32)
    pred = (tgt + 0.3 * scale * rng.standard_normal((3, 2, 5, 257))).astype(np.float32)
    pred[:, :, 1, 10:20] = 0.0
    tgt[:, :, 2, 30:40] = 0.0
    pred[:, :, 3, 50:60] = 0.0
    tgt[:, :, 3, 50:60] = 0.0
    return pred, tgt


def _autograd(pred, tgt, c, lam, eps, grad_scale):
    p = torch.from_numpy(pred).double().requires_grad_(True)
    t = torch.from_numpy(tgt).double()
    rp, rt = p[:, 0] ** 2 + p[:, 1] ** 2 + eps, t[:, 0] ** 2 + t[:, 1] ** 2 + eps
    Mp, Mt, gp, gt = rp ** (c / 2), rt ** (c / 2), rp ** ((c - 1) / 2), rt ** ((c - 1) / 2)
    mag = ((Mp - Mt) ** 2).sum()
    cplx = ((p[:, 0] * gp - t[:, 0] * gt) ** 2 + (p[:, 1] * gp - t[:, 1] * gt) ** 2).sum()
    total = ((1 - lam) * mag + lam * cplx) * grad_scale
    total.backward()
    return p.grad.numpy(), float(total.detach()) / grad_scale / pred.size


@pytest.mark.parametrize("c,lam,eps", tw.PARAMS)
def test_the_twins_gradient_is_autograds(c, lam, eps):
    pred, tgt = _mixed_case()
    gs = 1.0 / pred.size
    ref, ref_loss = _autograd(pred, tgt, c, lam, eps, gs)
    r = tw.loss_and_grad(pred, tgt, c, lam, eps, gs)
    err = np.abs(r["grad"] - ref).max() / np.abs(ref).max()
    print(f"c {c} mix {lam} eps {eps}: largest difference {err:.3g} of the largest element; loss {r['loss']!r} autograd {ref_loss!r}")
    assert err <= 1e-12
    assert abs(r["loss"] - ref_loss) <= 1e-12 * ref_loss


@pytest.mark.parametrize("shape", [(2, 8, 256), (3, 5, 257)])
def test_compress_1_mix_1_is_the_mse(shape):
    pred, tgt = tw.make_case(shape, "scale_0.3")
    n = pred.size
    d = pred.astype(np.float64) - tgt.astype(np.float64)
    r = tw.loss_and_grad(pred, tgt, 1.0, 1.0, 1e-12, 1.0 / n)
    per_bin = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    assert r["loss"] == math.fsum(per_bin.ravel()) / n
    assert r["cplx_mean"] == r["loss"]
    assert np.array_equal(r["grad"], (2.0 * (1.0 / n)) * d)
    if n & (n - 1) == 0:                              # a power of two: 2 d / N has one spelling
        assert np.array_equal(r["grad"], 2.0 * d / n)


def test_zero_bins_have_zero_gradient_and_equal_inputs_exact_zeros():
    for c, lam, eps in tw.PARAMS:
        pred, tgt = tw.make_case((3, 5, 257), "zero_both")
        hole = (pred == 0.0) & (tgt == 0.0)
        hole = hole[:, :1] & hole[:, 1:]               # both planes on both sides
        assert hole.sum() > 50
        r = tw.loss_and_grad(pred, tgt, c, lam, eps, 1.0 / pred.size)
        assert np.all(r["grad"][np.broadcast_to(hole, pred.shape)] == 0.0)
        pred, tgt = tw.make_case((3, 5, 257), "equal")
        r = tw.loss_and_grad(pred, tgt, c, lam, eps, 1.0 / pred.size)
        assert r["loss"] == 0.0 and np.all(r["rows"] == 0.0) and np.all(r["grad"] == 0.0)


def _mutant(pred, tgt, c, lam, eps, grad_scale, which):
    """The twin's gradient with one plausible mistake."""
    if which == "mix_swapped":
        return tw.loss_and_grad(pred, tgt, c, 1.0 - lam, eps, grad_scale)["grad"]
    q = tw.terms(pred, tgt, c, lam, eps)
    with np.errstate(all="ignore"):
        if which == "c_for_half_c":
            q["Mp"], q["Mt"] = np.power(q["rp"], c), np.power(q["rt"], c)
        elif which == "eps_outside":
            rp, rt = q["pr"] * q["pr"] + q["pi"] * q["pi"], q["tr"] * q["tr"] + q["ti"] * q["ti"]
            q["Mp"], q["Mt"] = np.power(rp, 0.5 * c) + eps, np.power(rt, 0.5 * c) + eps
            q["gp"], q["gt"] = np.power(rp, 0.5 * (c - 1.0)) + eps, np.power(rt, 0.5 * (c - 1.0)) + eps
            q["er"], q["ei"] = q["pr"] * q["gp"] - q["tr"] * q["gt"], q["pi"] * q["gp"] - q["ti"] * q["gt"]
        q["dm"] = q["Mp"] - q["Mt"]
    return tw.gradient(q, c, lam, grad_scale)


def _rel_l2(a, b):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.sum((a - b) ** 2)) / np.sqrt(np.sum(b ** 2)))


# where each mistake changes the definition at all: swapping the mix wherever tgt is not empty (against an empty tgt and with c = 1 the
# magnitude and the complex gradient are both 2 p, so the one-bin case is left to the other kinds); c for c / 2 only where the magnitude
# term counts (mix < 1); eps outside the power only where a bin is empty (eps = 1e-12 beside a power of 1e-2 is below f64's resolution of the sum)
# and the exponent of g is negative (c < 1): there the gradient stops being finite
TEETH = [("mix_swapped", tw.PARAMS, ("scale_0.3", "scale_1e-5", "zero_pred")),
         ("c_for_half_c", [p for p in tw.PARAMS if p[1] < 1.0], ("scale_0.3", "scale_1e-5", "zero_tgt")),
         ("eps_outside", [p for p in tw.PARAMS if p[0] < 1.0], ("zero_pred", "zero_both"))]


@pytest.mark.parametrize("which,params,kinds", TEETH, ids=[t[0] for t in TEETH])
def test_the_gate_has_teeth(which, params, kinds):
    least = math.inf
    for shape in tw.SHAPES:
        for c, lam, eps in params:
            for kind in kinds:
                pred, tgt = tw.make_case(shape, kind)
                gs = 1.0 / pred.size
                good = tw.loss_and_grad(pred, tgt, c, lam, eps, gs)["grad"]
                assert np.isfinite(good).all()
                rel = _rel_l2(_mutant(pred, tgt, c, lam, eps, gs, which), good)
                least = min(least, math.inf if rel != rel else rel)          # a gradient that is no longer finite has moved
                assert not rel <= 1e-3, (which, shape, (c, lam, eps), kind, rel)
    print(f"{which}: the smallest relative L2 move over the cases is {least:.3g}")


def test_a_correct_float64_evaluation_passes_the_identity_condition():
    """The twin's gradient times (1 + 1e-12 randn) -- an evaluation with four thousand times f64's rounding error -- rounds to the same
    f32 on at least 99.99 % of the elements of every finite GPU case: the 99.9 % the GPU test asks is a condition an f64 kernel meets.
    Elements whose float64 value lies exactly half way between two f32 numbers are left out of the count: with compress = 1, mix = 1 and a
    power of two for 2 B T F the gradient is the exact difference of two f32 numbers times a power of two, 3 % of them such ties, which
    any perturbation decides by chance and which every exact evaluation, the kernel's included, decides the same way (to even)."""
    rng = np.random.default_rng(5)
    worst = 1.0
    for shape in tw.SHAPES:
        for c, lam, eps in tw.PARAMS:
            for kind in tw.FINITE_KINDS:
                pred, tgt = tw.make_case(shape, kind)
                g = tw.loss_and_grad(pred, tgt, c, lam, eps, 1.0 / pred.size)["grad"]
                g32 = g.astype(np.float32)
                tie = np.abs(g - g32) == 0.5 * tw.ulp32(g32)
                same = (g32 == (g * (1.0 + 1e-12 * rng.standard_normal(g.shape))).astype(np.float32))[~tie]
                if same.size >= 10000:
                    worst = min(worst, same.mean())
                # a case of fewer than 10 000 elements cannot show 99.99 % with one element changed: there, all but one
                assert same.size - same.sum() <= max(1, int(1e-4 * same.size)), (shape, (c, lam, eps), kind, same.mean())
    print(f"the smallest identical share over the cases of 10 000 elements or more is {worst:.6f}")


def test_the_measured_constants_respect_their_caps():
    assert 0.0 < tw.K_GRAD <= tw.K_CAP and 0.0 < tw.K_SUM <= tw.K_CAP and 0.0 < tw.TRAIN_REL_L2 <= tw.REL_L2_CAP
    assert tw.mse_pair_bound(4112) == (9 + 12) * 2.0 ** -24


def test_spectral_loss_refuses_bad_parameters():
    import maavss_amd
    loss = maavss_amd.SpectralLoss()
    assert (loss.compress, loss.mix, loss.eps) == (0.3, 0.3, 1e-12)
    sig = inspect.signature(maavss_amd.SpectralLoss.__init__).parameters
    assert (sig["compress"].default, sig["mix"].default, sig["eps"].default) == (0.3, 0.3, 1e-12)
    assert maavss_amd.SpectralLoss(1, 1).compress == 1.0 and maavss_amd.SpectralLoss(0.5, 0).mix == 0.0
    for bad in (dict(compress=0.0), dict(compress=-0.3), dict(compress=1.01), dict(compress=float("nan")), dict(compress="0.3"),
                dict(compress=True), dict(mix=-0.1), dict(mix=1.5), dict(mix=float("nan")), dict(mix=None), dict(eps=0.0),
                dict(eps=-1e-12), dict(eps=float("inf")), dict(eps=float("nan"))):
        with pytest.raises(ValueError, match=next(iter(bad))):
            maavss_amd.SpectralLoss(**bad)
    x = torch.zeros(1, 2, 8, 5)
    with pytest.raises(ValueError, match=r"\[B, 2, T, F\]"):
        loss(torch.zeros(1, 3, 8, 5), torch.zeros(1, 3, 8, 5))
    with pytest.raises(ValueError, match=r"\[B, 2, T, F\]"):
        loss(x.double(), x.double())
    with pytest.raises(ValueError, match="differ in shape"):
        loss(x, torch.zeros(1, 2, 8, 6))
    with pytest.raises(ValueError, match="grad_scale"):
        loss(x, x, grad_scale=float("inf"))
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        loss(x, x)
    for cls in (maavss_amd.TrainStep, maavss_amd.Validator):
        assert inspect.signature(cls.__init__).parameters["audio_loss"].default is None
    with pytest.raises(ValueError, match="audio_loss must be None or a maavss_amd.SpectralLoss"):
        maavss_amd.Validator(types.SimpleNamespace(training=False), audio_loss="compressed")


def test_new_symbols_are_exported_and_the_abi_version_is_still_401():
    import maavss_amd
    from maavss_amd import ops
    assert hasattr(maavss_amd, "SpectralLoss") and hasattr(ops, "spectral_loss_pair")
    protos = _lib.parse_header()
    L = _lib.lib()
    for name in ("maavss_spectral_loss_ws_bytes", "maavss_spectral_loss", "maavss_spectral_loss_pair_ws_bytes", "maavss_spectral_loss_pair"):
        assert name in protos and hasattr(L.cdll, name), name
    assert _lib.header_abi_version() == 402 == L.cdll.maavss_version()
    assert _lib.query("maavss_spectral_loss_ws_bytes", 3, 8) == 512 and _lib.query("maavss_spectral_loss_ws_bytes", 0, 8) == 0
    assert _lib.query("maavss_spectral_loss_pair_ws_bytes", 3, 8) == 512 + 256 + 2048
    assert _lib.query("maavss_spectral_loss_pair_ws_bytes", 3, 0) == 0 and _lib.query("maavss_spectral_loss_ws_bytes", 1 << 20, 1 << 20) == 0


def _loss_args(**over):
    """A call of maavss_spectral_loss whose every argument passes (fake, aligned device addresses: never launched in these tests because
    one override makes a check fail)."""
    a = dict(pred=4100, tgt=4108, B=3, T=5, F=257, compress=0.3, mix=0.3, eps=1e-12, grad_scale=1.0, d_pred=4116, rows=8192, ws=8192,
             ws_bytes=1 << 20, stream=None)
    a.update(over)
    return tuple(a.values())


def _pair_args(**over):
    a = dict(a_pred=4100, a_tgt=4108, B=3, T=5, F=257, compress=0.3, mix=0.3, eps=1e-12, v_pred=4100, v_tgt=4104, nv=100, coeff=0.001,
             inv_num_seq=1.0, d_a=4116, d_v=4120, losses=4124, parts=8192, ws=8192, ws_bytes=1 << 20, stream=None)
    a.update(over)
    return tuple(a.values())


BAD = [(dict(pred=None), "null pointer"), (dict(tgt=None), "null pointer"), (dict(rows=None), "null pointer"), (dict(ws=None), "null pointer"),
       (dict(B=0), "bad sizes"), (dict(T=-1), "bad sizes"), (dict(F=0), "bad sizes"), (dict(F=1 << 24), "bad sizes"),
       (dict(B=1 << 20, T=1 << 20), "bad sizes"),
       (dict(compress=0.0), r"compress must be in \(0, 1\]"), (dict(compress=1.5), r"compress must be in \(0, 1\]"),
       (dict(compress=float("nan")), r"compress must be in \(0, 1\]"),
       (dict(mix=-0.5), r"mix must be in \[0, 1\]"), (dict(mix=1.0001), r"mix must be in \[0, 1\]"), (dict(mix=float("nan")), r"mix must be in \[0, 1\]"),
       (dict(eps=0.0), "eps must be positive and finite"), (dict(eps=float("inf")), "eps must be positive and finite"),
       (dict(eps=float("nan")), "eps must be positive and finite"),
       (dict(grad_scale=float("nan")), "grad_scale must be finite"),
       (dict(pred=4101), "4-byte aligned"), (dict(d_pred=4118), "4-byte aligned"), (dict(rows=8196), "8-byte aligned"), (dict(ws=8196), "8-byte aligned"),
       (dict(ws_bytes=64), "workspace of 64 bytes, 256 needed")]


@pytest.mark.parametrize("over,match", BAD, ids=[f"{next(iter(o))}-{i}" for i, (o, _) in enumerate(BAD)])
def test_spectral_loss_refuses_bad_arguments_before_any_launch(over, match):
    with pytest.raises(_lib.MaavssError, match="spectral_loss: .*" + match):
        _lib.call("maavss_spectral_loss", *_loss_args(**over))


BAD_PAIR = [(dict(a_pred=None), "null pointer"), (dict(v_tgt=None), "null pointer"), (dict(losses=None), "null pointer"),
            (dict(parts=None), "null pointer"), (dict(ws=None), "null pointer"),
            (dict(B=0), "bad sizes"), (dict(F=-3), "bad sizes"), (dict(nv=0), "bad sizes"),
            (dict(compress=2.0), r"compress must be in \(0, 1\]"), (dict(mix=-1.0), r"mix must be in \[0, 1\]"),
            (dict(eps=-1e-12), "eps must be positive and finite"), (dict(inv_num_seq=0.0), "inv_num_seq positive"),
            (dict(a_tgt=4110), "4-byte aligned"), (dict(d_a=4117), "4-byte aligned"), (dict(d_v=4121), "4-byte aligned"),
            (dict(parts=8194), "8-byte aligned"), (dict(ws_bytes=2048), "workspace of 2048 bytes, 2560 needed")]


@pytest.mark.parametrize("over,match", BAD_PAIR, ids=[f"{next(iter(o))}-{i}" for i, (o, _) in enumerate(BAD_PAIR)])
def test_spectral_loss_pair_refuses_bad_arguments_before_any_launch(over, match):
    with pytest.raises(_lib.MaavssError, match="spectral_loss_pair: .*" + match):
        _lib.call("maavss_spectral_loss_pair", *_pair_args(**over))


def test_the_nullable_gradients_pass_the_checks():
    """d_pred, d_a and d_v may be null (the forward-only form): with every other argument valid the call would launch, so the checks are
    shown to pass by the one that comes after them all."""
    with pytest.raises(_lib.MaavssError, match="workspace of 8 bytes"):
        _lib.call("maavss_spectral_loss", *_loss_args(d_pred=None, ws_bytes=8))
    with pytest.raises(_lib.MaavssError, match="workspace of 8 bytes"):
        _lib.call("maavss_spectral_loss_pair", *_pair_args(d_a=None, d_v=None, ws_bytes=8))


def test_a_validator_without_audio_loss_keeps_its_buffer_and_its_keys():
    import maavss_amd
    from maavss_amd import quality as q
    model = types.SimpleNamespace(training=False)
    base = q._ACC_LEN
    assert maavss_amd.Validator(model)._buf_len() == base == 51
    assert maavss_amd.Validator(model, intelligibility_sr=16000, bss_filter=32)._buf_len() == base + q._INTEL_LEN + q._BSS_LEN
    with_loss = maavss_amd.Validator(model, intelligibility_sr=16000, bss_filter=32, audio_loss=maavss_amd.SpectralLoss())
    assert with_loss._buf_len() == base + q._INTEL_LEN + q._BSS_LEN + 3
    new = {"val_loss_spectral_mag", "val_loss_spectral_cplx", "val_loss_spectral", "val_objective"}
    assert not new & set(maavss_amd.Validator(model).result())
    res = with_loss.result()                                       # nothing was added: NaN
    assert new <= set(res) and all(math.isnan(res[k]) for k in new)
    assert not with_loss.improved(res, key="val_objective")
    assert with_loss.improved({"val_objective": 2.0, "val_loss": 9.0}, key="val_objective") and with_loss.best == 2.0
    assert inspect.signature(maavss_amd.Validator.improved).parameters["key"].default == "val_loss"
