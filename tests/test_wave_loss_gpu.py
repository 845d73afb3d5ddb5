"""The waveform loss on the GPU (csrc/wave_loss.hip, maavss_amd.WaveformLoss) against tests/wave_loss_twin.py, which states the
definition, the cases and the bounds.  K_WGRAD is measured by scripts/wave_loss_parity.py (profiles/wave_loss_parity.json)."""
import functools

import numpy as np
import pytest
import torch

import maavss_amd
import wave_loss_twin as tw
from maavss_amd import _lib
from maavss_amd._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu

_ID = lambda s: "x".join(str(int(v)) for v in s)      # noqa: E731


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@functools.lru_cache(maxsize=None)
def _stft(shape):
    _, _, n, hop, trimmed, normalized = shape
    return maavss_amd.STFT(n, hop, normalized=normalized, trim_stft_end=trimmed)


@functools.lru_cache(maxsize=None)
def _case(shape, inp):
    return tw.make_case(shape, inp)


@functools.lru_cache(maxsize=None)
def _twin(shape, inp, kind):
    pred, tgt = _case(shape, inp)
    return tw.loss_and_grad(pred, tgt, shape, kind, tw.EPS, grad_scale=1.0 / shape[0])


# ---- 1, 2, 3: the waves, the rows and the gradient ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", tw.KINDS)
@pytest.mark.parametrize("shape", tw.SHAPES, ids=_ID)
def test_waves_rows_and_gradient(shape, kind):
    b, t, n, hop = shape[:4]
    length = hop * (t - 1)
    stft = _stft(shape)
    loss = maavss_amd.WaveformLoss(stft, kind=kind, eps=tw.EPS)
    worst = 0.0
    for inp in tw.INPUTS:
        pred_np, tgt_np = _case(shape, inp)
        pred, tgt = torch.from_numpy(pred_np).cuda(), torch.from_numpy(tgt_np).cuda()
        res = loss(pred, tgt, grad_scale=1.0 / b)
        # 1: the waves the op used are STFT.inverse's, bit for bit
        x, s = stft.inverse(pred), stft.inverse(tgt)
        assert res["waves"].shape == (2, b, length)
        assert torch.equal(_bits(res["waves"][0]), _bits(x)) and torch.equal(_bits(res["waves"][1]), _bits(s)), inp
        # 2: the rows against the twin on the device's own f32 waves
        on_waves = tw.wave_rows(x.cpu().numpy(), s.cpu().numpy(), kind, tw.EPS)
        rows = res["rows"].cpu().numpy()
        tw.check_rows(rows, on_waves, length, kind, tw.EPS, label=f"{inp} {kind}")
        want_loss = float(np.mean(rows[:, 0]))
        got_loss = float(res["loss"].cpu())
        assert got_loss != got_loss if want_loss != want_loss else abs(got_loss - want_loss) <= 4 * (b + 1) * tw.U53 * max(abs(rows[:, 0]).max(), 1.0)
        # 3: the gradient against the float64 end-to-end twin
        r = _twin(shape, inp, kind)
        got = res["grad"].cpu().numpy()
        bad = np.isnan(r["rows"][:, 0])
        assert np.array_equal(np.isnan(rows[:, 0]), bad), (inp, "a non-finite input makes its own row NaN, and no other")
        if inp == "nan":
            assert bad[-1] and not bad[:-1].any()
        elif inp == "inf":
            assert bad[0] and not bad[1:].any()
        else:
            assert not bad.any()
        assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all(), inp
        ratios = tw.grad_ratios(got, r, tw.EPS)
        assert len(ratios) == int((~bad).sum())
        if ratios:
            print(f"{inp} {kind}: gradient ratio {max(ratios):.3g} (gate {tw.K_WGRAD:g}); l {rows[:, 0]}")
            worst = max(worst, max(ratios))
            assert max(ratios) <= tw.K_WGRAD, (inp, ratios)
        if inp == "zero_pred" and kind == "si_sdr":
            assert not got.any()                      # x = 0: the function's own saddle, the twin's zeros are zeros
        fin = got[~bad]
        assert not fin[:, 1, :, 0].any(), "the imaginary gradient of DC is zero"
        if not shape[4]:
            assert not fin[:, 1, :, -1].any(), "the imaginary gradient of Nyquist is zero"
    print(f"largest gradient ratio of the shape: {worst:.3g}")


# ---- 4: the forward-only form, determinism, the accumulating form ------------------------------------------------------------------------

@pytest.mark.parametrize("kind", tw.KINDS)
def test_forward_only_and_two_runs(kind):
    shape = tw.SHAPES[1]
    loss = maavss_amd.WaveformLoss(_stft(shape), kind=kind, eps=tw.EPS)
    for inp in ("k0.3", "equal", "nan"):
        pred, tgt = (torch.from_numpy(a).cuda() for a in _case(shape, inp))
        first, second, fwd = loss(pred, tgt, grad_scale=0.25), loss(pred, tgt, grad_scale=0.25), loss(pred, tgt)
        assert fwd["grad"] is None
        for key in ("grad", "rows", "loss"):
            assert torch.equal(_bits(first[key]), _bits(second[key])), (inp, key)
        assert torch.equal(_bits(first["rows"]), _bits(fwd["rows"])) and torch.equal(_bits(first["loss"]), _bits(fwd["loss"]))


def _raw_call(loss, pred, tgt, grad_scale, d_pred, d_frames, d_block_stride, accumulate, rows):
    b, _, t, f = pred.shape
    st = loss.stft
    nbytes = int(_lib.query("maavss_wave_loss_ws_bytes", b, t, st.fft_len, st.hop))
    ws = _lib.workspace(nbytes, pred.device)
    _lib.call("maavss_wave_loss", ptr(pred), ptr(tgt), b, t, f, ptr(st.raw_window), st.fft_len, st.hop, 1 if st.normalized else 0,
              maavss_amd.wave_loss.KINDS.index(loss.kind), loss.eps, grad_scale, ptr(d_pred), d_frames, d_block_stride, accumulate, ptr(rows),
              ptr(ws), nbytes, stream_ptr())


@pytest.mark.parametrize("shape,d_frames", [(tw.SHAPES[2], 8), (tw.SHAPES[1], 1), (tw.SHAPES[4], 3)], ids=["2x24-by-8", "3x5-by-1", "2x3-whole"])
def test_the_accumulating_form_adds_the_plain_gradient_into_strided_blocks(shape, d_frames):
    b, t = shape[:2]
    loss = maavss_amd.WaveformLoss(_stft(shape), kind="si_sdr", eps=tw.EPS)
    pred, tgt = (torch.from_numpy(a).cuda() for a in _case(shape, "k0.3"))
    f = pred.shape[3]
    plain = loss(pred, tgt, grad_scale=0.5 / b)
    k, blk, pad = t // d_frames, b * 2 * d_frames * f, 37
    g = torch.Generator().manual_seed(5)
    buf = torch.randn(k * (blk + pad) + pad, generator=g).cuda()
    before = buf.clone()
    rows = torch.empty(b, 5, dtype=torch.float64, device="cuda")
    _raw_call(loss, pred, tgt, 0.5 / b, buf[pad:], d_frames, blk + pad, 1, rows)
    assert torch.equal(_bits(rows), _bits(plain["rows"]))
    assert torch.equal(buf[:pad], before[:pad])
    for j in range(k):
        lo = pad + j * (blk + pad)
        got, was = buf[lo:lo + blk].view(b, 2, d_frames, f), before[lo:lo + blk].view(b, 2, d_frames, f)
        # the gradient is rounded to f32 and then added: one f32 rounding per element, that of the sum
        assert torch.equal(got, was + plain["grad"][:, :, d_frames * j:d_frames * (j + 1)]), j
        assert torch.equal(buf[lo + blk:lo + blk + pad], before[lo + blk:lo + blk + pad]), (j, "the gap between two blocks is not written")
    # the same through WaveformLoss(into=...), and written (not added) into strided blocks
    into = torch.randn(k, b, 2, d_frames, f, generator=g).cuda()
    was = into.clone()
    res = loss(pred, tgt, grad_scale=0.5 / b, into=into)
    assert res["grad"] is None
    assert torch.equal(into, was + torch.stack(plain["grad"].split(d_frames, dim=2)))
    _raw_call(loss, pred, tgt, 0.5 / b, into, d_frames, into.stride(0), 0, rows)
    assert torch.equal(into, torch.stack(plain["grad"].split(d_frames, dim=2)))


# ---- 5: nothing waits for the device ---------------------------------------------------------------------------------------------------

def test_a_call_never_synchronises():
    shape = tw.SHAPES[2]
    loss = maavss_amd.WaveformLoss(_stft(shape), kind="si_sdr", eps=tw.EPS)
    pred, tgt = (torch.from_numpy(a).cuda() for a in _case(shape, "k0.3"))
    loss(pred, tgt, grad_scale=1.0)                      # warm: the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = loss(pred, tgt, grad_scale=1.0)
        fwd = loss(pred, tgt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(res["grad"]).all() and torch.equal(res["rows"], fwd["rows"])
