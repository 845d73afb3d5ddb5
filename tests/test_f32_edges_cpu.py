"""CPU checks of the references and bounds tests/test_f32_edges_gpu.py relies on, at that file's own shapes and inputs: a
reference that is wrong at an odd length, or a bound torch's own float32 arithmetic cannot keep, would make the GPU test
meaningless (or unpassable) without anyone noticing."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f32_edges_cases as cs
from oracle import f32_edges_ref as eref
from oracle import stft_ref_cpu as sref


def test_f32_edge_references_and_bounds():
    # --- generalised stft_direct_f64 against stft_ref (torch.stft, float32) at the odd lengths; 2e-6 as in
    #     test_stft_oracle_vs_direct_dft
    for fft_len in cs.FFTS:
        for batch, n_frames in cs.STFT_ODD:
            hop, length = cs.stft_hop(fft_len, n_frames), cs.stft_length(fft_len, n_frames)
            audio = cs.loud_audio(batch, length, 5)
            y = sref.stft_ref(audio, fft_len, hop)
            yd = sref.stft_direct_f64(audio, fft_len, hop)
            assert y.shape == yd.shape == (batch, 2, n_frames, fft_len // 2 + 1)
            np.testing.assert_allclose(y.numpy(), yd.numpy(), rtol=0, atol=2e-6)
            t = max(1, n_frames - 2)                # fewer frames and bins select, they do not change values
            part = sref.stft_direct_f64(audio, fft_len, hop, n_frames=t, n_bins=100)
            np.testing.assert_allclose(part.numpy(), yd[:, :, :t, :100].numpy(), rtol=0, atol=1e-14)
        # frames past torch.stft's own: the reflection written out as a signal (a, then a mirrored without its last sample)
        # and handed to torch.stft must give the same frames
        length, hop, n_frames = cs.stft_max_frames(fft_len)
        audio = cs.loud_audio(2, length, 6)
        ext = torch.cat([audio, audio[:, :-1].flip(-1)], -1)
        y = sref.stft_ref(ext.double(), fft_len, hop)[:, :, :n_frames]
        yd = sref.stft_direct_f64(audio, fft_len, hop, n_frames=n_frames)
        assert y.shape == yd.shape
        np.testing.assert_allclose(y.numpy(), yd.numpy(), rtol=0, atol=1e-12)
        with pytest.raises(ValueError, match="past the reflected signal"):
            sref.stft_direct_f64(audio, fft_len, hop, n_frames=n_frames + 1)
    # the wrap case takes torch.stft in float64 (the DFT matrix would be ~9 GFLOP): same function, same dtype, small shape
    audio = cs.loud_audio(3, cs.stft_length(512, 5), 5)
    np.testing.assert_allclose(sref.stft_ref(audio.double(), 512, cs.HOP).numpy(), sref.stft_direct_f64(audio, 512, cs.HOP).numpy(),
                               rtol=0, atol=1e-12)

    # --- float64 istft_ref against the float32 one at the new hops, at the tolerance the kernel is held to
    for fft_len in (256, 512):
        for hop, frames in cs.istft_hops(fft_len):
            for trim in (False, True):
                spec = cs.noise_like((2, 2, frames, fft_len // 2 + (0 if trim else 1)), 11)
                w32 = sref.istft_ref(spec, fft_len, hop, True, trim)
                w64 = sref.istft_ref(spec, fft_len, hop, True, trim, dtype=torch.float64)
                assert w64.dtype == torch.float64 and w64.shape == (2, hop * (frames - 1))
                np.testing.assert_allclose(w32.numpy(), w64.numpy(), rtol=0, atol=2e-5 * float(w64.abs().max()))

    # --- the LSTM step twin against torch.nn.LSTM, both float64
    for b, l in cs.LSTM_CASES:
        lstm, x, _ = cs.lstm_problem(b, l)
        p = {k: v.detach() for k, v in lstm.named_parameters()}
        with torch.no_grad():
            out, (h_n, c_n) = lstm(x)
        gx = torch.stack([x @ p["weight_ih_l0"].T, x @ p["weight_ih_l0_reverse"].T], 2).view(b, l, 2, 4, 256)
        av, hp, gs, c = eref.lstm_bidir_steps_f64(gx, p["weight_hh_l0"], p["weight_hh_l0_reverse"])
        np.testing.assert_allclose(av.numpy(), out.numpy(), rtol=0, atol=1e-13)
        np.testing.assert_allclose(c[:, l - 1, 0].numpy(), c_n[0].numpy(), rtol=0, atol=1e-13)
        np.testing.assert_allclose(c[:, 0, 1].numpy(), c_n[1].numpy(), rtol=0, atol=1e-13)
        assert hp[:, 0, 0].abs().max() == 0 and hp[:, l - 1, 1].abs().max() == 0
        if l > 1:
            assert torch.equal(hp[:, 1:, 0], av[:, :-1, :256]) and torch.equal(hp[:, :-1, 1], av[:, 1:, 256:])
        # h = o tanh(c) ties the saved gates and cell state to the output
        np.testing.assert_allclose((gs[:, :, :, 3] * c.tanh()).reshape(b, l, 512).numpy(), out.numpy(), rtol=0, atol=1e-13)

    # --- the adaptive-pool bounds hold for torch's own float32 forward and backward
    for shape in cs.POOL_SHAPES:
        b, h, w, c, ho, wo = shape
        x, dout = cs.pool_problem(shape)
        want, dwant = cs.pool_ref(x, dout, ho, wo)
        x32 = x.clone().requires_grad_(True)
        out32 = F.adaptive_avg_pool2d(x32, (ho, wo))
        dx32, = torch.autograd.grad(out32, x32, dout)
        assert bool(((out32.detach().double() - want).abs() <= eref.adaptive_pool_fwd_bound(x, ho, wo)).all()), shape
        assert bool(((dx32.double() - dwant).abs() <= eref.adaptive_pool_bwd_bound(dout, h, w)).all()), shape

    # --- the channel-sum bound holds for torch's float32 summation, and a dropped row breaks it by orders of magnitude
    for rows, c, _ in cs.CSUM_CASES:
        x, prior = cs.csum_problem(rows, c)
        for beta in (0, 1):
            want, bound = eref.channel_sum_bound(x, prior if beta else None)
            got = x.sum(0) + prior if beta else x.sum(0)
            assert bool(((got.double() - want).abs() <= bound).all()), (rows, c, beta)
            if 1 < rows <= 257:
                dropped = x[1:].sum(0) + prior if beta else x[1:].sum(0)
                assert bool(((dropped.double() - want).abs() > 100 * bound).all()), (rows, c, beta)
        xi, pi = cs.csum_integers(rows, c)
        want, _ = eref.channel_sum_bound(xi, pi)
        assert torch.equal((xi.sum(0) + pi).double(), want) and float(xi.abs().sum(0).max()) + 100 < 2 ** 24
