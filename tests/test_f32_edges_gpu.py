"""The f32 kernels around the ViT (STFT, inverse STFT, LSTM recurrence, pooling / bias / reduction / resize glue) off the
benched shapes, each against a plain float64 (or, where the result is one or two exactly rounded operations, float32) CPU
reference.  Branches reached here for the first time: an STFT frame pair that straddles two clips, the lone last frame of
an odd total, a partial bin pair, idle waves of the inverse STFT, hops up to n_fft, LSTM batch-slab edges and L = 1, the
strided adaptive-pool output.  References and inputs are checked on the CPU by tests/test_f32_edges_cpu.py.

Every case prints its worst error as a fraction of its tolerance (`pytest -s`); profiles/f32_edges_gpu.txt keeps that."""
import pytest
import torch
import torch.nn.functional as F

import f32_edges_cases as cs
from oracle import f32_edges_ref as eref
from oracle import stft_ref_cpu as sref

pytestmark = pytest.mark.gpu

SIGMA = 0.1
STFT_ATOL = 5e-6            # test_stft_matches_oracle's, for synthetic_audio (see cases.loud_audio)
SENTINEL = 777.0
GUARD = 4096                # floats behind an output that must stay untouched


def frac(got, want, atol, rtol=0.0):
    """worst |got - want| / (atol + rtol |want|); <= 1 is np.testing.assert_allclose's criterion"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all())
    return float(((got - want).abs() / (atol + rtol * want.abs())).max())


def report(tag, **fracs):
    print(f"[{tag}] " + " ".join(f"{k} {v:.2f}" for k, v in fracs.items()) + " of tol", flush=True)
    bad = {k: v for k, v in fracs.items() if not v <= 1.0}
    assert not bad, f"[{tag}] exceeds its tolerance: {bad}"


def bits_equal(got, want):
    return torch.equal(got.detach().cpu().contiguous().view(torch.int32), want.detach().contiguous().view(torch.int32))


def guarded(numel, fill=SENTINEL):
    return torch.full((numel + GUARD,), fill, device="cuda", dtype=torch.float32)


def guard_intact(buf, numel):
    return bool((buf[numel:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------ A. STFT forward
def _stft_checks(tag, st, audio_gpu, noise, want, atol=STFT_ATOL):
    """y, x (passed-in noise) and the per-clip maximum against `want`, the float64 STFT of the rows `audio_gpu` holds."""
    x, y, amax = st(audio_gpu, noise=noise.cuda(), return_scale=True)
    assert y.shape == want.shape
    fy, fx = frac(y, want, atol), frac(x, want + SIGMA * noise.double(), atol)
    # the maximum of the values the kernel stored, and credited to the right clip
    assert torch.equal(amax, y.abs().amax((1, 2, 3))), (amax, y.abs().amax((1, 2, 3)))
    fa = frac(amax, want.abs().amax((1, 2, 3)), atol)
    report(tag, y=fy, x=fx, amax=fa)
    return x, y, amax


@pytest.mark.parametrize("batch,n_frames", cs.STFT_ODD)
@pytest.mark.parametrize("fft_len", cs.FFTS)
def test_stft_odd_frame_counts(fft_len, batch, n_frames):
    """Pairs that straddle two clips (4 x 7), a lone last frame (3 x 5), a single frame (1 x 1); length no multiple of the hop."""
    import maavss_amd
    hop, length = cs.stft_hop(fft_len, n_frames), cs.stft_length(fft_len, n_frames)
    audio = cs.loud_audio(batch, length, 5)
    want = sref.stft_direct_f64(audio, fft_len, hop)
    assert want.shape == (batch, 2, n_frames, fft_len // 2 + 1)
    noise = cs.noise_like(want.shape, 9)
    st = maavss_amd.STFT(fft_len, hop, noise_std=SIGMA, device="cuda")
    _stft_checks(f"stft odd {fft_len} b{batch} t{n_frames}", st, audio.cuda(), noise, want)
    if (batch, n_frames) == cs.STFT_ODD[0]:
        # normalize_output_fft: gen_stft_example_ref's arithmetic in float64, at test_stft_trim_and_normalise_output's 2e-5
        stn = maavss_amd.STFT(fft_len, hop, noise_std=SIGMA, normalize_output_fft=True, device="cuda")
        x, y = stn(audio.cuda(), noise=noise.cuda())
        yn = want * (1.0 / (want.abs() + 1e-7).flatten(-3).max(-1).values)[:, None, None, None]
        report(f"stft odd normalised {fft_len} b{batch} t{n_frames}", y=frac(y, yn, 2e-5), x=frac(x, yn + noise.double() * SIGMA, 2e-5))
        # trimmed last bin at an odd frame count
        stt = maavss_amd.STFT(fft_len, hop, noise_std=SIGMA, trim_stft_end=True, device="cuda")
        _stft_checks(f"stft odd trimmed {fft_len} b{batch} t{n_frames}", stt, audio.cuda(), noise[..., :-1].contiguous(),
                     want[..., :-1])


def test_stft_odd_frame_counts_grid_stride_wrap():
    """131 clips x 127 frames = 8319 pairs: every wave walks the pair list a second time, with straddling pairs throughout and
    a lone last frame.  Reference: torch.stft in float64 (checked against the DFT-matrix form on the CPU)."""
    import maavss_amd
    batch, n_frames = cs.STFT_WRAP
    length = cs.stft_length(512, n_frames)
    audio = cs.loud_audio(batch, length, 5)
    want = sref.stft_ref(audio.double(), 512, cs.HOP)
    assert want.dtype == torch.float64 and want.shape == (batch, 2, n_frames, 257)
    st = maavss_amd.STFT(512, cs.HOP, noise_std=SIGMA, device="cuda")
    _stft_checks(f"stft odd wrap 512 b{batch} t{n_frames}", st, audio.cuda(), cs.noise_like(want.shape, 9), want)


@pytest.mark.parametrize("fft_len", cs.FFTS)
def test_stft_row_strides(fft_len):
    """Overlapping rows (stride L // 3) and padded rows (stride L + 37, padding 1e4): each row's STFT is that of the row alone."""
    import maavss_amd
    batch, n_frames = cs.STFT_ODD[0]
    hop, length = cs.stft_hop(fft_len, n_frames), cs.stft_length(fft_len, n_frames)
    st = maavss_amd.STFT(fft_len, hop, noise_std=SIGMA, device="cuda")
    stride = length // 3
    flat = sref.synthetic_audio(1, stride * (batch - 1) + length, 3)[0]
    rows = flat.as_strided((batch, length), (stride, 1)).clone()
    want = sref.stft_direct_f64(rows, fft_len, hop)
    noise = cs.noise_like(want.shape, 9)
    _stft_checks(f"stft rows overlapping {fft_len}", st, flat.cuda().as_strided((batch, length), (stride, 1)), noise, want)
    rows = cs.loud_audio(batch, length, 5)
    padded = torch.full((batch, length + 37), 1e4)
    padded[:, :length] = rows
    want = sref.stft_direct_f64(rows, fft_len, hop)
    _stft_checks(f"stft rows padded {fft_len}", st, padded.cuda()[:, :length], noise, want)


def _stft_call(st, audio, hop, n_frames, n_bins, y, x, noise, amax=None):
    from maavss_amd import _lib
    _lib.call("maavss_stft_fwd", _lib.ptr(audio), audio.shape[0], audio.shape[1], audio.stride(0), _lib.ptr(st.window), st.fft_len, hop,
              n_frames, n_bins, _lib.ptr(y), _lib.ptr(x), _lib.ptr(noise), SIGMA, 0, _lib.ptr(amax), _lib.stream_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize("fft_len", [256, 512])
def test_stft_bin_counts(fft_len):
    """n_bins_out from 1 to n_fft / 2 + 1 through the C-ABI: partial bin pairs (f, f + 64), compact noise, nothing written behind
    the outputs."""
    import maavss_amd
    batch, n_frames = 2, 5
    length = cs.stft_length(fft_len, n_frames)
    audio = cs.loud_audio(batch, length, 5)
    full = sref.stft_direct_f64(audio, fft_len, cs.HOP)
    st = maavss_amd.STFT(fft_len, cs.HOP, noise_std=SIGMA, device="cuda")
    ac = audio.cuda()
    for n_bins in (1, 63, 64, 65, 100, fft_len // 2, fft_len // 2 + 1):
        shape = (batch, 2, n_frames, n_bins)
        numel = batch * 2 * n_frames * n_bins
        noise = cs.noise_like(shape, 9)
        y, x, amax = guarded(numel), guarded(numel), torch.zeros(batch, device="cuda")
        _stft_call(st, ac, cs.HOP, n_frames, n_bins, y, x, noise.cuda(), amax)
        want = full[..., :n_bins]
        yv = y[:numel].view(shape)
        assert guard_intact(y, numel) and guard_intact(x, numel), n_bins
        assert torch.equal(amax, yv.abs().amax((1, 2, 3)))
        report(f"stft bins {fft_len} f{n_bins}", y=frac(yv, want, STFT_ATOL), x=frac(x[:numel].view(shape), want + SIGMA * noise.double(), STFT_ATOL),
               amax=frac(amax, want.abs().amax((1, 2, 3)), STFT_ATOL))


@pytest.mark.parametrize("fft_len", cs.FFTS)
def test_stft_shortest_signal_and_last_admitted_frame(fft_len):
    """length = n_fft / 2 + 1 (every frame is mostly reflection) at one and two frames; the largest frame count the argument check
    admits, whose last sample reflects onto index 0; one step past either limit is refused before any launch."""
    import maavss_amd
    from maavss_amd import _lib
    st = maavss_amd.STFT(fft_len, cs.HOP, noise_std=SIGMA, device="cuda")
    f = fft_len // 2 + 1
    short = fft_len // 2 + 1
    long_len, long_hop, long_frames = cs.stft_max_frames(fft_len)
    for tag, length, hop, n_frames in (("shortest t1", short, cs.HOP, 1), ("shortest t2", short, cs.HOP, 2),
                                       ("last admitted frame", long_len, long_hop, long_frames)):
        audio = cs.loud_audio(3, length, 6)
        want = sref.stft_direct_f64(audio, fft_len, hop, n_frames=n_frames)
        numel = want.numel()
        noise = cs.noise_like(want.shape, 9)
        y, x = guarded(numel), guarded(numel)
        _stft_call(st, audio.cuda(), hop, n_frames, f, y, x, noise.cuda())
        assert guard_intact(y, numel) and guard_intact(x, numel)
        report(f"stft {tag} {fft_len} L{length} hop{hop} t{n_frames}", y=frac(y[:numel].view(want.shape), want, STFT_ATOL),
               x=frac(x[:numel].view(want.shape), want + SIGMA * noise.double(), STFT_ATOL))
    # both limits are MAAVSS_CHECK_ARG lines ahead of the launch (stft.hip: "reflect padding needs length > n_fft/2", "frames run
    # past the reflected signal"); the buffers are sized for the refused problem all the same
    y = guarded(3 * 2 * (long_frames + 1) * f)
    with pytest.raises(_lib.MaavssError, match="length > n_fft/2"):
        _stft_call(st, cs.loud_audio(3, fft_len // 2, 6).cuda(), cs.HOP, 1, f, y, None, None)
    with pytest.raises(_lib.MaavssError, match="past the reflected signal"):
        _stft_call(st, cs.loud_audio(3, long_len, 6).cuda(), long_hop, long_frames + 1, f, y, None, None)
    assert bool((y == SENTINEL).all())


@pytest.mark.parametrize("fft_len", cs.FFTS)
def test_stft_device_noise_odd_frame_count(fft_len):
    """In-kernel Philox noise at 9 x 15 frames (pairs straddle clips, the last pair holds one frame): the draw of a frame does not
    depend on the launch it is part of, no two frames share their last-bin draw, and the noise is N(0, sigma^2)."""
    import maavss_amd
    batch, n_frames = 9, 15
    hop, length = cs.stft_hop(fft_len, n_frames), cs.stft_length(fft_len, n_frames)
    audio = cs.loud_audio(batch, length, 7).cuda()
    st = maavss_amd.STFT(fft_len, hop, noise_std=SIGMA, device="cuda")
    x, y = st(audio, seed=5)
    xs, ys = st(audio[:4].contiguous(), seed=5)
    assert torch.equal(y[:4], ys)
    assert torch.equal(x[:4], xs)
    d = ((x - y) / SIGMA).double().cpu()
    last = d[..., fft_len // 2].flatten()                      # [9 * 2 * 15]: re and im of every frame's last bin
    assert last.unique().numel() == last.numel()
    assert bool((last.abs() > 0).all())
    report(f"stft device noise {fft_len} b{batch} t{n_frames}", mean=abs(d.mean().item()) / 2e-2, std=abs(d.std().item() - 1) / 2e-2)


# ------------------------------------------------------------------------------------------------------------ B. inverse STFT
def _istft_check(tag, fft_len, hop, batch, frames, trim, normalized):
    import maavss_amd
    f = fft_len // 2 + (0 if trim else 1)
    spec = cs.noise_like((batch, 2, frames, f), 11)
    st = maavss_amd.STFT(fft_len, hop, normalized=normalized, trim_stft_end=trim)
    got = st.inverse(spec.cuda())
    want = sref.istft_ref(spec, fft_len, hop, normalized, trim, dtype=torch.float64)
    assert got.shape == want.shape == (batch, hop * (frames - 1))
    report(tag, audio=frac(got, want, 2e-5 * float(want.abs().max())))


@pytest.mark.parametrize("batch,frames", cs.ISTFT_IDLE)
@pytest.mark.parametrize("fft_len", cs.FFTS)
def test_istft_idle_waves(fft_len, batch, frames):
    """Frame totals (3, 15, 2) that are no multiple of the workgroup's 4 (2 at 1024 points) frames."""
    hop = cs.HOP if fft_len < 1024 else 100
    _istft_check(f"istft idle {fft_len} b{batch} t{frames}", fft_len, hop, batch, frames, False, True)


@pytest.mark.parametrize("fft_len", [256, 512])
def test_istft_hops(fft_len):
    """Hops from 1 to n_fft: the first / last covering frame of the overlap-add in every regime; n_fft + 1 is refused."""
    import maavss_amd
    from maavss_amd import _lib
    for hop, frames in cs.istft_hops(fft_len):
        for trim in (False, True):
            _istft_check(f"istft hop {fft_len} hop{hop} t{frames}{' trimmed' if trim else ''}", fft_len, hop, 2, frames, trim, True)
    _istft_check(f"istft hop {fft_len} hop133 t7 not normalized", fft_len, 133, 2, 7, False, False)
    # "hop larger than the window" is a MAAVSS_CHECK_ARG ahead of both launches (stft.hip)
    st = maavss_amd.STFT(fft_len, fft_len + 1)
    with pytest.raises(_lib.MaavssError, match="hop larger than the window"):
        st.inverse(cs.noise_like((2, 2, 7, fft_len // 2 + 1), 11).cuda())


def test_istft_padded_output_rows():
    """audio_stride > hop * (frames - 1) through the C-ABI: the gap between rows keeps its sentinel."""
    import maavss_amd
    from maavss_amd import _lib
    fft_len, hop, batch, frames = 512, 133, 3, 5
    out_len, stride = hop * (frames - 1), hop * (frames - 1) + 29
    spec = cs.noise_like((batch, 2, frames, fft_len // 2 + 1), 11)
    st = maavss_amd.STFT(fft_len, hop)
    ws = torch.empty(batch, frames, fft_len, device="cuda")
    audio, specc = guarded(batch * stride), spec.cuda()
    _lib.call("maavss_istft", _lib.ptr(specc), batch, frames, fft_len // 2 + 1, _lib.ptr(st.raw_window), fft_len, hop, 1, _lib.ptr(ws),
              _lib.ptr(audio), stride, _lib.stream_ptr())
    torch.cuda.synchronize()
    rows = audio[:batch * stride].view(batch, stride)
    assert guard_intact(audio, batch * stride) and bool((rows[:, out_len:] == SENTINEL).all())
    want = sref.istft_ref(spec, fft_len, hop, dtype=torch.float64)
    report(f"istft padded rows {fft_len} hop{hop} stride{stride}", audio=frac(rows[:, :out_len], want, 2e-5 * float(want.abs().max())))


# ------------------------------------------------------------------------------------------------------------ C. LSTM
@pytest.mark.parametrize("b,l", cs.LSTM_CASES)
def test_lstm_slab_edges(b, l):
    """test_lstm's arrangement and tolerances at one short, one exact, one over-full and two-plus-one batch slabs of 32 and at L = 1, 2
    (a step that is first and last; both neighbours at an end), against torch.nn.LSTM in float64; the saved state hp / gs / cs
    against the float64 step twin.  gs and cs take the output's tolerance (1e-4 / 1e-5): h = o tanh(c) passes their error on with
    a factor of at most 1, so a kernel that meets it on h and misses it on them would be wrong in what the backward reads."""
    from maavss_amd import ops
    lstm, x, dout = cs.lstm_problem(b, l)
    x = x.requires_grad_(True)
    out_ref, _ = lstm(x)
    grads = torch.autograd.grad(out_ref, [x] + list(lstm.parameters()), dout)
    p = {k: v.detach() for k, v in lstm.named_parameters()}
    wih64 = torch.cat([p["weight_ih_l0"], p["weight_ih_l0_reverse"]], 0)
    wih, whf, whb = wih64.float().cuda(), p["weight_hh_l0"].float().cuda(), p["weight_hh_l0_reverse"].float().cuda()
    xc = x.detach().float().cuda().reshape(b * l, cs.LSTM_IN)
    gx = ops.gemm(xc, wih, precise=True).reshape(b, l, 2, 4, 256)
    av, hp, gs, c = ops.lstm_fwd(gx, whf, whb)
    f = dict(out=frac(av, out_ref, 1e-5, 1e-4))
    # saved state
    _, hp64, gs64, c64 = eref.lstm_bidir_steps_f64((x.detach() @ wih64.T).view(b, l, 2, 4, 256), p["weight_hh_l0"], p["weight_hh_l0_reverse"])
    assert float(hp[:, 0, 0].abs().max()) == 0 and float(hp[:, l - 1, 1].abs().max()) == 0
    if l > 1:
        assert torch.equal(hp[:, 1:, 0], av[:, :-1, :256]) and torch.equal(hp[:, :-1, 1], av[:, 1:, 256:])
    f.update(hp=frac(hp, hp64, 1e-5, 1e-4), gs=frac(gs, gs64, 1e-5, 1e-4), cs=frac(c, c64, 1e-5, 1e-4))
    # backward
    dgx = ops.lstm_bwd(dout.float().cuda(), whf, whb, gs, c).reshape(b * l, 2048)
    dx = ops.gemm(dgx, wih, trans_b=True, precise=True).reshape(b, l, cs.LSTM_IN)
    f.update(dx=frac(dx, grads[0], 2e-5, 1e-3))
    dwih = ops.gemm(dgx, xc, trans_a=True, trans_b=True, precise=True)
    hp2 = hp.reshape(b * l, 512)
    dwhf = ops.gemm(dgx[:, :1024].contiguous(), hp2[:, :256].contiguous(), trans_a=True, trans_b=True, precise=True)
    dwhb = ops.gemm(dgx[:, 1024:].contiguous(), hp2[:, 256:].contiguous(), trans_a=True, trans_b=True, precise=True)
    f.update(dwih_f=frac(dwih[:1024], grads[1], 1e-4, 1e-3), dwih_b=frac(dwih[1024:], grads[3], 1e-4, 1e-3),
             dwhh_f=frac(dwhf, grads[2], 1e-4, 1e-3), dwhh_b=frac(dwhb, grads[4], 1e-4, 1e-3))
    report(f"lstm b{b} L{l}", **f)


# ------------------------------------------------------------------------------------------------------------ D. small kernels
@pytest.mark.parametrize("shape", cs.POOL_SHAPES)
def test_adaptive_pool(shape):
    """Forward and backward against F.adaptive_avg_pool2d in float64 within the derived bounds (oracle/f32_edges_ref.py), contiguous
    and with the strides the model passes to write the audio half of the LSTM sequence buffer [B][C][2 ts] (os_b = C 2 ts, os_p = 1,
    os_c = 2 ts, destination offset ts): same values bit for bit, nothing outside the addressed set touched."""
    from maavss_amd import _lib
    b, h, w, c, ho, wo = shape
    ts = ho * wo
    x, dout = cs.pool_problem(shape)
    want, dwant = cs.pool_ref(x, dout, ho, wo)
    xc = x.permute(0, 2, 3, 1).contiguous().cuda()                              # NHWC
    st = _lib.stream_ptr()
    # forward
    out = guarded(b * ts * c)
    _lib.call("maavss_adaptive_pool_fwd", _lib.ptr(xc), _lib.ptr(out), b, h, w, c, ho, wo, ts * c, c, 1, st)
    seq = guarded(b * c * 2 * ts)
    _lib.call("maavss_adaptive_pool_fwd", _lib.ptr(xc), seq.data_ptr() + 4 * ts, b, h, w, c, ho, wo, c * 2 * ts, 1, 2 * ts, st)
    torch.cuda.synchronize()
    assert guard_intact(out, b * ts * c) and guard_intact(seq, b * c * 2 * ts)
    got = out[:b * ts * c].view(b, ho, wo, c).permute(0, 3, 1, 2)              # -> [B, C, Ho, Wo]
    seqv = seq[:b * c * 2 * ts].view(b, c, 2 * ts)
    assert bool((seqv[:, :, :ts] == SENTINEL).all())                            # the video half is not this kernel's
    assert torch.equal(seqv[:, :, ts:].reshape(b, c, ho, wo), got)
    ffwd = float(((got.double().cpu() - want).abs() / eref.adaptive_pool_fwd_bound(x, ho, wo)).max())
    # backward: the strided gradient buffer holds 1e6 wherever the kernel has no business reading
    dc = dout.permute(0, 2, 3, 1).contiguous().cuda()
    dx = guarded(b * h * w * c)
    _lib.call("maavss_adaptive_pool_bwd", _lib.ptr(dc), _lib.ptr(dx), b, h, w, c, ho, wo, ts * c, c, 1, st)
    dseq = torch.full((b, c, 2 * ts), 1e6, device="cuda")
    dseq[:, :, ts:] = dout.reshape(b, c, ts).cuda()
    dx2 = guarded(b * h * w * c)
    _lib.call("maavss_adaptive_pool_bwd", dseq.data_ptr() + 4 * ts, _lib.ptr(dx2), b, h, w, c, ho, wo, c * 2 * ts, 1, 2 * ts, st)
    torch.cuda.synchronize()
    assert guard_intact(dx, b * h * w * c) and guard_intact(dx2, b * h * w * c)
    assert torch.equal(dx, dx2)
    gdx = dx[:b * h * w * c].view(b, h, w, c).permute(0, 3, 1, 2)
    fbwd = float(((gdx.double().cpu() - dwant).abs() / eref.adaptive_pool_bwd_bound(dout, h, w)).max())
    report(f"adaptive_pool {shape}", fwd=ffwd, bwd=fbwd)


def _with_specials(t):
    """+0, -0, a positive and a negative subnormal, the smallest normal, in the first row"""
    sp = torch.tensor([0.0, -0.0, 1e-40, -1e-39, 1.1754944e-38])
    t.view(-1)[:5] = sp
    return t


@pytest.mark.parametrize("rows,n", [(3, 5), (37, 4112), (1100, 1000)])
def test_bias_act_and_leaky_bwd_bit_exact(rows, n):
    """z + bias, LeakyReLU and its backward are one or two correctly rounded float32 operations (an add, then a select or a multiply:
    nothing to contract), so the kernel must equal torch float32 on the CPU bit for bit, signed zeros and subnormals included.
    1100 x 1000 elements pass the 4096 x 256 threads of one grid pass."""
    from maavss_amd import _lib, ops
    z = _with_specials(cs.noise_like((rows, n), 1))
    bias = cs.noise_like((n,), 2)
    bias[:5] = torch.tensor([-0.0, -0.0, 0.0, 1e-39, -1.1754944e-38])       # -> +0, -0, subnormal, +0, +0
    slope = 0.3
    s32 = torch.tensor(slope, dtype=torch.float32)
    for act in (ops.ACT_NONE, ops.ACT_LEAKY):
        for bvec in (bias, None):
            v = z + bvec if bvec is not None else z.clone()
            want = torch.where(v > 0, v, v * s32) if act == ops.ACT_LEAKY else v
            got = ops.bias_act_(z.cuda().clone(), None if bvec is None else bvec.cuda(), act, slope)
            assert bits_equal(got, want), (act, bvec is not None, int((got.cpu().view(torch.int32) != want.view(torch.int32)).sum()))
    out, dout = _with_specials(cs.noise_like((rows, n), 3)), cs.noise_like((rows, n), 4)      # out = +-0 takes the slope branch
    dout.view(-1)[5:10] = torch.tensor([0.0, -0.0, 1e-40, -1e-39, 3e-38])
    out.view(-1)[5:10] = torch.tensor([1.0, -1.0, -1.0, -1.0, -1.0])        # -> +0, -0 * slope, subnormal products
    want = torch.where(out > 0, dout, dout * s32)
    assert bits_equal(ops.leaky_bwd(dout.cuda(), out.cuda(), slope), want)
    print(f"[bias_act / leaky_bwd {rows} x {n}] bit-identical to float32 torch", flush=True)
    if rows == 3:
        # refused by MAAVSS_CHECK_ARG ahead of the launch (elementwise.hip): act other than 0 / 3, a slope that is not positive
        for act in (1, 2, 4):
            with pytest.raises(_lib.MaavssError, match="act must be 0 or 3"):
                ops.bias_act_(z.cuda().clone(), bias.cuda(), act, slope)
        for bad in (0.0, -0.3):
            with pytest.raises(_lib.MaavssError, match="slope must be > 0"):
                ops.leaky_bwd(dout.cuda(), out.cuda(), bad)


@pytest.mark.parametrize("rows,c,layout", cs.CSUM_CASES)
def test_channel_sum(rows, c, layout):
    """out[c] (+)= sum over rows, for row counts around the block's 256 threads, with a padded row stride and in the NCHW form, within
    (rows - 1) u sum|x| (+ u |result| for the beta add); integer inputs, whose every partial sum is exact, must give the exact sum."""
    from maavss_amd import _lib

    def run(x, prior, beta):
        if layout == "rows":
            buf, rs, chs = x.contiguous(), c, 1
        elif layout == "pad":
            buf, rs, chs = torch.full((rows, c + 3), 1e6), c + 3, 1
            buf[:, :c] = x
        else:
            buf, rs, chs = x.t().contiguous(), 1, rows
        out = guarded(c)
        out[:c] = prior.cuda()                       # beta = 0 must overwrite it
        buf = buf.cuda()
        _lib.call("maavss_channel_sum", _lib.ptr(buf), _lib.ptr(out), rows, c, rs, chs, beta, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert guard_intact(out, c)
        return out[:c].double().cpu()

    x, prior = cs.csum_problem(rows, c)
    xi, pi = cs.csum_integers(rows, c)
    f = {}
    for beta in (0, 1):
        want, bound = eref.channel_sum_bound(x, prior if beta else None)
        got = run(x, prior, beta)
        # one row: the sum is the element itself
        f[f"beta{beta}"] = float(((got - want).abs() / bound).max()) if rows > 1 or beta else 2.0 * float((got != want).any())
        wanti, _ = eref.channel_sum_bound(xi, pi if beta else None)
        assert torch.equal(run(xi, pi, beta), wanti), (beta, "integer inputs")
    report(f"channel_sum rows{rows} C{c} {layout}", **f)


@pytest.mark.parametrize("n,H,W,h,w", [(3, 224, 224, 64, 64), (2, 37, 53, 16, 20), (2, 16, 20, 37, 53), (1, 5, 7, 5, 7), (2, 9, 1, 4, 1),
                                       (2, 1, 9, 1, 4), (70, 64, 64, 128, 128)])
def test_resize_bilinear(n, H, W, h, w):
    """test_video_phasegram_with_resize's reference and 2e-6 (inputs in [0, 1)) at odd down- and up-sampling ratios, a one-pixel axis
    and more outputs (70 x 128 x 128) than the 4096 x 256 threads of one grid pass; the identity must be bit-exact."""
    from maavss_amd import _lib
    x = torch.rand(n, H, W, generator=torch.Generator().manual_seed(3))
    want = F.interpolate(x[:, None], size=(h, w), mode="bilinear", align_corners=False)[:, 0]
    out = guarded(n * h * w)
    xc = x.cuda()
    _lib.call("maavss_resize_bilinear", _lib.ptr(xc), _lib.ptr(out), n, H, W, h, w, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert guard_intact(out, n * h * w)
    got = out[:n * h * w].view(n, h, w)
    if (H, W) == (h, w):
        assert torch.equal(got.cpu(), x)
    report(f"resize_bilinear {n}x{H}x{W} -> {h}x{w}", out=frac(got, want, 2e-6))
