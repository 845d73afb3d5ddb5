"""maavss_amd.Reverb on the GPU against its float64 twin (tests/reverb_twin.py).  The convolution must give the twin's bytes at every
output: tile and chunk edges, rows with and without history, shared and permuted rooms, non-finite samples.  The bank-fed form must
hear a clip's own recording and nothing else.  Synthesis is held to one f32 ulp of the twin's taps (its exp is not numpy's) and, drawn
from a seed, to the request it was made for.  Every library call runs under torch's sync debug mode "error": none may synchronise."""
import contextlib

import numpy as np
import pytest
import torch

import reverb_twin as tw
import maavss_amd
from maavss_amd import ClipBank, Reverb

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def nosync():
    torch.cuda.set_sync_debug_mode("error")                  # any blocking call of torch's raises
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _table(h):
    """A Reverb whose table is the given taps [R, K] (no synthesis)."""
    h = np.atleast_2d(np.asarray(h, dtype=np.float32))
    rv = Reverb(h.shape[1])
    rv.rirs = torch.from_numpy(h).cuda()
    return rv


def _taps(rng, rooms, k_taps):
    h = rng.standard_normal((rooms, k_taps)) * np.exp(-4.0 * np.arange(k_taps) / k_taps)
    h[:, 0] = 1.0
    return h.astype(np.float32)


def _rows(buf, b, length, stride, lead):
    """[b, length] rows of the 1-D device buffer, row r from sample lead + r * stride."""
    return buf.as_strided((b, length), (stride, 1), lead)


def _same(got, want):
    got = np.ascontiguousarray(got.cpu().numpy())
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, f"{bad.size} of {got.size} outputs differ from the twin, first at {bad[0]}: {got.ravel()[bad[0]]!r} != {want.ravel()[bad[0]]!r}"


# K: 1, 2, around one wave's 64, 257, above one LDS chunk of 1024 taps (1100) and above two (2049).  L: 1, 5, around 256, 1000 (under
# one workgroup's 1024 outputs), 1030 and 2100 (two and three workgroups a row), L < K twice.  lead: 0, a few, more than K - 1.
# stride: None = rows back to back; 3 = rows that overlap, starting at an odd 4-byte offset
CASES = [
    (1, 1, 1, 0, None, "one"), (2, 5, 2, 3, None, "perm"), (63, 255, 3, 0, None, "perm"), (64, 256, 4, 7, None, "shared"),
    (65, 257, 5, 100, None, "perm"), (65, 257, 3, 7, 3, "perm"), (257, 1000, 2, 0, None, "one"), (257, 5, 3, 300, None, "perm"),
    (1100, 1000, 2, 50, None, "perm"), (1100, 2100, 2, 1500, None, "shared"), (2049, 1030, 1, 0, None, "perm"),
]


@pytest.mark.parametrize("k_taps,length,b,lead,stride,rooms", CASES)
def test_convolution_is_the_twin_bit_for_bit(k_taps, length, b, lead, stride, rooms):
    rng = np.random.default_rng(k_taps * 7 + length)
    n_rooms = 1 if rooms == "one" else 3
    h = _taps(rng, n_rooms, k_taps)
    index = {"one": np.zeros(b), "shared": np.full(b, 2), "perm": np.arange(b)[::-1] % n_rooms}[rooms].astype(np.int32)
    stride = length if stride is None else stride
    src = rng.standard_normal(lead + (b - 1) * stride + length + 3).astype(np.float32)
    start = [lead + r * stride for r in range(b)]
    want = tw.reverb(src, start, [s - lead for s in start], length, h, index)
    rv = _table(h)
    audio = _rows(torch.from_numpy(src).cuda(), b, length, stride, lead)
    with nosync():
        got = rv(audio, torch.from_numpy(index), lead=lead)
        again = rv(audio, torch.from_numpy(index), lead=lead)
        alone = [rv(audio[r:r + 1], torch.from_numpy(index[r:r + 1]), lead=lead) for r in range(b)]
    _same(got, want)
    assert torch.equal(got, again), "two runs give identical bytes"
    assert all(torch.equal(alone[r][0], got[r]) for r in range(b)), "a row alone equals its row in the batch"
    if lead:                                                  # the history is heard: the zero-state result is another one
        with nosync():
            dry_start = rv(audio, torch.from_numpy(index))
        _same(dry_start, tw.reverb(src, start, start, length, h, index))
        assert k_taps == 1 or not torch.equal(dry_start, got)


def test_one_tap_of_one_returns_the_input_bytes():
    rng = np.random.default_rng(1)
    src = rng.standard_normal(3 * 300).astype(np.float32)
    src[[5, 400]] = [-0.0, 1e-42]                            # a negative zero becomes +0.0 + (-0.0) = +0.0: the one exception, by IEEE
    audio, rv = torch.from_numpy(src).cuda().view(3, 300), _table([[1.0]])
    with nosync():
        out = rv(audio, torch.zeros(3, dtype=torch.int32))
    want = src.copy()
    want[5] = 0.0
    assert out.cpu().numpy().tobytes() == want.tobytes()


def test_non_finite_samples_reach_the_k_outputs_behind_them_and_no_others():
    rng = np.random.default_rng(2)
    k_taps, length, lead = 65, 600, 80
    h = _taps(rng, 2, k_taps)
    h[1, 7] = 0.0                                             # a zero tap is not skipped: 0 * inf is a NaN
    src = rng.standard_normal(lead + 2 * length).astype(np.float32)
    src[lead + 100], src[lead + length + 300], src[lead - 10] = np.nan, np.inf, -np.inf
    index = np.array([0, 1], dtype=np.int32)
    start = [lead, lead + length]
    want = tw.reverb(src, start, [0, length], length, h, index)
    rv, audio = _table(h), _rows(torch.from_numpy(src).cuda(), 2, length, length, lead)
    with nosync():
        got = rv(audio, torch.from_numpy(index), lead=lead)
    got = got.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    assert got[fin].tobytes() == want[fin].tobytes() and np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
    hit = np.zeros((2, length), dtype=bool)
    hit[0, 100:100 + k_taps], hit[1, 300:300 + k_taps], hit[0, :k_taps - 10] = True, True, True
    assert not (~fin & ~hit).any() and (~fin)[0, 100:100 + k_taps].all() and (~fin)[1, 300:300 + k_taps].all()
    assert np.isnan(got[1, 307]), "inf under the zero tap"


def test_out_is_written_where_it_should_be_and_nowhere_else():
    rng = np.random.default_rng(3)
    k_taps, length, b, ld = 65, 257, 3, 263
    h = _taps(rng, 2, k_taps)
    src = rng.standard_normal(b * length).astype(np.float32)
    index = torch.tensor([1, 0, 1], dtype=torch.int32)
    rv = _table(h)
    sentinel = float(np.float32(-1234.5))
    room = torch.full((5 + b * ld + 5,), sentinel, device="cuda")
    out = room.as_strided((b, length), (ld, 1), 5)
    start = torch.arange(b, dtype=torch.int64) * length
    src_d = torch.from_numpy(src).cuda()
    with nosync():
        rv._convolve(src_d.data_ptr(), src.size, start, start, index, length, out)
    _same(out, tw.reverb(src, start.tolist(), start.tolist(), length, h, index.numpy()))
    mask = torch.ones_like(room, dtype=torch.bool)
    mask.as_strided((b, length), (ld, 1), 5).fill_(False)
    assert bool((room[mask] == sentinel).all()), "the ld_out padding and the floats around out are untouched"
    # the entry point's own refusals, on the host copy of the tables and on the pointers
    for bad_start, bad_floor, bad_index, match in ((start + 1, start, index, "lies outside src"), (start, start + 1, index, r"floor .* must be in \[0, start"),
                                                   (start, start, torch.tensor([1, 2, 0], dtype=torch.int32), r"response 2 is outside \[0, 2\)")):
        with pytest.raises(maavss_amd._lib.MaavssError, match=match):
            rv._convolve(src_d.data_ptr(), src.size, bad_start, bad_floor, bad_index, length, out)
    with pytest.raises(maavss_amd._lib.MaavssError, match="out overlaps src"):
        rv._convolve(src_d.data_ptr(), src.size, start[:1], start[:1], index[:1], length, src_d[100:100 + length].view(1, length))
    with pytest.raises(maavss_amd._lib.MaavssError, match="out overlaps rirs"):
        rv._convolve(src_d.data_ptr(), src.size, start[:1], start[:1], index[:1], 100, rv.rirs.view(-1)[10:110].view(1, 100))
    assert bool((room[mask] == sentinel).all())


# ---- the clip bank ---------------------------------------------------------------------------------------------------------------------
S, T, FRAME_HOP, HPF, HOP = 16, 5, 2, 8, 66                  # clips of 2640 samples, starting 0, 1067, 2133 into a recording


def _bank(seed=4):
    g = torch.Generator().manual_seed(seed)
    bank = ClipBank(S, T, FRAME_HOP, HPF, HOP, capacity_frames=32, capacity_samples=12000)
    for frames, samples in ((9, 6000), (7, 5000)):
        bank.add_recording((torch.rand(samples, generator=g) - 0.5).cuda(), maps=torch.rand(frames, 4, generator=g).cuda())
    assert len(bank) == 5 and bank.recordings[1][1] == 4773
    return bank


def test_bank_clips_hear_their_own_recording_only():
    bank = _bank()
    bank.audio[4773 - 100:4773] = float("nan")               # the tail of the first recording, poisoned after banking
    rng = np.random.default_rng(5)
    h = _taps(rng, 3, 257)
    rv = _table(h)
    indices, index = [3, 4, 1, 0], torch.tensor([0, 2, 1, 1], dtype=torch.int32)
    with nosync():
        wet = rv.bank_clips(bank, indices, index)
        again = rv.bank_clips(bank, indices, index, out=torch.empty(4, 2700, device="cuda")[:, 7:2647])
        _, dry = bank.batch(indices)
        zero_state = rv(dry, index)
    src = bank.audio[:bank.n_samples].cpu().numpy()
    start = [bank.clip_start(i)[1] for i in indices]
    assert start == [4773, 4773 + 1067, 1067, 0]
    want = tw.reverb(src, start, [4773, 4773, 0, 0], 2640, h, index.numpy())
    assert np.isfinite(want).all() and bool(torch.isfinite(wet).all()), "no clip of the second recording hears the first one's tail"
    _same(wet, want)
    assert torch.equal(again, wet)
    assert not torch.equal(wet[1], zero_state[1]) and not torch.equal(wet[2], zero_state[2]), "a clip inside a recording hears its past"
    assert torch.equal(wet[0], zero_state[0]) and torch.equal(wet[3], zero_state[3]), "a recording's first clip starts from silence"
    # one tap of 1: the bank's own clips
    one = _table([[1.0]])
    with nosync():
        same = one.bank_clips(bank, indices)
    assert same.cpu().numpy().tobytes() == dry.cpu().numpy().tobytes()


# ---- synthesis -------------------------------------------------------------------------------------------------------------------------
def test_synthesis_from_given_noise_is_within_an_ulp_of_the_twin():
    k_taps, sr = 1500, 16000
    rng = np.random.default_rng(6)
    noise = rng.standard_normal((6, k_taps)).astype(np.float32)
    noise[4] = 0.0                                            # a silent tail
    rt60, drr, pre = [0.05, 0.2, 0.5, 0.03, 0.2, 0.2], [0.0, 12.0, -3.0, 6.0, 3.0, 3.0], [1, 16, 80, 1027, 5, k_taps + 3]
    rv, noise_d = Reverb(k_taps, sr=sr), torch.from_numpy(noise).cuda()
    with nosync():
        rirs = rv.make_rirs(6, rt60=rt60, drr_db=drr, predelay=torch.tensor(pre), noise=noise_d)
        again = Reverb(k_taps, sr=sr).make_rirs(6, rt60=rt60, drr_db=drr, predelay=torch.tensor(pre), noise=noise_d)
    assert rirs is rv.rirs and rirs.shape == (6, k_taps) and torch.equal(rirs, again)
    got = rirs.cpu().numpy()
    identical = total = 0
    for r in range(6):
        want, _, s = tw.rir(noise[r], tw.lam_of(rt60[r], sr), 10.0 ** (drr[r] / 10.0), pre[r])
        k0 = min(pre[r], k_taps)
        assert got[r, 0] == 1.0 and not got[r, 1:k0].any() and not np.signbit(got[r, :k0]).any(), "the direct path and the predelay are exact"
        d = tw.ulp_distance_f32(got[r], want)
        assert d.max() <= tw.TAP_ULPS, (r, int(d.max()), int(d.argmax()))
        identical, total = identical + int((d == 0).sum()), total + k_taps
        if r >= 4:
            assert s == 0.0 and got[r].tobytes() == want.tobytes() and got[r, 1:].tobytes() == bytes(4 * (k_taps - 1)), "zero energy: [1, 0, ...]"
        else:
            assert abs(tw.drr_db(got[r], k0) - drr[r]) <= tw.drr_bound_db(k_taps)
    print(f"[reverb] {identical} of {total} taps identical to the twin's, the rest one ulp away")


def test_synthesis_from_the_seed():
    k_taps, sr, rows, k0, drr = 4096, 16000, 16, 32, 4.0
    rt60 = 2048 / sr
    rv = Reverb(k_taps, sr=sr)
    kw = dict(rt60=rt60, drr_db=drr, predelay=k0)
    with nosync():
        a = rv.make_rirs(rows, seed=12, **kw).clone()
        b = rv.make_rirs(rows, seed=12, **kw)
        c = rv.make_rirs(rows, seed=13, **kw)
        mixed = rv.make_rirs(5, seed=12, rt60=[0.05, 0.1, 0.2, rt60, 0.3], drr_db=[0.0, 1.0, 2.0, drr, 5.0], predelay=torch.tensor([1, 9, 20, k0, 64])).clone()
        part = [rv.make_rirs(r + 1, seed=12, rt60=[0.05, 0.1, 0.2, rt60, 0.3][:r + 1], drr_db=[0.0, 1.0, 2.0, drr, 5.0][:r + 1],
                             predelay=torch.tensor([1, 9, 20, k0, 64][:r + 1])).clone() for r in range(5)]
    assert torch.equal(a, b), "the same seed gives the same bytes"
    assert all(not torch.equal(a[r], c[r]) for r in range(rows)), "another seed differs"
    assert all(not torch.equal(a[0], a[r]) for r in range(1, rows)), "rows draw their own normals"
    assert all(torch.equal(part[r][r], mixed[r]) for r in range(5)), "a row does not depend on how many rows the table has"
    assert torch.equal(mixed[3], a[3]), "nor on its neighbours' parameters"
    h = a.cpu().numpy()
    assert (h[:, 0] == 1.0).all() and not h[:, 1:k0].any() and np.isfinite(h).all()
    for r in range(rows):
        assert abs(tw.drr_db(h[r], k0) - drr) <= tw.drr_bound_db(k_taps), r
    for r, (rt, d, p) in enumerate(zip([0.05, 0.1, 0.2, rt60, 0.3], [0.0, 1.0, 2.0, drr, 5.0], [1, 9, 20, k0, 64])):
        assert abs(tw.drr_db(mixed[r].cpu().numpy(), p) - d) <= tw.drr_bound_db(k_taps), r
    lam = tw.lam_of(rt60, sr)
    got, expect = tw.normal_stats(h, lam, 10.0 ** (drr / 10.0), k0), tw.normal_stats_expect(rows, k_taps, lam, k0)
    print(f"[reverb] normals over {rows} x {k_taps - k0} taps: mean {got[0]:+.4f} (se {expect[0][1]:.4f}), variance {got[1]:.4f} "
          f"(expected {expect[1][0]:.4f}, se {expect[1][1]:.4f}), lag-1 autocorrelation {got[2]:+.4f} (se {expect[2][1]:.4f})")
    for name, g, (e, se) in zip(("mean", "variance", "lag-1 autocorrelation"), got, expect):
        assert abs(g - e) <= 6.0 * se, (name, g, e, se)


def test_sampled_rooms_and_default_index():
    rv = Reverb(512)
    with nosync():
        rirs = rv.make_rirs(8, seed=3)
    rt60, drr, pre = rv.sample(8, torch.Generator().manual_seed(3))
    h = rirs.cpu().numpy()
    for r in range(8):
        assert h[r, 0] == 1.0 and not h[r, 1:int(pre[r])].any()
        assert abs(tw.drr_db(h[r], int(pre[r])) - float(drr[r])) <= tw.drr_bound_db(512)
    audio = torch.randn(4, 700, device="cuda")
    with nosync():
        got = rv(audio, seed=9)
        want = rv(audio, rv.sample_index(4, torch.Generator().manual_seed(9)))
    assert torch.equal(got, want)


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
def _serial(stft, mixer, target, dry, wet, seed):
    if target == "dry":
        return stft(wet, seed=seed)[0], stft(dry, want_x=False)[1]
    return mixer(wet, seed=seed) if mixer is not None else stft(wet, seed=seed)


CONFIGS = [("wet", False), ("dry", False), ("wet", True)]


def test_bank_fed_pipeline_with_reverb_equals_the_serial_calls():
    bank = _bank()
    stft = maavss_amd.STFT(256, HOP, noise_std=0.1, device="cuda")
    rv = Reverb(300)
    rv.make_rirs(6, seed=1)
    batches = [[4, 1], [2, 3], [0, 4]]
    for target, mixed in CONFIGS:
        mixer = maavss_amd.Mixer(stft, interferers=1) if mixed else None
        pipe = maavss_amd.ClipPipeline(None, stft, T, bank=bank, mixer=mixer, reverb=rv, reverb_target=target)
        with nosync():
            pipe.submit_clips(batches[0], seed=50)
        for i in range(len(batches)):
            with nosync():
                if i + 1 < len(batches):
                    pipe.submit_clips(batches[i + 1], seed=50 + i + 1)
                got = pipe.get()
                attn, dry = bank.batch(batches[i])
                want = _serial(stft, mixer, target, dry, rv.bank_clips(bank, batches[i], seed=50 + i), 50 + i)
            assert torch.equal(got[0], attn) and torch.equal(got[1], want[0]) and torch.equal(got[2], want[1]), (target, mixed, i)
            pipe.release()
        pipe.drain()
    # without a reverb: the bytes of a pipeline built without the argument
    plain, none = maavss_amd.ClipPipeline(None, stft, T, bank=bank), maavss_amd.ClipPipeline(None, stft, T, bank=bank, reverb=None)
    for p in (plain, none):
        p.submit_clips(batches[0], seed=50)
    assert all(torch.equal(x, y) for x, y in zip(plain.get(), none.get()))
    assert set(none.slots[0]) == set(plain.slots[0])
    wet_pipe = maavss_amd.ClipPipeline(None, stft, T, bank=bank, reverb=rv)
    wet_pipe.submit_clips(batches[0], seed=50)
    assert not torch.equal(wet_pipe.get()[1], plain.get()[1]), "the reverb changes what the network sees"


def test_frames_fed_pipeline_with_reverb_equals_the_serial_calls():
    from oracle import stft_ref_cpu as sref, vit_ref_cpu as vref
    b, t, w, fft, hpf = 2, 8, 128, 256, 8                     # the shapes of tests/test_pipeline_gpu.py
    hop, length, _ = maavss_amd.calc_hop_size(t, hpf, 30, 16000)
    va = maavss_amd.VideoAttention(path_to_weights="/nonexistent.pth")
    va.load_state_dict(vref.seeded_vit_state(3))
    stft = maavss_amd.STFT(fft, hop, noise_std=0.1, device="cuda")
    rv = Reverb(300)
    rv.make_rirs(6, seed=1)
    frames = [vref.synthetic_frames(b * t, w, 100 + i).cuda() for i in range(3)]
    audio = [sref.synthetic_audio(b, length, 200 + i).cuda() for i in range(3)]
    attn = [va.attention_frames(f, clip_frames=t).view(b, 1, t, w, w).clone() for f in frames]
    for target, mixed in CONFIGS:
        mixer = maavss_amd.Mixer(stft, interferers=1) if mixed else None
        pipe = maavss_amd.ClipPipeline(va, stft, t, mixer=mixer, reverb=rv, reverb_target=target)
        pipe.submit(frames[0], audio[0], seed=70)
        for i in range(3):
            if i + 1 < 3:
                pipe.submit(frames[i + 1], audio[i + 1], seed=70 + i + 1)
            got = pipe.get()
            with nosync():
                want = _serial(stft, mixer, target, audio[i], rv(audio[i], seed=70 + i), 70 + i)
            assert torch.equal(got[0], attn[i]) and torch.equal(got[1], want[0]) and torch.equal(got[2], want[1]), (target, mixed, i)
            pipe.release()
        pipe.drain()
    explicit = torch.tensor([5, 0], dtype=torch.int32)
    pipe.submit(frames[0], audio[0], seed=70, rir_index=explicit)
    assert torch.equal(pipe.get()[1], mixer(rv(audio[0], explicit), seed=70)[0])
    plain, none = maavss_amd.ClipPipeline(va, stft, t), maavss_amd.ClipPipeline(va, stft, t, reverb=None)
    for p in (plain, none):
        p.submit(frames[0], audio[0], seed=70)
    assert all(torch.equal(x, y) for x, y in zip(plain.get(), none.get()))
