"""ClipBank (maavss_amd/clip_bank.py, csrc/clip_bank.hip) on the MI355X: the 16-bit pack against tests/bank_twin.py, batches from an
f32 bank against the extractor itself, batches from synthetic maps against the definition written in torch ops, the audio gather
against slices, and the bank-fed ClipPipeline against the frames-fed one -- all bit for bit.  Shapes are the smallest that reach
every edge: frames of 132 (4 pixels outside the patch grid) and of 8 (one patch), clips of 111 samples at odd offsets, batches of 1
and 7, recordings placed so that any read across a boundary changes the result."""
import numpy as np
import pytest
import torch

import bank_twin as tw
import maavss_amd
from maavss_amd import ClipBank, _lib
from maavss_amd._lib import call, ptr, stream_ptr

pytestmark = pytest.mark.gpu


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _pack_values(n, seed):
    """Crafted values first, then seeded ones: inside [0, 1], around it, and on the half-way points (k + 0.5) / 65535."""
    r = np.random.default_rng(seed)
    k = r.integers(0, 65535, n).astype(np.float64)
    v = np.concatenate([np.array(tw.CRAFTED), r.random(n), r.random(n) * 1.4 - 0.2, (k + 0.5) / 65535, k / 65535])
    return v.astype(np.float32)[:n] if n < 8 else r.permutation(v.astype(np.float32))[:n]


@pytest.mark.parametrize("n", [1, 255, 1027])
def test_pack_and_unpack_are_the_twin_bit_for_bit(n):
    v = _pack_values(n, n)
    if n >= 255:
        v[:8] = np.array(tw.CRAFTED, dtype=np.float32)
        v[8:11] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    dev = torch.from_numpy(v).cuda()
    q = torch.full((n + 2,), 0x5a5a, device="cuda", dtype=torch.int16)
    call("maavss_bank_pack_u16", ptr(dev), ptr(q[1:]), n, stream_ptr())
    assert _u16(q[1:n + 1]).tolist() == tw.pack(v).tolist()
    assert q[0].item() == 0x5a5a and q[n + 1].item() == 0x5a5a, "pack wrote outside its n values"
    codes = np.random.default_rng(n + 1).integers(0, 65536, n).astype(np.uint16)
    codes[0] = 65535
    out, codes_dev = torch.full((n + 2,), 7.0, device="cuda"), torch.from_numpy(codes.view(np.int16)).cuda()
    call("maavss_bank_unpack_u16", ptr(codes_dev), ptr(out[1:]), n, stream_ptr())
    assert out[1:n + 1].cpu().numpy().view(np.uint32).tolist() == tw.unpack(codes).view(np.uint32).tolist()
    assert out[0].item() == 7.0 and out[n + 1].item() == 7.0 and out[1].item() == 1.0


def test_unpack_of_every_code_is_the_correctly_rounded_quotient():
    codes = np.arange(65536, dtype=np.uint16)
    out, codes_dev = torch.empty(65536, device="cuda"), torch.from_numpy(codes.view(np.int16)).cuda()
    call("maavss_bank_unpack_u16", ptr(codes_dev), ptr(out), 65536, stream_ptr())
    assert np.array_equal(out.cpu().numpy().view(np.uint32), tw.unpack(codes).view(np.uint32))
    back = torch.empty(65536, device="cuda", dtype=torch.int16)
    call("maavss_bank_pack_u16", ptr(out), ptr(back), 65536, stream_ptr())
    assert np.array_equal(_u16(back), codes)


# ---- f32 bank against the extractor ------------------------------------------------------------------------------------------
W, T, FRAME_HOP, HPF, HOP = 128, 5, 2, 8, 66
N = HPF * HOP * T


@pytest.fixture(scope="module")
def vit_bank():
    from oracle import stft_ref_cpu as sref, vit_ref_cpu as vref
    va = maavss_amd.VideoAttention(path_to_weights="/nonexistent.pth")
    va.load_state_dict(vref.seeded_vit_state(3))
    recs = [(vref.synthetic_frames(n, W, 300 + i), sref.synthetic_audio(1, 4000 + 2 * N + 33 * i, 400 + i)[0]) for i, n in enumerate((9, 6))]
    bank = ClipBank(W, T, FRAME_HOP, HPF, HOP, capacity_frames=16, capacity_samples=12000)
    step, va.frames_per_launch = va.frames_per_launch, 4          # 9 frames in launches of 4, 4 and 1
    try:
        counts = [bank.add_recording(a.cuda(), frames=f.cuda(), video_attention=va) for f, a in recs]
    finally:
        va.frames_per_launch = step
    assert counts == [3, 1] and len(bank) == 4
    return va, bank, recs


@pytest.mark.parametrize("attn_diff", [False, True])
def test_f32_bank_gives_what_the_extractor_gives(vit_bank, attn_diff):
    va, bank, recs = vit_bank
    indices = [0, 2, 3, 3, 0]              # first and last clip of recording 0, first = last clip of recording 1, a duplicate
    attn, audio = bank.batch(indices, attn_diff=attn_diff)
    assert attn.shape == (5, 1, T, W, W) and audio.shape == (5, N)
    for b, idx in enumerate(indices):
        r, k = bank.locate(idx)
        frames, wave = recs[r]
        v, s = k * FRAME_HOP, tw.sample_start(k, FRAME_HOP, 30, 16000)
        want = va.attention_frames(frames[v:v + T].cuda(), clip_frames=T, attn_diff=attn_diff)
        assert torch.equal(attn[b, 0], want[:, 0]), f"clip {idx} (recording {r}, k = {k}) differs from attention_frames(attn_diff={attn_diff})"
        assert torch.equal(audio[b].cpu(), wave[s:s + N]), f"clip {idx}: audio"


# ---- synthetic maps: the definition in torch ops ---------------------------------------------------------------------------------
def _maps(n_frames, elems, seed):
    g = torch.Generator().manual_seed(seed)
    # odd frames lie above even ones: every clip of 3 frames holds a rise, so the temporal difference has a positive maximum with a
    # single patch too (a maximum of 0 makes both sides 0 * inf = NaN, which compares unequal to itself)
    return torch.rand(n_frames, elems, generator=g) * 0.3 + 0.1 + 0.5 * (torch.arange(n_frames)[:, None] % 2)


@pytest.mark.parametrize("attn_diff", [False, True])
@pytest.mark.parametrize("storage", ["f32", "u16"])
@pytest.mark.parametrize("size", [132, 8])
def test_batches_from_synthetic_maps_are_the_definition(size, storage, attn_diff):
    t, elems = 3, (size // 8) ** 2
    bank = ClipBank(size, t, 1, 1, 5, capacity_frames=32, capacity_samples=4000, storage=storage)
    # the recording in front ends in a frame of the largest values the storage holds: a read across the boundary changes the result
    front = _maps(4, elems, 1)
    front[-1] = 1.0 if storage == "u16" else 50.0
    tested, behind = _maps(9, elems, 2), torch.full((3, elems), 1.0 if storage == "u16" else 50.0)
    for m in (front, tested, behind):
        bank.add_recording(torch.zeros(8000).cuda(), maps=m.cuda())
    assert len(bank) == 2 + 7 + 1
    stored = tested if storage == "f32" else torch.from_numpy(tw.unpack(tw.pack(tested.numpy())))
    assert torch.equal(bank.unpacked_maps(1).cpu(), stored)
    if storage == "u16":
        assert bank.maps.dtype == torch.int16 and bank.maps.element_size() * 2 == torch.empty(0).element_size()
        assert float((stored - tested).abs().max()) <= 1 / 131070 + 2.0 ** -23
    stored = stored.cuda()
    for indices in ([2], [8, 2, 5, 3, 3, 7, 4, 6][:7]):
        attn, _ = bank.batch(indices, attn_diff=attn_diff)
        assert attn.shape == (len(indices), 1, t, size, size)
        for b, idx in enumerate(indices):
            k = idx - 2
            want = tw.expected_attn(stored[k:k + t], size, attn_diff)
            assert torch.equal(attn[b], want), f"storage {storage}, attn_diff {attn_diff}: clip {idx} of batch {indices}"
        if size % 8:
            grid = size // 8 * 8
            assert not attn[..., grid:, :].any() and not attn[..., :, grid:].any(), "pixels outside the patch grid must be 0"
        if attn_diff:
            assert not attn[:, :, 0].any(), "clip frame 0 of a temporal difference is 0"


# ---- the audio gather ----------------------------------------------------------------------------------------------------------
def test_audio_rows_are_the_slices_at_odd_offsets_and_strides():
    t, hop = 3, 37
    n = t * hop                                          # 111 samples: not a multiple of 4
    bank = ClipBank(8, t, 1, 1, hop, capacity_frames=16, capacity_samples=4000)
    g = torch.Generator().manual_seed(9)
    # 1, 4 and 2 clips; the bank keeps 111, 1711 and 644 samples of them, so recordings start at samples 0, 111 and 1822 and every
    # recording's last clip ends on its last banked sample, the next recording's different values right behind it
    waves = [torch.randn(length, generator=g) + 10.0 * i for i, length in enumerate((111, 1801, 701))]
    for wave, n_frames in zip(waves, (3, 6, 4)):
        bank.add_recording(wave.cuda(), maps=_maps(n_frames, 1, 3).cuda())
    assert len(bank) == 7 and [r[1] for r in bank.recordings] == [0, 111, 1822] and bank.n_samples == 2466
    starts = [bank.clip_start(i)[1] for i in range(7)]
    assert starts == [0, 111, 644, 1178, 1711, 1822, 2355] and any(s % 4 for s in starts)
    indices = [4, 0, 6, 1, 5, 3, 2, 4]
    want = torch.stack([waves[bank.locate(i)[0]][tw.sample_start(bank.locate(i)[1], 1, 30, 16000):][:n] for i in indices])
    _, audio = bank.batch(indices)
    assert torch.equal(audio.cpu(), want)
    attn = torch.empty(len(indices), 1, t, 8, 8, device="cuda")
    for ld in (128, 113):                                # 16-byte stores with a 3-sample tail per row; element stores
        buf = torch.full((len(indices), ld), -7.0, device="cuda")
        _, audio = bank.batch(indices, out=(attn, buf[:, :n]))
        assert audio.data_ptr() == buf.data_ptr() and torch.equal(audio.cpu(), want), ld
        assert bool((buf[:, n:] == -7.0).all()), f"ld_out = {ld}: the gather wrote behind a row's {n} samples"
    _, one = bank.batch([4])
    assert torch.equal(one.cpu(), want[:1])


def test_batch_does_not_synchronise():
    bank = ClipBank(16, 3, 1, 1, 37, capacity_frames=16, capacity_samples=4000, storage="u16")
    bank.add_recording(torch.randn(3000).cuda(), maps=_maps(8, 4, 4).cuda())
    first = bank.batch([1, 0, 3])                        # loads the library, warms the allocators
    out = (torch.empty_like(first[0]), torch.empty_like(first[1]))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")              # any blocking call of torch's raises
    try:
        second = bank.batch([1, 0, 3])
        third = bank.batch(torch.tensor([1, 0, 3]), attn_diff=True, out=out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]) and torch.equal(third[1], first[1])
    assert third[0].data_ptr() == out[0].data_ptr()


# ---- one file --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "u16"])
def test_save_and_load_round_trip(tmp_path, storage):
    bank = ClipBank(16, 3, 2, 1, 37, fps=25, sr=22050, capacity_frames=40, capacity_samples=30000, storage=storage)
    g = torch.Generator().manual_seed(6)
    for i, n_frames in enumerate((7, 4)):
        bank.add_recording(torch.randn(9000 + i, generator=g).cuda(), maps=_maps(n_frames, 4, 10 + i).cuda())
    indices = list(range(len(bank))) + [0]
    before = [bank.batch(indices, attn_diff=d) for d in (False, True)]
    path = str(tmp_path / "bank.pt")
    bank.save(path)
    payload = torch.load(path, weights_only=True)
    assert payload["maps"].dtype == (torch.int16 if storage == "u16" else torch.float32) and payload["maps"].shape[0] == bank.n_frames
    again = ClipBank.load(path, frame_size=16, storage=storage)
    assert (again.capacity_frames, again.capacity_samples) == (bank.n_frames, bank.n_samples)
    assert again.recordings == bank.recordings and len(again) == len(bank) and (again.fps, again.sr, again.frame_hop) == (25, 22050, 2)
    roomy = ClipBank.load(path, capacity_frames=64, capacity_samples=40000)
    extra = (torch.randn(9000, generator=g).cuda(), _maps(5, 4, 12).cuda())
    assert roomy.add_recording(extra[0], maps=extra[1]) == bank.add_recording(extra[0], maps=extra[1]) == 2
    with pytest.raises(ValueError, match="capacity_frames"):
        again.add_recording(extra[0], maps=extra[1])          # loaded at the stored size: full
    for loaded in (again, roomy):
        for d, (attn, audio) in zip((False, True), before):
            got = loaded.batch(indices, attn_diff=d)
            assert torch.equal(got[0], attn) and torch.equal(got[1], audio)
    last = [len(bank) - 1, len(bank) - 2]
    assert all(torch.equal(a, b) for a, b in zip(roomy.batch(last), bank.batch(last)))
    with pytest.raises(ValueError, match="frame_size 16 in the file, frame_size=24"):
        ClipBank.load(path, frame_size=24)
    other = "f32" if storage == "u16" else "u16"
    with pytest.raises(ValueError, match=f"storage '{storage}' in the file, storage='{other}'"):
        ClipBank.load(path, storage=other)
    with pytest.raises(ValueError, match="more than capacity_frames=3"):
        ClipBank.load(path, capacity_frames=3)
    payload["version"] = 0
    torch.save(payload, path)
    with pytest.raises(ValueError, match="version 0 of the ClipBank format"):
        ClipBank.load(path)
    torch.save({"maps": payload["maps"]}, path)
    with pytest.raises(ValueError, match="not a ClipBank file"):
        ClipBank.load(path)


# ---- the bank-fed pipeline ---------------------------------------------------------------------------------------------------------
def test_bank_fed_pipeline_equals_the_frames_fed_pipeline():
    from oracle import stft_ref_cpu as sref, vit_ref_cpu as vref
    b, t, w, fft, hpf, frame_hop = 2, 8, 128, 256, 8, 4              # the shapes of tests/test_pipeline_gpu.py
    hop, length, _ = maavss_amd.calc_hop_size(t, hpf, 30, 16000)
    va = maavss_amd.VideoAttention(path_to_weights="/nonexistent.pth")
    va.load_state_dict(vref.seeded_vit_state(3))
    stft = maavss_amd.STFT(fft, hop, noise_std=0.1, device="cuda")
    mixer = maavss_amd.Mixer(stft, interferers=1)
    recs = [(vref.synthetic_frames(n, w, 500 + i).cuda(), sref.synthetic_audio(1, 12000, 600 + i)[0].cuda()) for i, n in enumerate((16, 12))]
    bank = ClipBank(w, t, frame_hop, hpf, hop, capacity_frames=32, capacity_samples=24000)
    assert [bank.add_recording(a, frames=f, video_attention=va) for f, a in recs] == [3, 2]
    batches = [[4, 1], [2, 3]]

    def clips(indices):
        frames, audio = [], []
        for idx in indices:
            r, k = bank.locate(idx)
            s = tw.sample_start(k, frame_hop, 30, 16000)
            frames.append(recs[r][0][k * frame_hop:k * frame_hop + t])
            audio.append(recs[r][1][s:s + length])
        return torch.cat(frames), torch.stack(audio)

    fed = maavss_amd.ClipPipeline(va, stft, t, mixer=mixer)
    want = []
    for i, indices in enumerate(batches):
        fed.submit(*clips(indices), seed=40 + i)
    for _ in batches:
        want.append([x.clone() for x in fed.get()])
        fed.release()
    fed.drain()
    pipe = maavss_amd.ClipPipeline(None, stft, t, bank=bank, mixer=mixer)
    for i, indices in enumerate(batches):                             # both slots in flight
        pipe.submit_clips(indices, seed=40 + i)
    for i in range(len(batches)):
        got = pipe.get()
        assert got[0].shape == (b, 1, t, w, w)
        for name, x, y in zip(("attention frames", "x_stft", "y_stft"), got, want[i]):
            assert torch.equal(x, y), f"batch {i}: {name} differ from the frames-fed pipeline"
        pipe.release()
    pipe.submit_clips(batches[0], seed=40)                            # a slot reused after release()
    assert all(torch.equal(x, y) for x, y in zip(pipe.get(), want[0]))
    pipe.release()
    pipe.drain()                                                      # no extractor to ask for its finite flag
