"""The crop-and-flip of the clip bank's maps on the MI355X (maavss_bank_warp_maps, csrc/bank_warp.hip; ClipBank.batch(boxes=, flip=),
warp_maps, BankCrop, ClipPipeline(bank_crop=)) against tests/bank_warp_twin.py, bit for bit: every operation of the definition is a
correctly rounded IEEE operation, the file is compiled without contraction and the index arithmetic is integer, so there is no
tolerance.  Frames of 8 (one patch: every clamp active), 16, 24, 64 and 136 (289 patches: a thread takes two), clips of 1, 2 and 3
frames, batches of 1, 3 and 7 with duplicates.  The maps are finite and positive, so that the exactness of the whole-frame box is a
property of the definition and not of -0.0.  Every call of the library runs under torch.cuda.set_sync_debug_mode("error")."""
import numpy as np
import pytest
import torch

import bank_twin as tw
import bank_warp_twin as ww
import maavss_amd
from maavss_amd import BankCrop, ClipBank
from maavss_amd._lib import call, ptr, stream_ptr

pytestmark = pytest.mark.gpu

SIZES = (8, 16, 24, 64, 136)
HOP = 5


def _maps(n_frames, elems, seed):
    g = torch.Generator().manual_seed(seed)
    # odd frames lie above even ones: a clip of two or more frames holds a rise, so the temporal difference has a positive maximum
    return torch.rand(n_frames, elems, generator=g) * 0.3 + 0.1 + 0.5 * (torch.arange(n_frames)[:, None] % 2)


def _same(a, b):
    """Equal element for element, a NaN equal to a NaN (0 * inf where a clip's maximum is 0: the payload is the machine's)."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _nosync(fn, *args, **kw):
    torch.cuda.set_sync_debug_mode("error")              # any blocking call of torch's raises
    try:
        return fn(*args, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _box_cases(s, seed):
    """Every kind of box the definition has an edge for, on an s x s frame."""
    h = s // 2
    cases = [(0, 0, s, s),                                                    # the whole frame
             (0, 0, 1, 1), (0, s - 1, 1, 1), (s - 1, 0, 1, 1), (s - 1, s - 1, 1, 1),      # one pixel in each corner
             (h, s // 3, s - h, s - s // 3), (s - 3, 1, 3, s - 2), (2, s - 5, s - 3, 5),  # touching the bottom / right edge
             (h, 0, 1, s), (3, 0, 2, s), (0, h, s, 1), (0, 5, s, 2),                   # thin, full width / full height
             (1, 3, s - 5, h + 1), (3, 1, h, s - 2), (2, 1, 5, 3)]                     # anisotropic, not patch-aligned
    drawn = BankCrop().sample(5, s, torch.Generator().manual_seed(seed))[0].tolist()
    return cases + [tuple(b) for b in drawn]


def _bank(size, t, storage, seed=0):
    """Three recordings of 4, 2 and 1 clips (frame_hop 1) -> (bank, what bank_load returns for every banked frame)."""
    elems = (size // 8) ** 2
    bank = ClipBank(size, t, 1, 1, HOP, capacity_frames=32, capacity_samples=4000, storage=storage)
    recs = [_maps(t + 3, elems, seed + 1), _maps(t + 1, elems, seed + 2), _maps(t, elems, seed + 3)]
    g = torch.Generator().manual_seed(seed + 4)
    for m in recs:
        bank.add_recording(torch.randn(2000, generator=g).cuda(), maps=m.cuda())
    assert len(bank) == 7
    stored = torch.cat(recs).numpy()
    return bank, (stored if storage == "f32" else tw.unpack(tw.pack(stored)))


def _expected(bank, stored, indices, boxes, flip, frame_norm):
    """The twin's warped maps of a batch: float32 [B, T, hp, hp]."""
    t, s = bank.clip_frames, bank.frame_size
    out = []
    for b, idx in enumerate(indices):
        f0 = bank.clip_start(idx)[0]
        out.append(ww.warp_clip(stored[f0:f0 + t], s, boxes[b].tolist(), bool(flip[b]), frame_norm))
    return np.stack(out)


BATCHES = ([4], [6, 0, 3], [5, 2, 2, 0, 6, 3, 2])


@pytest.mark.parametrize("storage", ["f32", "u16"])
@pytest.mark.parametrize("size", SIZES)
def test_warped_maps_and_batches_are_the_twin_bit_for_bit(size, storage):
    cases = _box_cases(size, size)
    hp, k = size // 8, 0
    for t in (1, 2, 3):
        bank, stored = _bank(size, t, storage, seed=10 * t)
        plain = {len(ix): bank.batch(ix) for ix in BATCHES}                  # loads the library, warms the allocators
        torch.cuda.synchronize()
        for indices in BATCHES:
            nb = len(indices)
            boxes = torch.tensor([cases[(k + i) % len(cases)] for i in range(nb)], dtype=torch.int32)
            k += nb
            some = torch.arange(nb) % 2 == (t % 2)
            for flip in (None, some):
                for frame_norm in (True, False):
                    want = _expected(bank, stored, indices, boxes, some if flip is not None else torch.zeros(nb), frame_norm)
                    where = f"S {size}, {storage}, T {t}, clips {indices}, boxes {boxes.tolist()}, flip {flip is not None}, frame_norm {frame_norm}"
                    got = _nosync(bank.warp_maps, indices, boxes, flip, frame_norm)
                    assert got.shape == (nb, t, hp, hp) and got.dtype == torch.float32
                    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), where
                    for attn_diff in (False, True):
                        attn, audio = _nosync(bank.batch, indices, attn_diff=attn_diff, boxes=boxes, flip=flip, frame_norm=frame_norm)
                        assert attn.shape == (nb, 1, t, size, size)
                        attn = attn.cpu()
                        for b in range(nb):
                            exp = tw.expected_attn(torch.from_numpy(want[b]).reshape(t, hp * hp), size, attn_diff)
                            assert _same(attn[b], exp), f"{where}, attn_diff {attn_diff}: clip {b}"
                        assert torch.equal(audio, plain[nb][1]), f"{where}: the audio half is not batch(indices)'s"
    assert k >= len(cases), "not every box case was used"


@pytest.mark.parametrize("storage", ["f32", "u16"])
@pytest.mark.parametrize("size", [8, 24, 136])
def test_whole_frame_is_the_plain_batch_and_flip_alone_its_mirror_image(size, storage):
    bank, _ = _bank(size, 3, storage, seed=5)
    indices = BATCHES[2]
    nb = len(indices)
    whole = torch.tensor([[0, 0, size, size]] * nb, dtype=torch.int32)
    flags = torch.tensor([True, False, True, True, False, False, True])
    for attn_diff in (False, True):
        plain = bank.batch(indices, attn_diff=attn_diff)
        torch.cuda.synchronize()
        same = _nosync(bank.batch, indices, attn_diff=attn_diff, boxes=whole, frame_norm=False)
        assert torch.equal(same[0], plain[0]) and torch.equal(same[1], plain[1])
        for kw in (dict(flip=flags), dict(flip=flags.to(torch.uint8), boxes=whole)):
            flipped = _nosync(bank.batch, indices, attn_diff=attn_diff, frame_norm=False, **kw)
            want = torch.where(flags.cuda()[:, None, None, None, None], plain[0].flip(-1), plain[0])
            assert torch.equal(flipped[0], want) and torch.equal(flipped[1], plain[1])
    # the stored frames have maximum < 1, so the frame normalisation changes them: frame_norm is not silently off
    assert not torch.equal(bank.warp_maps(indices, whole), bank.warp_maps(indices, whole, frame_norm=False))


def test_a_row_of_a_batch_has_the_bytes_of_a_call_of_its_own_and_of_a_second_run():
    size, t = 136, 3
    bank, _ = _bank(size, t, "u16", seed=7)
    indices = BATCHES[2]
    cases = _box_cases(size, 3)
    boxes = torch.tensor(cases[9:9 + len(indices)], dtype=torch.int32)
    flip = torch.tensor([False, True, False, True, True, False, True])
    first = bank.batch(indices, attn_diff=True, boxes=boxes, flip=flip)
    out = (torch.full_like(first[0], 7.0), torch.full_like(first[1], 7.0))
    torch.cuda.synchronize()
    second = _nosync(bank.batch, indices, attn_diff=True, boxes=boxes, flip=flip, out=out)
    # the box inside one patch makes every frame of its clip all ones: a temporal difference of 0 and 0 * inf, a NaN on both sides
    assert second[0].data_ptr() == out[0].data_ptr() and _same(first[0], second[0]) and torch.equal(first[1], second[1])
    assert bool(first[0][5].isnan().any()) and bool(first[0][[0, 1, 2, 3, 4, 6]].isfinite().all())
    maps = bank.warp_maps(indices, boxes, flip)
    for b, idx in enumerate(indices):
        own = _nosync(bank.batch, [idx], attn_diff=True, boxes=boxes[b:b + 1], flip=flip[b:b + 1])
        assert _same(own[0][0], first[0][b]) and torch.equal(own[1][0], first[1][b]), f"clip {b}"
        assert torch.equal(_nosync(bank.warp_maps, [idx], boxes[b:b + 1], flip[b:b + 1])[0], maps[b])
    assert indices[1] == indices[2] and not torch.equal(maps[1], maps[2])            # the same clip under two boxes


@pytest.mark.parametrize("storage,elems", [(0, 1), (0, 289), (1, 9)])
def test_the_raw_entry_point_writes_its_rows_and_nothing_else(storage, elems):
    hp = int(round(elems ** 0.5))
    size, t, nb, n_frames, pad = 8 * hp, 2, 3, 7, 64
    maps = _maps(n_frames, elems, 21)
    stored = maps.numpy() if storage == 0 else tw.unpack(tw.pack(maps.numpy()))
    dev = maps.cuda() if storage == 0 else torch.from_numpy(tw.pack(maps.numpy()).view(np.int16)).cuda()
    start = torch.tensor([5, 0, 3], dtype=torch.int32)
    boxes = torch.tensor([(1, 0, size - 1, size), (size - 1, size - 1, 1, 1), (0, 2, size - 3, 5)], dtype=torch.int32)
    flips = torch.tensor([1, 0, 1, 0], dtype=torch.uint8)                    # one byte behind the three flags
    buf = torch.full((pad + nb * t * elems + pad,), -7.0, device="cuda")
    start_d, boxes_d, flips_d = start.cuda(), boxes.cuda(), flips.cuda()      # named: a temporary's memory is handed to the next one
    call("maavss_bank_warp_maps", ptr(dev), storage, ptr(start_d), ptr(boxes_d), ptr(flips_d), nb, n_frames, t, size, 1, ptr(buf[pad:]),
         stream_ptr())
    want = np.stack([ww.warp_clip(stored[s:s + t], size, boxes[b].tolist(), bool(flips[b])) for b, s in enumerate(start.tolist())])
    got = buf.cpu().numpy()
    assert np.array_equal(got[pad:-pad].view(np.uint32), want.reshape(-1).view(np.uint32))
    assert (got[:pad] == -7.0).all() and (got[-pad:] == -7.0).all(), "the kernel wrote outside its B * T * n values"
    # no flags at all: nobody is flipped
    call("maavss_bank_warp_maps", ptr(dev), storage, ptr(start_d), ptr(boxes_d), None, nb, n_frames, t, size, 0, ptr(buf[pad:]), stream_ptr())
    want = np.stack([ww.warp_clip(stored[s:s + t], size, boxes[b].tolist(), False, False) for b, s in enumerate(start.tolist())])
    assert np.array_equal(buf.cpu().numpy()[pad:-pad].view(np.uint32), want.reshape(-1).view(np.uint32))


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    from maavss_amd._lib import MaavssError
    maps, out = torch.zeros(4, 4, device="cuda"), torch.zeros(16, device="cuda")
    tab = torch.zeros(8, device="cuda", dtype=torch.int32)
    good = dict(maps=ptr(maps), storage=0, start=ptr(tab), boxes=ptr(tab), flips=None, n=1, frames=4, t=2, s=16, norm=1, out=ptr(out))
    for change, message in ((dict(maps=None), "null pointer"), (dict(start=None), "null pointer"), (dict(boxes=None), "null pointer"),
                            (dict(out=None), "null pointer"), (dict(storage=2), "storage must be 0"), (dict(s=12), "multiple of 8"),
                            (dict(s=0), "multiple of 8"), (dict(n=0), "empty problem"), (dict(t=5), "hold no clip"),
                            (dict(n=2 ** 31, t=1), "32-bit workgroup index"), (dict(n=2 ** 30, t=2), "32-bit workgroup index")):
        with pytest.raises(MaavssError, match=message):
            call("maavss_bank_warp_maps", *{**good, **change}.values(), stream_ptr())
    torch.cuda.synchronize()
    assert not out.any()


@pytest.mark.parametrize("attn_diff", [False, True])
def test_a_clip_next_to_a_recording_of_nan_stays_finite(attn_diff):
    size, t, elems = 24, 3, 9
    bank = ClipBank(size, t, 1, 1, HOP, capacity_frames=32, capacity_samples=4000)
    tested = _maps(5, elems, 31)
    for m in (torch.full((t, elems), float("nan")), tested, torch.full((t + 1, elems), float("nan"))):
        bank.add_recording(torch.zeros(2000).cuda(), maps=m.cuda())
    assert len(bank) == 1 + 3 + 2 and bank.unpacked_maps(0).isnan().all() and bank.unpacked_maps(2).isnan().all()
    indices = [1, 3, 2]                                  # first and last clip of the recording between the two, and the middle one
    boxes = torch.tensor([(0, 0, 1, 1), (size - 1, size - 1, 1, 1), (3, 1, 17, 22)], dtype=torch.int32)
    flip = torch.tensor([True, False, True])
    bank.batch(indices)
    torch.cuda.synchronize()
    attn, _ = _nosync(bank.batch, indices, attn_diff=attn_diff, boxes=boxes, flip=flip, frame_norm=False)
    assert bool(attn.isfinite().all()), "a clip read a map of the recording next to it"
    want = np.stack([ww.warp_clip(tested.numpy()[k:k + t], size, boxes[b].tolist(), bool(flip[b]), False) for b, k in enumerate((0, 2, 1))])
    for b in range(3):
        assert torch.equal(attn[b].cpu(), tw.expected_attn(torch.from_numpy(want[b]).reshape(t, elems), size, attn_diff)), b
    assert bool(_nosync(bank.warp_maps, indices, boxes, flip).isfinite().all())
    assert bool(bank.batch([0], boxes=boxes[:1])[0].isnan().any())              # the poison is where it was put


def test_bank_fed_pipeline_with_bank_crop_equals_the_serial_calls():
    b, t, size, fft, hpf, frame_hop = 2, 8, 64, 256, 8, 4
    hop, length, _ = maavss_amd.calc_hop_size(t, hpf, 30, 16000)
    stft = maavss_amd.STFT(fft, hop, noise_std=0.1, device="cuda")
    bank = ClipBank(size, t, frame_hop, hpf, hop, capacity_frames=32, capacity_samples=24000, storage="u16")
    g = torch.Generator().manual_seed(8)
    assert [bank.add_recording(torch.randn(12000, generator=g).cuda(), maps=_maps(n, 64, 40 + n).cuda()) for n in (16, 12)] == [3, 2]
    crop = BankCrop(flip=0.5)
    batches = [[4, 1], [2, 3], [0, 0]]
    want = []
    for i, indices in enumerate(batches):
        boxes, flip = crop.sample(b, size, torch.Generator().manual_seed(40 + i))
        attn, audio = bank.batch(indices, boxes=boxes, flip=flip)
        want.append((attn, *stft(audio, seed=40 + i)))
    assert not torch.equal(want[0][0], bank.batch(batches[0])[0]), "the crops changed nothing"
    pipe = maavss_amd.ClipPipeline(None, stft, t, bank=bank, bank_crop=crop)
    for i in (0, 1):                                                          # both slots in flight
        pipe.submit_clips(batches[i], seed=40 + i)
    for i in (0, 1):
        got = pipe.get()
        assert got[0].shape == (b, 1, t, size, size)
        for name, x, y in zip(("attention frames", "x_stft", "y_stft"), got, want[i]):
            assert torch.equal(x, y), f"batch {i}: {name} differ from the serial calls"
        pipe.release()
    # a slot reused after release(), the crops given by the caller: the seed still drives the STFT noise
    boxes, flip = crop.sample(b, size, torch.Generator().manual_seed(42))
    pipe.submit_clips(batches[2], 42, boxes, flip)
    assert all(torch.equal(x, y) for x, y in zip(pipe.get(), want[2]))
    pipe.release()
    pipe.drain()
