"""ClipBank (maavss_amd/clip_bank.py) on the host: the clip index against a brute-force loop, every refusal that needs no device,
and the 16-bit pack rule of tests/bank_twin.py on crafted values.  A bank on device="cpu" holds f32 maps given through maps= (a plain
copy) and answers every index question; cutting a batch from it is refused like every other op without the MI355X."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import bank_twin as tw
import maavss_amd
from maavss_amd import ClipBank, _lib
from maavss_amd.clip_bank import clip_sample_start, count_clips

T, FRAME_HOP, HPF, HOP, S = 5, 2, 8, 66, 16
N = HPF * HOP * T                     # 2640 samples per clip
FRAMES = (9, 6, 5)                    # 3, 1 and 1 clips by their frames


def _bank(capacity_frames=64, capacity_samples=40000, **kw):
    return ClipBank(S, T, FRAME_HOP, HPF, HOP, capacity_frames=capacity_frames, capacity_samples=capacity_samples, device="cpu", **kw)


def _recording(n_frames, n_samples, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n_samples, generator=g), torch.rand(n_frames, (S // 8) ** 2, generator=g)


def _ample(n_frames):
    return tw.sample_start(n_frames, FRAME_HOP, 30, 16000) + N + 7


def test_clip_count_is_limited_by_frames_or_by_samples_as_a_brute_force_loop_finds():
    for n_frames, by_frames in zip(FRAMES, (3, 1, 1)):
        want = tw.clips_brute_force(n_frames, _ample(n_frames), T, FRAME_HOP, N)
        assert len(want) == by_frames == count_clips(n_frames, _ample(n_frames), T, FRAME_HOP, N)
        # one sample short of the last clip: the samples now limit the count
        short = want[-1][1] + N - 1
        assert len(tw.clips_brute_force(n_frames, short, T, FRAME_HOP, N)) == by_frames - 1 == count_clips(n_frames, short, T, FRAME_HOP, N)
        assert count_clips(n_frames, short + 1, T, FRAME_HOP, N) == by_frames
        bank = _bank()
        audio, maps = _recording(n_frames, short)
        if by_frames == 1:
            with pytest.raises(ValueError, match="no whole clip"):
                bank.add_recording(audio, maps=maps)
            assert len(bank) == 0 and bank.recordings == []
        else:
            assert bank.add_recording(audio, maps=maps) == by_frames - 1 == len(bank)
        bank = _bank()
        audio, maps = _recording(n_frames, _ample(n_frames))
        assert bank.add_recording(audio, maps=maps) == by_frames
        assert [bank.clip_start(i) for i in range(len(bank))] == want


def test_sample_starts_at_two_rate_pairs():
    for k in range(40):
        assert clip_sample_start(k, FRAME_HOP, 30, 16000) == round(k * FRAME_HOP / 30 * 16000)
        assert clip_sample_start(k, 3, 25, 22050) == round(Fraction(k * 3 * 22050, 25)) == tw.sample_start(k, 3, 25, 22050)
    assert clip_sample_start(1, FRAME_HOP, 30, 16000) == 1067 and clip_sample_start(3, FRAME_HOP, 30, 16000) == 3200
    assert clip_sample_start(1, 1, 25, 22050) == 882 and clip_sample_start(5, 3, 25, 22050) == 13230
    # a half-way case rounds to even, as Python's round does on the exact fraction: 3 * 22050 / 20 = 3307.5
    assert clip_sample_start(1, 3, 20, 22050) == 3308 and clip_sample_start(1, 1, 20, 22050) == 1102       # 1102.5 -> 1102
    bank = ClipBank(S, T, 3, HPF, HOP, fps=25, sr=22050, capacity_frames=32, capacity_samples=60000, device="cpu")
    audio, maps = _recording(14, 50000)
    assert bank.add_recording(audio, maps=maps) == 4          # frames: 3 k + 5 <= 14
    assert [bank.clip_start(i) for i in range(4)] == [(3 * k, round(Fraction(3 * k * 22050, 25))) for k in range(4)]


def test_locate_and_clip_start_across_recordings():
    bank = _bank()
    lengths = []
    for i, n_frames in enumerate(FRAMES):
        audio, maps = _recording(n_frames, _ample(n_frames), seed=i)
        bank.add_recording(audio, maps=maps)
        lengths.append((n_frames, audio.shape[0]))
    assert len(bank) == 5
    assert [bank.locate(i) for i in range(5)] == [(0, 0), (0, 1), (0, 2), (1, 0), (2, 0)]
    # the bank keeps what a recording's clips use: 9, 5 and 5 frames; s_2 + N, N and N samples
    used = [(9, tw.sample_start(2, FRAME_HOP, 30, 16000) + N), (5, N), (5, N)]
    assert [r[2:] for r in bank.recordings] == [(f, s, c) for (f, s), c in zip(used, (3, 1, 1))]
    want, f0, s0 = [], 0, 0
    for (n_frames, n_samples), (uf, us) in zip(lengths, used):
        want += [(f0 + v, s0 + s) for v, s in tw.clips_brute_force(n_frames, n_samples, T, FRAME_HOP, N)]
        f0, s0 = f0 + uf, s0 + us
    assert [bank.clip_start(i) for i in range(5)] == want
    assert (bank.n_frames, bank.n_samples) == (f0, s0)
    frame_start, sample_start = bank.check_indices([4, 0, 2, 2, 3])
    assert frame_start.dtype == torch.int32 and sample_start.dtype == torch.int64
    assert list(zip(frame_start.tolist(), sample_start.tolist())) == [want[i] for i in (4, 0, 2, 2, 3)]
    assert torch.equal(bank.check_indices(torch.tensor([4, 0], dtype=torch.int32))[1], sample_start[:2])
    # the banked data is the recordings' prefix
    audio1, maps1 = _recording(FRAMES[1], _ample(FRAMES[1]), seed=1)
    assert torch.equal(bank.audio[used[0][1]:used[0][1] + N], audio1[:N]) and torch.equal(bank.maps[9:14], maps1[:5])


def test_refusals_need_no_device():
    with pytest.raises(ValueError, match="multiple of 4"):
        ClipBank(18, T, FRAME_HOP, HPF, HOP, capacity_frames=8, capacity_samples=8, device="cpu")
    with pytest.raises(ValueError, match="at least 8"):
        ClipBank(4, T, FRAME_HOP, HPF, HOP, capacity_frames=8, capacity_samples=8, device="cpu")
    with pytest.raises(ValueError, match="storage"):
        _bank(storage="f16")
    with pytest.raises(ValueError, match="frame_hop"):
        ClipBank(S, T, 0, HPF, HOP, capacity_frames=8, capacity_samples=8, device="cpu")
    bank = _bank(capacity_frames=15, capacity_samples=2 * N + tw.sample_start(2, FRAME_HOP, 30, 16000))
    audio, maps = _recording(9, _ample(9))
    frames = torch.zeros(9, 3, S, S)
    with pytest.raises(ValueError, match="exactly one"):
        bank.add_recording(audio)
    with pytest.raises(ValueError, match="exactly one"):
        bank.add_recording(audio, frames=frames, maps=maps, video_attention=object())
    with pytest.raises(ValueError, match="needs video_attention"):
        bank.add_recording(audio, frames=frames)
    with pytest.raises(ValueError, match=r"frames must be float32 \[N, 3, 16, 16\]"):
        bank.add_recording(audio, frames=torch.zeros(9, 3, S, S + 8), video_attention=object())
    with pytest.raises(ValueError, match="frames must be float32"):
        bank.add_recording(audio, frames=frames.double(), video_attention=object())
    with pytest.raises(ValueError, match=r"maps must be float32 \[N, 4\]"):
        bank.add_recording(audio, maps=torch.zeros(9, 5))
    with pytest.raises(ValueError, match="maps must be float32"):
        bank.add_recording(audio, maps=maps.double())
    with pytest.raises(ValueError, match="maps must be float32"):
        bank.add_recording(audio, maps=maps.view(9, 2, 2))
    with pytest.raises(ValueError, match="audio must be a 1-D float32"):
        bank.add_recording(audio[None], maps=maps)
    with pytest.raises(ValueError, match="audio must be a 1-D float32"):
        bank.add_recording(audio.double(), maps=maps)
    with pytest.raises(ValueError, match="no whole clip"):
        bank.add_recording(audio, maps=maps[:4])
    with pytest.raises(ValueError, match="no whole clip"):
        bank.add_recording(audio[:N - 1], maps=maps)
    assert len(bank) == 0
    # capacity: 15 frames and the samples of a 3-clip plus a 1-clip recording
    assert bank.add_recording(audio, maps=maps) == 3
    audio6, maps6 = _recording(6, _ample(6), seed=1)
    assert bank.add_recording(audio6, maps=maps6) == 1           # uses 5 frames
    state = (len(bank), bank.n_frames, bank.n_samples, list(bank.recordings), bank.maps.clone(), bank.audio.clone())
    with pytest.raises(ValueError, match="capacity_frames=15 exceeded"):
        bank.add_recording(audio, maps=maps[:5])                 # 14 frames banked, one clip needs 5 more
    roomy = _bank(capacity_frames=64, capacity_samples=N + 10)
    roomy.add_recording(audio, maps=maps[:5])
    with pytest.raises(ValueError, match="capacity_samples=2650 exceeded"):
        roomy.add_recording(audio, maps=maps[:5])
    assert len(roomy) == 1 and (roomy.n_frames, roomy.n_samples) == (5, N)
    assert state[:4] == (len(bank), bank.n_frames, bank.n_samples, bank.recordings)
    assert torch.equal(state[4][:14], bank.maps[:14]) and torch.equal(state[5][:bank.n_samples], bank.audio[:bank.n_samples])
    # indices
    for bad in ([4], [-1], [0, 1, 7], torch.tensor([0, 4])):
        with pytest.raises(IndexError, match=r"\[0, 4\)"):
            bank.batch(bad)
    with pytest.raises(ValueError, match="integers"):
        bank.batch([0.0])
    with pytest.raises(ValueError, match="empty"):
        bank.batch([])
    with pytest.raises(ValueError, match="integer tensor"):
        bank.batch(torch.tensor([0.0]))
    with pytest.raises(IndexError):
        bank.locate(4)
    with pytest.raises(IndexError):
        bank.clip_start(-1)
    with pytest.raises(ValueError, match=r"out\[0\] must be a contiguous float32 \[2, 1, 5, 16, 16\]"):
        bank.batch([0, 1], out=(torch.zeros(2, 1, T, S, S + 4), torch.zeros(2, N)))
    with pytest.raises(ValueError, match=r"out\[1\] must be a float32 \[2, 2640\]"):
        bank.batch([0, 1], out=(torch.zeros(2, 1, T, S, S), torch.zeros(2, N + 1)))
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        bank.batch([0, 1])                                       # valid indices: the cut itself runs on the MI355X only
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        _bank(storage="u16").add_recording(audio, maps=maps)     # so does the pack


def test_pipeline_refusals_with_a_bank():
    bank = _bank()
    audio, maps = _recording(9, _ample(9))
    bank.add_recording(audio, maps=maps)
    stft = maavss_amd.STFT(512, HOP, device="cpu")
    with pytest.raises(ValueError, match="clips of 5 frames.*clip_frames=8"):
        maavss_amd.ClipPipeline(None, stft, 8, bank=bank)
    with pytest.raises(ValueError, match="do not go with bank="):
        maavss_amd.ClipPipeline(None, stft, T, bank=bank, transform=object())
    with pytest.raises(ValueError, match="do not go with bank="):
        maavss_amd.ClipPipeline(None, stft, T, bank=bank, audio_transform=object(), audio_length=N)
    # the host-side checks of the two submit calls, on a pipeline without its side stream (the constructor opens one on the device)
    pipe = object.__new__(maavss_amd.ClipPipeline)
    pipe.bank, pipe.va = None, None
    with pytest.raises(ValueError, match="built with bank="):
        pipe.submit_clips([0], 0)
    with pytest.raises(ValueError, match="submit_clips"):
        pipe.submit(torch.zeros(T, 3, S, S), torch.zeros(1, N), 0)
    pipe.bank, pipe.mixer, pipe.head, pipe.tail, pipe.depth, pipe.slots = bank, None, 0, 0, 2, [None, None]
    with pytest.raises(IndexError, match=r"\[0, 3\)"):
        pipe.submit_clips([3], 0)
    with pytest.raises(ValueError, match="built with mixer="):
        pipe.submit_clips([0, 1], 0, snr_db=torch.zeros(2))


def test_pack_twin_on_crafted_values():
    v = np.array(tw.CRAFTED, dtype=np.float32)
    q = tw.pack(v)
    assert q.dtype == np.uint16
    assert q.tolist() == [tw.pack_exact(x) for x in tw.CRAFTED]
    for x, want in tw.CRAFTED_BY_HAND.items():
        assert q[tw.CRAFTED.index(x)] == want, x
    # the two half-way products: float32(0.5 / 65535) * 65535 and float32(1.5 / 65535) * 65535 land on or beside .5; half to even
    # gives 0 and 2 when they land on it, and the exact rule says which
    assert q[3] in (0, 1) and q[4] in (1, 2) and q[3] == tw.pack_exact(0.5 / 65535) and q[4] == tw.pack_exact(1.5 / 65535)
    assert tw.pack(np.array([np.nan, np.inf, -np.inf], dtype=np.float32)).tolist() == [0, 65535, 0]
    # unpack: the correctly rounded quotient; 65535 gives exactly 1 where a product with the rounded reciprocal need not
    u = tw.unpack(np.arange(65536, dtype=np.uint16))
    assert u.dtype == np.float32 and u[0] == 0.0 and u[65535] == 1.0
    exact = np.array([float(np.float32(float(Fraction(int(k), 65535)))) for k in (1, 2, 3, 21845, 32767, 32768, 43690, 65534)])
    assert u[[1, 2, 3, 21845, 32767, 32768, 43690, 65534]].astype(np.float64).tolist() == exact.tolist()
    by_product = np.arange(65536, dtype=np.float32) * (np.float32(1) / np.float32(65535))
    assert (by_product != u).any(), "the quotient and the reciprocal product agree everywhere: the crafted contrast shows nothing"
    # pack inverts unpack, and the round trip stays within half a step plus the float32 roundings of the product (2^-24 relative)
    # and of the quotient (2^-25)
    assert tw.pack(u).tolist() == list(range(65536))
    r = np.random.default_rng(5).random(20000, dtype=np.float32)
    err = np.abs(tw.unpack(tw.pack(r)).astype(np.float64) - r.astype(np.float64)).max()
    assert err <= 1 / 131070 + 2.0 ** -23, err
