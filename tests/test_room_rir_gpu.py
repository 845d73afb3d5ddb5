"""maavss_amd.Reverb.make_room_rirs on the GPU against its float64 twin (tests/room_twin.py): every tap of every case must have the
twin's bits (the taps are integer sums, so there is no order to allow for; a difference would be an f64 operation the device rounds
otherwise).  The table then feeds the convolution unchanged.  Every library call runs under torch's sync debug mode "error"."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import reverb_twin as cw
import room_twin as tw
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


def _args(rooms):
    """rooms of room_twin.CASES -> dims [n, 3], mic [n, 3], sources [n, S, 3], beta [n, 6] as nested lists."""
    return [r[0] for r in rooms], [r[1] for r in rooms], [r[2] for r in rooms], [r[3] for r in rooms]


@functools.lru_cache(maxsize=None)
def _want(name):
    """The twin's table of a case, computed once and left unchanged."""
    _, k, h, r, sr, rooms = next(c for c in tw.CASES if c[0] == name)
    want = tw.table_of(rooms, k, sr, h, r, table=Reverb.kernel_table(h, r).numpy())
    want.setflags(write=False)
    return want


def _same(got, want):
    got = np.ascontiguousarray(got.cpu().numpy())
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, f"{bad.size} of {got.size} taps differ from the twin, first at {bad[0]}: {got.ravel()[bad[0]]!r} != {want.ravel()[bad[0]]!r}"


@pytest.mark.parametrize("name", [c[0] for c in tw.CASES])
def test_every_tap_is_the_twin_bit_for_bit(name):
    _, k, h, r, sr, rooms = next(c for c in tw.CASES if c[0] == name)
    dims, mic, sources, beta = _args(rooms)
    rv = Reverb(k, sr=sr)
    with nosync():
        got = rv.make_room_rirs(dims, mic, sources, beta=beta, half_width=h, resolution=r)
        again = Reverb(k, sr=sr).make_room_rirs(dims, mic, sources, beta=beta, half_width=h, resolution=r)
    assert got is rv.rirs and rv.sources_per_room == len(sources[0]) and tuple(got.shape) == (len(rooms) * len(sources[0]), k)
    _same(got, _want(name))
    assert torch.equal(got, again), "two runs give identical bytes"


def test_a_row_of_a_table_is_the_room_made_alone():
    _, k, h, r, sr, rooms = next(c for c in tw.CASES if c[0] == "two_sizes")
    dims, mic, sources, beta = _args(rooms)
    rv = Reverb(k, sr=sr)
    with nosync():
        table = rv.make_room_rirs(dims, mic, sources, beta=beta).clone()
        alone = [rv.make_room_rirs(dims[i:i + 1], mic[i:i + 1], sources[i:i + 1], beta=beta[i:i + 1]).clone() for i in range(3)]
    assert all(torch.equal(alone[i][0], table[i]) for i in range(3))
    # a room with five sources: each row is the room with that source alone
    _, k, h, r, sr, rooms = next(c for c in tw.CASES if c[0] == "s5")
    dims, mic, sources, beta = _args(rooms)
    rv = Reverb(k, sr=sr)
    with nosync():
        table = rv.make_room_rirs(dims, mic, sources, beta=beta).clone()
        alone = [rv.make_room_rirs(dims, mic, [[s]], beta=beta).clone() for s in sources[0]]
    assert all(torch.equal(alone[j][0], table[j]) for j in range(5))


def test_rirs_is_written_where_it_should_be_and_nowhere_else():
    name = "k4097"                                            # two tiles: the second one holds a single tap
    _, k, h, r, sr, rooms = next(c for c in tw.CASES if c[0] == name)
    rooms = rooms * 2
    rv = Reverb(k, sr=sr)
    geom, bounds, table, _ = rv.check_rooms(*_args(rooms)[:3], beta=_args(rooms)[3], half_width=h, resolution=r)
    ld, sentinel = k + 5, float(np.float32(-1234.5))
    room = torch.full((7 + 2 * ld + 7,), sentinel, device="cuda")
    out = room.as_strided((2, k), (ld, 1), 7)
    with nosync():
        rv._fill_rooms(geom, bounds, table, h, r, 343.0, out)
    _same(out, np.concatenate([_want(name), _want(name)]))
    mask = torch.ones_like(room, dtype=torch.bool)
    mask.as_strided((2, k), (ld, 1), 7).fill_(False)
    assert bool((room[mask] == sentinel).all()), "the ld_rir padding and the floats around rirs are untouched"
    # the entry point's own refusals, on the host copy of the geometry, leave it so
    broken = geom.clone()
    broken[1, 6] = broken[1, 0]                               # the second row's source on the wall x1
    with pytest.raises(maavss_amd._lib.MaavssError, match="strictly inside"):
        rv._fill_rooms(broken, bounds, table, h, r, 343.0, out)
    huge = bounds.clone()
    huge[0] = 700
    with pytest.raises(maavss_amd._lib.MaavssError, match="more than 2\\^31 images"):
        rv._fill_rooms(geom, huge, table, h, r, 343.0, out)
    assert bool((room[mask] == sentinel).all())


# ---- the table feeds the convolution unchanged -----------------------------------------------------------------------------------------
S, T, FRAME_HOP, HPF, HOP = 16, 5, 2, 8, 66                  # tests/test_reverb_gpu.py's bank: clips of 2640 samples


def _bank(seed=4):
    g = torch.Generator().manual_seed(seed)
    bank = ClipBank(S, T, FRAME_HOP, HPF, HOP, capacity_frames=32, capacity_samples=12000)
    for frames, samples in ((9, 6000), (7, 5000)):
        bank.add_recording((torch.rand(samples, generator=g) - 0.5).cuda(), maps=torch.rand(frames, 4, generator=g).cuda())
    return bank


def test_the_new_table_feeds_the_convolution_unchanged():
    name = "s5"
    _, k, h, r, sr, rooms = next(c for c in tw.CASES if c[0] == name)
    dims, mic, sources, beta = _args(rooms)
    taps = _want(name)
    rv = Reverb(k, sr=sr)
    rng = np.random.default_rng(11)
    lead, length, b = 1000, 1500, 4
    src = rng.standard_normal(lead + b * length).astype(np.float32)
    index = torch.tensor([4, 0, 2, 2], dtype=torch.int32)
    audio = torch.from_numpy(src).cuda().as_strided((b, length), (length, 1), lead)
    bank = _bank()
    indices, bank_index = [3, 4, 1, 0], torch.tensor([1, 3, 0, 4], dtype=torch.int32)
    with nosync():
        rv.make_room_rirs(dims, mic, sources, beta=beta)
        wet = rv(audio, index, lead=lead)
        clips = rv.bank_clips(bank, indices, bank_index)
        _, dry = bank.batch(indices)
    start = [lead + i * length for i in range(b)]
    _same(wet, cw.reverb(src, start, [s - lead for s in start], length, taps, index.numpy()))
    bank_src = bank.audio[:bank.n_samples].cpu().numpy()
    bank_start = [bank.clip_start(i)[1] for i in indices]
    bank_floor = maavss_amd.reverb.bank_floor(bank, indices).tolist()
    _same(clips, cw.reverb(bank_src, bank_start, bank_floor, bank.clip_samples, taps, bank_index.numpy()))
    # an anechoic room: [1, 0, ...], and the clips are bank.batch's bytes (no sample of this bank is a negative zero)
    with nosync():
        dead = rv.make_room_rirs(dims, mic, sources, beta=[[0.0] * 6])
        same = rv.bank_clips(bank, indices, bank_index)
    want = np.zeros((5, k), dtype=np.float32)
    want[:, 0] = 1.0
    _same(dead, want)
    assert same.cpu().numpy().tobytes() == dry.cpu().numpy().tobytes()


def test_same_room_groups_reach_the_pipeline():
    """sample_room_index' rows through rir_index=: a target and the partner inside its group are heard in one room."""
    bank = _bank()
    stft = maavss_amd.STFT(256, HOP, noise_std=0.1, device="cuda")
    rv = Reverb(300)
    g = torch.Generator().manual_seed(5)
    dims, mic, sources, rt60 = rv.sample_rooms(3, g, sources=2)
    rv.make_room_rirs(dims, mic, sources, rt60=rt60)
    index = rv.sample_room_index(4, g, group=2)
    assert (index[0::2] // 2 == index[1::2] // 2).all() and (index[0::2] != index[1::2]).all()
    partners = torch.tensor([[1], [0], [3], [2]], dtype=torch.int32)
    mixer = maavss_amd.Mixer(stft, interferers=1)
    pipe = maavss_amd.ClipPipeline(None, stft, T, bank=bank, mixer=mixer, reverb=rv)
    snr = torch.zeros(4)
    pipe.submit_clips([0, 1, 2, 3], seed=7, partners=partners, snr_db=snr, rir_index=index)
    got = pipe.get()
    with nosync():
        want = mixer(rv.bank_clips(bank, [0, 1, 2, 3], index), partners, snr, seed=7)
    assert torch.equal(got[1], want[0]) and torch.equal(got[2], want[1])
    pipe.release()
    pipe.drain()
