"""ClipBank.activity and ClipSampler on the MI355X (maavss_amd/csrc/clip_select.hip) against tests/select_twin.py: the exact columns and
the reason bytes equal the twin's; energy, motion, the recording levels and the frame-pair table equal it bit for bit (the twin restates
the kernels' order), rms_db and rel_db lie within the derived bounds (select_twin's docstring) with -inf and NaN where the twin has
them; nothing is written outside the outputs, two runs and a bank of one recording alone give the same bytes, nothing
synchronises but the sampler's one copy, and a bank-fed ClipPipeline driven by the sampler sees the accepted clips and no other."""
import warnings

import numpy as np
import pytest
import torch

import select_twin as tw
import maavss_amd
from maavss_amd import ClipBank, ClipSampler, _lib
from maavss_amd._lib import call, ptr, stream_ptr

pytestmark = pytest.mark.gpu

F64 = ("energy", "rms_db", "rel_db", "motion_mean", "motion_peak")
EXACT = ("peak", "n_bad", "n_active", "recording")


def _bank(case, only=None, room=0):
    size, storage, T, fh, hop, hpf, (fps, sr), _ = case
    recs = tw.build(case)["recordings"]
    recs = recs if only is None else [recs[only]]
    bank = ClipBank(size, T, fh, hpf, hop, fps=fps, sr=sr, capacity_frames=sum(m.shape[0] for _, m in recs) + room,
                    capacity_samples=sum(len(a) for a, _ in recs) + room * 4096, storage=storage)
    for audio, maps in recs:
        bank.add_recording(torch.from_numpy(audio).cuda(), maps=torch.from_numpy(maps).cuda())
    return bank


def _bytes(t):
    return t.cpu().numpy().tobytes()


BITS = ("energy", "motion_mean", "motion_peak")          # the twin's order is the kernels': equal bit for bit
BOUND = ("rms_db", "rel_db")                              # through log10: within the derived bounds


def _check_against_twin(act, b, rows=slice(None)):
    t, bd = b["table"], tw.bounds(b)
    for k in EXACT:
        got = act[k].cpu().numpy()
        assert got.dtype == t[k].dtype and np.array_equal(got, t[k][rows]), k
    for k in BITS:
        got = act[k].cpu().numpy()
        assert got.dtype == np.float64 and tw.same_bits(got, t[k][rows]), (k, got, t[k][rows])
    for k in BOUND:
        got = act[k].cpu().numpy()
        assert got.dtype == np.float64 and tw.close(got, t[k][rows], bd[k][rows]), (k, got, t[k][rows])


@pytest.mark.parametrize("case", tw.CASES, ids=tw.case_id)
def test_activity_and_reasons_are_the_twins(case):
    b = tw.build(case)
    bank = _bank(case)
    assert [bank.clip_start(i) for i in range(len(bank))] == [(v, s) for v, s, _ in b["where"]], "the twin's index is the bank's"
    act = bank.activity()
    assert set(act) == set(F64 + EXACT) and all(v.is_cuda and v.shape == (len(bank),) for v in act.values())
    assert act["peak"].dtype == torch.float32 and all(act[k].dtype == torch.int32 for k in EXACT[1:])
    _check_against_twin(act, b)
    assert bank.activity() is act, "cached until the next add_recording"
    # two runs: identical bytes
    bank._activity = None
    again = bank.activity()
    assert again is not act and all(_bytes(again[k]) == _bytes(act[k]) for k in act)
    # the reasons, and through them accepted / rejected
    counts = {name: int(((b["reasons"] >> k) & 1).sum()) for k, name in enumerate(tw.REASONS)}
    if (b["reasons"] == 0).any():
        s = ClipSampler(bank, 1, drop_last=False, **tw.THRESHOLDS)
        assert np.array_equal(s.reasons.numpy(), b["reasons"])
        assert s.accepted.tolist() == np.flatnonzero(b["reasons"] == 0).tolist() and s.rejected == counts
    else:                                                       # clips of one frame have no motion: min_motion leaves nothing
        with pytest.raises(ValueError, match=f"no clip is accepted: {len(bank)} clips considered.*'static': {counts['static']}"):
            ClipSampler(bank, 1, drop_last=False, **tw.THRESHOLDS)
        rest = b["reasons"] & ~np.uint8(8)
        if (rest == 0).any():
            s = ClipSampler(bank, 1, drop_last=False, **dict(tw.THRESHOLDS, min_motion=None))
            assert np.array_equal(s.reasons.numpy(), rest) and s.accepted.tolist() == np.flatnonzero(rest == 0).tolist()
    # the bytes the kernel writes, whatever the sampler makes of them
    dev = torch.full((len(bank) + 2,), 0xA5, device="cuda", dtype=torch.uint8)
    th = tw.THRESHOLDS
    call("maavss_bank_clip_select", *(ptr(act[k]) for k in ("rms_db", "rel_db", "n_active", "motion_mean", "motion_peak", "peak", "n_bad")), len(bank),
         127, th["min_rms_db"], th["min_rel_db"], th["min_active_fraction"] * b["J"], th["min_motion"], th["max_motion_peak"], th["max_peak"],
         ptr(dev[1:]), stream_ptr())
    assert dev[1:-1].cpu().numpy().tolist() == b["reasons"].tolist() and dev[0].item() == dev[-1].item() == 0xA5
    # a recording banked alone: the rows it has in the full table, byte for byte
    for r in range(len(b["recordings"])):
        alone = _bank(case, only=r).activity()
        rows = np.flatnonzero(b["table"]["recording"] == r)
        for k in F64 + EXACT[:-1]:
            assert _bytes(alone[k]) == _bytes(act[k][rows[0]:rows[-1] + 1]), (r, k)
        assert not alone["recording"].any()


def _raw(bank, pad=3, fill=-7.0):
    """activity()'s launches into buffers with `pad` sentinels on either side of every output -> the padded buffers."""
    c, r = len(bank), len(bank.recordings)
    frame_start, sample_start = bank.check_indices(torch.arange(c))
    rec = bank.clip_recordings()
    chunks = [_lib.query("maavss_bank_level_chunks", q[3]) for q in bank.recordings]
    first = [sum(chunks[:i]) for i in range(r)]
    rec_tab = torch.tensor([[q[1] for q in bank.recordings], [q[3] for q in bank.recordings], first], dtype=torch.int64)
    d_tab, d_sample, d_frame, d_rec = rec_tab.cuda(), sample_start.cuda(), frame_start.cuda(), rec.cuda()

    def padded(n, dtype):
        return torch.full((n + 2 * pad,), fill, device="cuda", dtype=dtype)

    buf = {k: padded(c, torch.float64) for k in F64}
    buf.update(peak=padded(c, torch.float32), n_bad=padded(c, torch.int32), n_active=padded(c, torch.int32), partials=padded(sum(chunks), torch.float64),
               level=padded(r, torch.float64), D=padded(bank.n_frames - 1, torch.float64), reasons=torch.full((c + 2 * pad,), 0xA5, device="cuda", dtype=torch.uint8))
    p = {k: ptr(v[pad:]) for k, v in buf.items()}
    st = stream_ptr()
    call("maavss_bank_recording_level", ptr(bank.audio), bank.n_samples, ptr(d_tab), ptr(rec_tab), r, p["partials"], sum(chunks), p["level"], st)
    call("maavss_bank_frame_motion", ptr(bank.maps), 0 if bank.storage == "f32" else 1, bank.n_frames, bank.frame_elems, p["D"], st)
    # clips of one frame read no pair: D may be null there, as activity() passes it
    call("maavss_bank_clip_activity", ptr(bank.audio), bank.n_samples, p["D"] if bank.clip_frames > 1 else None, bank.n_frames, p["level"], ptr(d_tab), r, ptr(d_sample), ptr(d_frame),
         ptr(d_rec), ptr(sample_start), ptr(frame_start), ptr(rec), c, bank.clip_frames, bank.hops_per_frame, bank.hop, 10.0 ** (-tw.RANGE_DB / 10.0),
         p["energy"], p["rms_db"], p["rel_db"], p["motion_mean"], p["motion_peak"], p["peak"], p["n_bad"], p["n_active"], st)
    th = tw.THRESHOLDS
    call("maavss_bank_clip_select", p["rms_db"], p["rel_db"], p["n_active"], p["motion_mean"], p["motion_peak"], p["peak"], p["n_bad"], c, 127,
         th["min_rms_db"], th["min_rel_db"], th["min_active_fraction"] * bank.hops_per_frame * bank.clip_frames, th["min_motion"], th["max_motion_peak"],
         th["max_peak"], p["reasons"], st)
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("case", tw.CASES, ids=tw.case_id)
def test_sentinels_around_every_output_are_untouched(case):
    b, bank, pad = tw.build(case), _bank(case), 3
    buf = _raw(bank, pad)
    for k, v in buf.items():
        want = 0xA5 if k == "reasons" else -7
        assert bool((v[:pad] == want).all()) and bool((v[-pad:] == want).all()), f"{k}: written outside its {v.numel() - 2 * pad} values"
    act = {k: buf[k][pad:-pad] for k in F64 + EXACT[:-1]}
    act["recording"] = bank.clip_recordings().cuda()
    _check_against_twin(act, b)
    assert np.array_equal(buf["reasons"][pad:-pad].cpu().numpy(), b["reasons"])
    assert tw.same_bits(buf["level"][pad:-pad].cpu().numpy(), np.array(b["levels"])), "the recording levels are not the twin's bits"
    assert tw.same_bits(buf["D"][pad:-pad].cpu().numpy(), b["D"]), "the frame-pair table is not the twin's bits"
    # the bank's own path gives the same bytes as the raw calls
    own = bank.activity()
    assert all(_bytes(own[k]) == _bytes(act[k]) for k in F64 + EXACT[:-1])


def test_recordings_of_several_chunks_have_the_twins_level():
    """The shared cases' recordings fit one chunk of 16384 samples.  Here one of two chunks and a tail next to a short one, with an inf
    and a NaN the level has to pass over: the partials added in index order, bit for bit, and the clips' rows with them."""
    T, fh, hop = 2, 2, 100
    n = T * hop
    rng = np.random.default_rng(5)
    waves, maps = [], []
    for clips in (38, 2):
        used = tw.sample_start(clips - 1, fh, 30, 16000) + n
        audio = (0.2 * rng.standard_normal(used)).astype(np.float32)
        audio[tw.sample_start(clips // 2, fh, 30, 16000) + 5], audio[tw.sample_start(clips - 1, fh, 30, 16000) + 7] = np.inf, np.nan      # inside clips
        waves.append(audio)
        maps.append(rng.random(((clips - 1) * fh + T, 1)).astype(np.float32))
    bank = ClipBank(8, T, fh, 1, hop, capacity_frames=sum(len(m) for m in maps), capacity_samples=sum(len(a) for a in waves))
    assert [bank.add_recording(torch.from_numpy(a).cuda(), maps=torch.from_numpy(m).cuda()) for a, m in zip(waves, maps)] == [38, 2]
    assert [q[3] for q in bank.recordings] == [len(a) for a in waves] and len(waves[0]) > 2 * 16384
    assert [_lib.query("maavss_bank_level_chunks", len(a)) for a in waves] == [3, 1]
    buf = _raw(bank)
    assert buf["partials"].numel() == 4 + 6 and bool((buf["partials"][:3] == -7).all()) and bool((buf["partials"][-3:] == -7).all())
    levels = [tw.recording_level(a) for a in waves]
    assert np.isfinite(levels).all() and tw.same_bits(buf["level"][3:-3].cpu().numpy(), np.array(levels))
    audio, D = np.concatenate(waves), tw.frame_motion(np.concatenate(maps))
    rows = []
    for i in range(len(bank)):
        v, s = bank.clip_start(i)
        r = bank.locate(i)[0]
        rows.append(tw.clip_row(audio, s, D, v, T, 1 * T, hop, levels[r], len(waves[r]))[0])      # J = hops_per_frame * T
    for k in BITS:
        assert tw.same_bits(buf[k][3:-3].cpu().numpy(), np.array([row[k] for row in rows])), k
    for k in ("n_bad", "n_active"):
        assert buf[k][3:-3].cpu().numpy().tolist() == [row[k] for row in rows], k
    assert sum(row["n_bad"] for row in rows) == 4


def test_activity_does_not_synchronise_and_the_sampler_copies_once():
    case = tw.CASES[3]
    bank = _bank(case)
    first = bank.activity()                                  # loads the library, warms the allocators
    ClipSampler(bank, 2, **tw.THRESHOLDS)
    bank._activity = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                  # any blocking call of torch's raises
    try:
        second = bank.activity()
        other = bank.activity(range_db=20.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(_bytes(first[k]) == _bytes(second[k]) for k in first)
    assert other is not second and _bytes(other["energy"]) == _bytes(second["energy"])
    assert bool((other["n_active"] <= second["n_active"]).all()), "a narrower range keeps fewer segments"
    bank._activity = None
    bank.activity()
    bank.batch([0, 1])                                       # warms the pinned staging
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            s = ClipSampler(bank, 2, **tw.THRESHOLDS)
        torch.cuda.set_sync_debug_mode("error")
        batches = [bank.batch(idx) for e in (0, 1) for idx in s.epoch(e)]          # epochs and batches: no synchronisation at all
        free = ClipSampler(bank, 2, reject_nonfinite=False)                           # no threshold: no statistic, no copy
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in seen if "synchroniz" in str(w.message)]
    assert len(syncs) == 1, [str(w.message) for w in seen]
    assert len(batches) == 2 * len(s) and free.accepted.tolist() == list(range(len(bank)))


def test_the_samplers_range_db_is_the_tables():
    """range_db= goes to bank.activity(): two samplers with different ranges threshold n_active against different tables, and say so."""
    case = tw.CASES[3]
    bank = _bank(case)
    kw = dict(min_active_fraction=0.9, reject_nonfinite=False, drop_last=False)
    wide = ClipSampler(bank, 1, **kw)
    assert bank._activity[0] == 40.0
    wide_table = {k: v.cpu() for k, v in bank.activity().items()}
    narrow = ClipSampler(bank, 1, range_db=3.0, **kw)
    assert bank._activity[0] == 3.0
    narrow_table = {k: v.cpu() for k, v in bank.activity(range_db=3.0).items()}
    j = bank.hops_per_frame * bank.clip_frames
    for s, table in ((wide, wide_table), (narrow, narrow_table)):
        assert torch.equal(s.reasons, ClipSampler(dict(table, segments=j), 1, **kw).reasons)
    assert bool((narrow_table["n_active"] <= wide_table["n_active"]).all()) and not torch.equal(narrow_table["n_active"], wide_table["n_active"])
    assert narrow.rejected["few_active_segments"] > wide.rejected["few_active_segments"]
    with pytest.raises(ValueError, match="range_db"):
        ClipSampler(bank, 1, range_db=-1.0, **kw)


def test_another_recording_invalidates_the_cache():
    case = tw.CASES[4]
    b = tw.build(case)
    bank = _bank(case, room=64)
    act = bank.activity()
    audio, maps = b["recordings"][2]
    added = bank.add_recording(torch.from_numpy(audio).cuda(), maps=torch.from_numpy(maps).cuda())
    more = bank.activity()
    assert more is not act and more["energy"].numel() == len(bank) == act["energy"].numel() + added
    for k in F64 + EXACT[:-1]:
        assert _bytes(more[k][:len(bank) - added]) == _bytes(act[k]), k
        rows = np.flatnonzero(b["table"]["recording"] == 2)
        assert _bytes(more[k][-added:]) == _bytes(act[k][rows[0]:rows[-1] + 1]), f"{k}: the same recording banked again has the same rows"
    assert more["recording"][-added:].tolist() == [len(b["recordings"])] * added
    s = ClipSampler(bank, 1, recordings=[len(b["recordings"])], **tw.THRESHOLDS)
    assert s.n_considered == added and s.accepted.min().item() >= len(bank) - added


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """With real device buffers behind every pointer: null pointers, a J beyond the kernel's limit, negative counts, an unknown storage
    code and a host table entry outside the bank are refused with a message (tests/test_clip_select_cpu.py holds the full list), and the
    outputs keep their sentinels -- nothing was launched."""
    case = tw.CASES[2]
    bank = _bank(case)
    c, r = len(bank), len(bank.recordings)
    frame_start, sample_start = bank.check_indices(torch.arange(c))
    rec = bank.clip_recordings()
    chunks = [_lib.query("maavss_bank_level_chunks", q[3]) for q in bank.recordings]
    rec_tab = torch.tensor([[q[1] for q in bank.recordings], [q[3] for q in bank.recordings], [sum(chunks[:i]) for i in range(r)]], dtype=torch.int64)
    d_tab, d_sample, d_frame, d_rec = rec_tab.cuda(), sample_start.cuda(), frame_start.cuda(), rec.cuda()
    out = torch.full((8, c), -7.0, device="cuda", dtype=torch.float64)
    small = torch.full((3, c), -7, device="cuda", dtype=torch.int32)
    work = torch.full((sum(chunks) + r + bank.n_frames,), -7.0, device="cuda", dtype=torch.float64)
    partials, level, D = work[:sum(chunks)], work[sum(chunks):sum(chunks) + r], work[sum(chunks) + r:]
    st = stream_ptr()

    def level_call(audio=ptr(bank.audio), host=ptr(rec_tab), n_rec=r, room=sum(chunks)):
        call("maavss_bank_recording_level", audio, bank.n_samples, ptr(d_tab), host, n_rec, ptr(partials), room, ptr(level), st)

    def motion_call(maps=ptr(bank.maps), storage=0, n_frames=bank.n_frames):
        call("maavss_bank_frame_motion", maps, storage, n_frames, bank.frame_elems, ptr(D), st)

    def clips_call(hpf=bank.hops_per_frame, n_clips=c, energy=ptr(out[0]), host_sample=ptr(sample_start)):
        call("maavss_bank_clip_activity", ptr(bank.audio), bank.n_samples, ptr(D), bank.n_frames, ptr(level), ptr(d_tab), r, ptr(d_sample), ptr(d_frame),
             ptr(d_rec), host_sample, ptr(frame_start), ptr(rec), n_clips, bank.clip_frames, hpf, bank.hop, 1e-4, energy, *(ptr(out[k]) for k in range(1, 5)),
             ptr(small[0].view(torch.float32)), ptr(small[1]), ptr(small[2]), st)

    def select_call(n_clips=c, reasons=ptr(small[0]), first=ptr(out[1])):
        call("maavss_bank_clip_select", first, ptr(out[2]), ptr(small[2]), ptr(out[3]), ptr(out[4]), ptr(small[0].view(torch.float32)), ptr(small[1]), n_clips,
             127, -50.0, -20.0, 4.0, 1e-3, 0.3, 1.0, reasons, st)

    outside = sample_start.clone()
    outside[-1] = bank.n_samples
    for fn, kw, match in ((level_call, dict(audio=None), "null pointer"), (level_call, dict(host=None), "null pointer"), (level_call, dict(n_rec=-1), "must be positive"),
                          (level_call, dict(room=1), "chunk partials needed, room for 1"),
                          (motion_call, dict(maps=None), "null pointer"), (motion_call, dict(storage=2), "storage must be 0"), (motion_call, dict(n_frames=-5), "hold no pair"),
                          (clips_call, dict(energy=None), "null output pointer"), (clips_call, dict(host_sample=None), "null pointer"),
                          (clips_call, dict(hpf=2000), "segments, the kernel holds 2048"), (clips_call, dict(n_clips=-3), "must be positive"),
                          (clips_call, dict(host_sample=ptr(outside)), f"clip {c - 1} .* lies outside the bank"),
                          (select_call, dict(reasons=None), "null pointer"), (select_call, dict(first=None), "null pointer"), (select_call, dict(n_clips=-1), "n_clips = -1")):
        with pytest.raises(_lib.MaavssError, match=match):
            fn(**kw)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((small == -7).all()) and bool((work == -7.0).all()), "a refused call launched something"
    long_bank = ClipBank(8, 300, 300, 8, 1, capacity_frames=300, capacity_samples=2400)          # J = 2400 segments a clip
    long_bank.add_recording(torch.zeros(2400).cuda(), maps=torch.zeros(300, 1).cuda())
    with pytest.raises(ValueError, match="2400 segments per clip, the activity kernel holds 2048"):
        long_bank.activity()
    with pytest.raises(ValueError, match="range_db"):
        bank.activity(range_db=-1.0)


def test_a_sampler_fed_pipeline_sees_every_accepted_clip_once_an_epoch():
    t, size, fft, hpf, frame_hop, per_rec = 3, 16, 256, 8, 1, 14
    hop, length, _ = maavss_amd.calc_hop_size(t, hpf, 30, 16000)
    stft = maavss_amd.STFT(fft, hop, noise_std=0.1, device="cuda")
    n_f = (per_rec - 1) * frame_hop + t
    n_s = tw.sample_start(per_rec - 1, frame_hop, 30, 16000) + length
    bank = ClipBank(size, t, frame_hop, hpf, hop, capacity_frames=3 * n_f, capacity_samples=3 * n_s)
    g = torch.Generator().manual_seed(77)
    for r in range(3):
        audio = 0.1 * torch.randn(n_s, generator=g)
        maps = 0.3 + 0.05 * torch.rand(n_f, 4, generator=g)
        if r == 1:
            audio[n_s // 3:] = 0.0                              # the later clips are silent
        if r == 2:
            maps[6:] = maps[6]                                  # the later clips are frozen
        assert bank.add_recording(audio.cuda(), maps=maps.cuda()) == per_rec
    assert len(bank) == 42
    s = ClipSampler(bank, 4, min_rms_db=-50.0, min_motion=1e-3, seed=3)
    table = {k: v.cpu().numpy() for k, v in bank.activity().items()}
    want = tw.select(table, hpf * t, dict(min_rms_db=-50.0, min_motion=1e-3))
    assert np.array_equal(s.reasons.numpy(), want) and s.rejected["too_quiet"] >= 5 and s.rejected["static"] >= 5
    accepted = set(s.accepted.tolist())
    assert 8 <= len(accepted) < 42 and accepted == set(np.flatnonzero(want == 0).tolist())
    pipe = maavss_amd.ClipPipeline(None, stft, t, bank=bank)
    orders = []
    for e in (0, 1):
        seen = []
        for i, indices in enumerate(s.epoch(e)):
            pipe.submit_clips(indices, seed=10 * e + i)
            attn, x_stft, y_stft = pipe.get()
            want_attn, want_audio = bank.batch(indices)
            assert torch.equal(attn, want_attn), f"epoch {e}, batch {i}: the pipeline's clips are not bank.batch({indices.tolist()})"
            want_x, want_y = stft(want_audio, seed=10 * e + i)
            assert torch.equal(x_stft, want_x) and torch.equal(y_stft, want_y)
            pipe.release()
            seen += indices.tolist()
        assert len(seen) == len(s) * 4 and len(set(seen)) == len(seen) and set(seen) <= accepted, f"epoch {e}"
        assert len(accepted) - len(seen) < 4, "only the dropped tail is missing"
        orders.append(seen)
    pipe.drain()
    assert orders[0] != orders[1]
