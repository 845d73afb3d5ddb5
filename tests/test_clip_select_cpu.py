"""CPU-only: the twin of the clip activity statistics (tests/select_twin.py) against an independent formulation, the margin condition
that makes the device's decisions the twin's, maavss_amd.ClipSampler's host logic on a precomputed activity table, and the argument
checks of the new entry points (which refuse before they touch the device)."""
import numpy as np
import pytest
import torch

import select_twin as tw
from maavss_amd import ClipSampler, _lib
from maavss_amd.sampler import REASONS


@pytest.mark.parametrize("case", tw.CASES, ids=tw.case_id)
def test_twin_agrees_with_an_independent_formulation(case):
    b = tw.build(case)
    t, bd = b["table"], tw.bounds(b)
    n, T = b["n"], b["T"]
    maps64 = b["bank_maps"].astype(np.float64)
    D = np.abs(np.diff(maps64, axis=0)).mean(1)
    energy, mean_motion, peak_motion = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for v, s, r in b["where"]:
            energy.append(np.sum(b["bank_audio"][s:s + n].astype(np.float64) ** 2))
            mean_motion.append(D[v:v + T - 1].mean() if T > 1 else 0.0)
            peak_motion.append(D[v:v + T - 1].max() if T > 1 else 0.0)
    energy = np.array(energy)
    assert tw.close(energy, t["energy"], bd["energy"])
    assert tw.close(mean_motion, t["motion_mean"], bd["motion_mean"])
    assert tw.close(peak_motion, t["motion_peak"], bd["motion_peak"])
    with np.errstate(divide="ignore", invalid="ignore"):
        assert tw.close(10 * np.log10(energy / n), t["rms_db"], bd["rms_db"])
        N = np.array([b["tab"][r][3] for _, _, r in b["where"]], dtype=np.float64)
        lev = []
        for _, rs, _, L, _, _ in b["tab"]:
            x = b["bank_audio"][rs:rs + L].astype(np.float64)
            lev.append(np.sum(np.where(np.isfinite(x), x, 0.0) ** 2))
        lev = np.array(lev)[t["recording"]]
        assert tw.close(10 * np.log10((energy / n) / (lev / N)), t["rel_db"], bd["rel_db"])
    # what the data was built to show
    silent = t["recording"] == 1
    assert np.all(t["energy"][silent] == 0) and np.all(t["peak"][silent] == 0) and np.all(np.isneginf(t["rms_db"][silent]))
    assert np.all(np.isnan(t["rel_db"][silent])) and np.all(t["motion_mean"][silent] == 0) and np.all(t["motion_peak"][silent] == 0)
    assert t["energy"][1] == 0 and t["recording"][1] == 0, "clip 1 of recording 0 is the silent stretch"
    assert t["n_bad"].sum() >= 2 and np.isnan(t["energy"][3]) and t["peak"][0] == 1.0
    if T > 1:
        assert t["motion_peak"][0] > 0.3 > t["motion_peak"][t["recording"] == 1].max()
    reasons = b["reasons"]
    assert reasons[0] & 32 and reasons[3] & 64 and np.all(reasons[silent] & 1) and (T == 1 or reasons[0] & 16)
    assert np.all(reasons[silent] & 8), "frozen frames (and clips of one frame) have no motion"


def test_the_inputs_keep_their_margin_from_every_threshold():
    for case in tw.CASES:
        assert tw.margin_violations(tw.build(case)) == [], tw.case_id(case)


def test_clip_starts_fall_on_every_alignment():
    starts = {s % 4 for case in tw.CASES for _, s, _ in tw.build(case)["where"]}
    assert starts == {0, 1, 2, 3}
    assert {tw.build(case)["J"] for case in tw.CASES} >= {1, 40}


# ---- ClipSampler on a precomputed table ----------------------------------------------------------------------------------------------
def _table(n=57, seed=3):
    """A made-up activity table of n clips in 4 recordings: every 5th clip too quiet, every 7th static, clip 11 non-finite."""
    g = np.random.default_rng(seed)
    rms = -20.0 - 10.0 * g.random(n)
    rms[::5] = -80.0
    motion = 0.01 + 0.01 * g.random(n)
    motion[::7] = 0.0
    n_bad = np.zeros(n, dtype=np.int32)
    n_bad[11] = 2
    act = dict(rms_db=rms, rel_db=rms + 25.0, motion_mean=motion, motion_peak=motion * 2, peak=np.full(n, 0.5, dtype=np.float32), n_bad=n_bad,
               n_active=np.full(n, 8, dtype=np.int32), recording=(np.arange(n) * 4 // n).astype(np.int32))
    return {k: torch.from_numpy(v) for k, v in act.items()}


def _rejected_set(n=57):
    return {i for i in range(n) if i % 5 == 0 or i % 7 == 0 or i == 11}


def test_selection_on_a_table_is_the_twins_rule():
    act = _table()
    s = ClipSampler(act, 4, min_rms_db=-50.0, min_motion=1e-3)
    want = sorted(set(range(57)) - _rejected_set())
    assert s.accepted.dtype == torch.int64 and s.accepted.tolist() == want
    table = {k: v.numpy() for k, v in act.items()}
    ref = tw.select(table, 8, dict(min_rms_db=-50.0, min_motion=1e-3))
    assert np.array_equal(s.reasons.numpy(), ref)
    assert s.rejected == {name: int(((ref >> k) & 1).sum()) for k, name in enumerate(REASONS)}
    assert s.rejected["too_quiet"] == 12 and s.rejected["static"] == 9 and s.rejected["nonfinite"] == 1 and s.rejected["clipped"] == 0
    everything = ClipSampler(dict(act, segments=8), 4, **tw.THRESHOLDS)
    assert np.array_equal(everything.reasons.numpy(), tw.select(table, 8))
    # no threshold, no statistic: the recording column alone
    free = ClipSampler({"recording": act["recording"]}, 4, reject_nonfinite=False)
    assert free.accepted.tolist() == list(range(57)) and not any(free.rejected.values())


def test_epochs_are_seeded_permutations_of_the_accepted_clips():
    s = ClipSampler(_table(), 4, min_rms_db=-50.0, min_motion=1e-3, seed=5)
    accepted = s.accepted.tolist()
    assert len(s) == len(accepted) // 4
    e0 = [b.tolist() for b in s.epoch(0)]
    assert len(e0) == len(s) and all(len(b) == 4 for b in e0)
    flat = sum(e0, [])
    assert len(set(flat)) == len(flat) and set(flat) <= set(accepted) and not set(flat) & _rejected_set()
    assert sorted(s.order(0).tolist()) == accepted, "the order is a permutation of accepted"
    assert flat == s.order(0).tolist()[:len(flat)]
    e1 = sum((b.tolist() for b in s.epoch(1)), [])
    assert e1 != flat
    again = ClipSampler(_table(), 4, min_rms_db=-50.0, min_motion=1e-3, seed=5)
    assert sum((b.tolist() for b in again.epoch(1)), []) == e1 and sum((b.tolist() for b in again.epoch(0)), []) == flat
    other = ClipSampler(_table(), 4, min_rms_db=-50.0, min_motion=1e-3, seed=6)
    assert sum((b.tolist() for b in other.epoch(0)), []) != flat
    assert all(b.dtype == torch.int64 and not b.is_cuda for b in s.epoch(2))


def test_ranks_take_disjoint_equal_shares():
    kw = dict(min_rms_db=-50.0, min_motion=1e-3, seed=1, world=3)
    ranks = [ClipSampler(_table(), 2, rank=r, **kw) for r in range(3)]
    order = ranks[0].order(4).tolist()
    shares = [sum((b.tolist() for b in s.epoch(4)), []) for s in ranks]
    assert len({len(s) for s in ranks}) == 1 and len({len(x) for x in shares}) == 1 and len(shares[0]) == len(ranks[0]) * 2
    union = sum(shares, [])
    used = len(ranks[0]) * 2 * 3
    assert len(set(union)) == len(union) == used and set(union) == set(order[:used]), "the union is the epoch less the dropped tail"
    assert used <= len(order) < used + 2 * 3
    assert all(shares[r] == order[:used][r::3] for r in range(3))


def test_drop_last_false_shuffle_false_and_recordings():
    act = _table()
    s = ClipSampler(act, 4, min_rms_db=-50.0, min_motion=1e-3, drop_last=False, shuffle=False)
    accepted = s.accepted.tolist()
    batches = [b.tolist() for b in s.epoch(0)]
    assert sum(batches, []) == accepted and len(s) == len(batches) == -(-len(accepted) // 4) and len(batches[-1]) == len(accepted) % 4 != 0
    assert [b.tolist() for b in s.epoch(9)] == batches, "shuffle=False: every epoch ascending"
    two = [ClipSampler(act, 4, min_rms_db=-50.0, min_motion=1e-3, drop_last=False, world=2, rank=r) for r in range(2)]
    shares = [sum((b.tolist() for b in t.epoch(0)), []) for t in two]
    assert len(two[0]) == len(two[1]) and len(shares[0]) == len(shares[1]) == -(-len(accepted) // 2) and set(shares[0]) | set(shares[1]) == set(accepted)
    rec = act["recording"].tolist()
    val = ClipSampler(act, 2, min_rms_db=-50.0, min_motion=1e-3, recordings=[3, 1])
    assert val.recordings == [1, 3] and val.accepted.tolist() == [i for i in accepted if rec[i] in (1, 3)]
    assert val.n_considered == sum(1 for q in rec if q in (1, 3))
    assert val.rejected["too_quiet"] == sum(1 for i in range(57) if i % 5 == 0 and rec[i] in (1, 3))
    train = ClipSampler(act, 2, min_rms_db=-50.0, min_motion=1e-3, recordings=[0, 2])
    assert not set(train.accepted.tolist()) & set(val.accepted.tolist())
    assert sorted(train.accepted.tolist() + val.accepted.tolist()) == accepted


def test_resuming_from_a_state_dict_yields_the_remaining_batches():
    kw = dict(min_rms_db=-50.0, min_motion=1e-3, seed=2)
    s = ClipSampler(_table(), 4, **kw)
    assert s.state_dict() == {"epoch": 0, "step": 0}
    full = [b.tolist() for b in s.epoch(3)]
    assert s.state_dict() == {"epoch": 4, "step": 0}
    it = s.epoch(3)
    seen = [next(it).tolist() for _ in range(3)]
    state = s.state_dict()
    assert state == {"epoch": 3, "step": 3}
    fresh = ClipSampler(_table(), 4, **kw)
    fresh.load_state_dict(state)
    rest = [b.tolist() for b in fresh.epoch(state["epoch"])]
    assert seen + rest == full and fresh.state_dict() == {"epoch": 4, "step": 0}
    assert [b.tolist() for b in fresh.epoch(3)] == full, "the resume point is used once"
    fresh.load_state_dict(state)
    assert len(list(fresh.epoch(5))) == len(full), "another epoch starts at its first batch"
    with pytest.raises(ValueError, match="state step"):
        fresh.load_state_dict({"epoch": 0, "step": len(full)})
    with pytest.raises(ValueError, match="state epoch"):
        fresh.load_state_dict({"step": 0})


def test_all_rejected_raises_with_the_counts():
    with pytest.raises(ValueError, match=r"no clip is accepted: 57 clips considered.*'too_quiet': 57"):
        ClipSampler(_table(), 4, min_rms_db=0.0)
    with pytest.raises(ValueError, match="do not fill one batch of 64"):
        ClipSampler(_table(), 64, min_rms_db=-50.0)


def test_argument_refusals():
    act = _table()
    for kw, match in ((dict(batch_size=0), "batch_size"), (dict(batch_size=True), "batch_size"), (dict(world=0), "world"),
                      (dict(rank=2, world=2), "rank 2"), (dict(seed=-1), "seed"), (dict(seed=1 << 31), "seed"),
                      (dict(min_rms_db="loud"), "min_rms_db"), (dict(min_motion=float("nan")), "min_motion"),
                      (dict(min_active_fraction=1.5), r"min_active_fraction must be in \[0, 1\]"),
                      (dict(min_active_fraction=0.5), "segments"), (dict(recordings=[4]), "recordings"), (dict(recordings=[]), "recordings")):
        args = dict(batch_size=4)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ClipSampler(act, **args)
    with pytest.raises(ValueError, match="'rms_db' must be a 1-D CPU torch.float64"):
        ClipSampler(dict(act, rms_db=act["rms_db"].float()), 4, min_rms_db=-50.0)
    with pytest.raises(ValueError, match="'n_bad' must be a 1-D CPU torch.int32 tensor of 57 clips"):
        ClipSampler(dict(act, n_bad=act["n_bad"][:5]), 4)
    with pytest.raises(ValueError, match="'recording'"):
        ClipSampler({"rms_db": act["rms_db"]}, 4)
    with pytest.raises(ValueError, match="expected a ClipBank"):
        ClipSampler([1, 2, 3], 4)
    s = ClipSampler(act, 4)
    with pytest.raises(ValueError, match="epoch"):
        next(s.epoch(-1))


# ---- the entry points refuse before they touch the device ----------------------------------------------------------------------------
def test_activity_entry_points_validate_their_arguments():
    import ctypes
    assert _lib.query("maavss_bank_level_chunks", 1) == 1 and _lib.query("maavss_bank_level_chunks", 16384) == 1
    assert _lib.query("maavss_bank_level_chunks", 16385) == 2 and _lib.query("maavss_bank_level_chunks", -1) == -1
    max_j = _lib.query("maavss_bank_max_segments")
    assert max_j == 2048
    rec = (ctypes.c_int64 * 6)(0, 100, 100, 50, 0, 1)            # two recordings: starts, samples, first partial
    p = ctypes.addressof(rec)
    with pytest.raises(_lib.MaavssError, match="bank_recording_level: null pointer"):
        _lib.call("maavss_bank_recording_level", 256, 150, 256, None, 2, 256, 2, 256, None)
    with pytest.raises(_lib.MaavssError, match="must be positive"):
        _lib.call("maavss_bank_recording_level", 256, 150, 256, p, -2, 256, 2, 256, None)
    with pytest.raises(_lib.MaavssError, match=r"recording 1 \(samples \[100, 100 \+ 50\)\) lies outside the bank's 120 samples"):
        _lib.call("maavss_bank_recording_level", 256, 120, 256, p, 2, 256, 2, 256, None)
    with pytest.raises(_lib.MaavssError, match="2 chunk partials needed, room for 1"):
        _lib.call("maavss_bank_recording_level", 256, 150, 256, p, 2, 256, 1, 256, None)
    rec[5] = 3
    with pytest.raises(_lib.MaavssError, match="recording 1's first partial is 3, expected 1"):
        _lib.call("maavss_bank_recording_level", 256, 150, 256, p, 2, 256, 2, 256, None)
    long_rec = (ctypes.c_int64 * 3)(0, 65536 * 16384, 0)
    with pytest.raises(_lib.MaavssError, match="more than 65535 chunks"):
        _lib.call("maavss_bank_recording_level", 256, 65536 * 16384, 256, ctypes.addressof(long_rec), 1, 256, 1 << 20, 256, None)
    with pytest.raises(_lib.MaavssError, match="8-byte aligned"):
        _lib.call("maavss_bank_recording_level", 256, 150, 260, p, 2, 256, 2, 256, None)

    with pytest.raises(_lib.MaavssError, match="bank_frame_motion: null pointer"):
        _lib.call("maavss_bank_frame_motion", 256, 0, 4, 4, None, None)
    with pytest.raises(_lib.MaavssError, match=r"storage must be 0 \(f32\) or 1 \(u16\), got 2"):
        _lib.call("maavss_bank_frame_motion", 256, 2, 4, 4, 256, None)
    with pytest.raises(_lib.MaavssError, match="hold no pair"):
        _lib.call("maavss_bank_frame_motion", 256, 0, 1, 4, 256, None)
    with pytest.raises(_lib.MaavssError, match="hold no pair"):
        _lib.call("maavss_bank_frame_motion", 256, 0, -3, 4, 256, None)

    cs = (ctypes.c_int64 * 2)(0, 40)
    cf, cr = (ctypes.c_int32 * 2)(0, 3), (ctypes.c_int32 * 2)(0, 1)
    hs, hf, hr = (ctypes.addressof(x) for x in (cs, cf, cr))

    def activity(n_samples=150, n_frames=8, n_rec=2, n_clips=2, T=5, hpf=2, hop=6, factor=1e-4, D=256, out=256, host=(hs, hf, hr), last_out=256):
        _lib.call("maavss_bank_clip_activity", 256, n_samples, D, n_frames, 256, 256, n_rec, 256, 256, 256, *host, n_clips, T, hpf, hop, factor,
                  out, 256, 256, 256, 256, 256, 256, last_out, None)

    for kw, match in ((dict(host=(None, hf, hr)), "bank_clip_activity: null pointer"), (dict(out=None), "null output pointer"),
                      (dict(last_out=None), "null output pointer"), (dict(n_clips=-1), "must be positive"), (dict(n_rec=0), "must be positive"),
                      (dict(hop=0), "must be positive"), (dict(T=5, hpf=410), f"J = hops_per_frame \\* clip_frames = 2050 segments, the kernel holds {max_j}"),
                      (dict(n_samples=59), "hold no clip"), (dict(D=None), "D is required"), (dict(factor=2.0), "floor_factor"),
                      (dict(n_samples=99), r"clip 1 \(sample 40, frame 3, recording 1\) lies outside the bank"),
                      (dict(n_frames=7), r"clip 1 \(sample 40, frame 3, recording 1\) lies outside the bank"),
                      (dict(n_rec=1), r"clip 1 \(sample 40, frame 3, recording 1\) lies outside the bank")):
        with pytest.raises(_lib.MaavssError, match=match):
            activity(**kw)
    cs[0] = -1
    with pytest.raises(_lib.MaavssError, match=r"clip 0 \(sample -1, frame 0, recording 0\)"):
        activity()

    def select(n_clips=4, enabled=127, first=256, reasons=256):
        _lib.call("maavss_bank_clip_select", first, 256, 256, 256, 256, 256, 256, n_clips, enabled, -50.0, -20.0, 4.0, 1e-3, 0.3, 1.0, reasons, None)

    for kw, match in ((dict(first=None), "bank_clip_select: null pointer"), (dict(reasons=None), "bank_clip_select: null pointer"),
                      (dict(n_clips=-4), "n_clips = -4"), (dict(enabled=128), "enabled = 128"), (dict(first=260), "8-byte aligned")):
        with pytest.raises(_lib.MaavssError, match=match):
            select(**kw)
