"""csrc/stoi.hip on the GPU against the float64 twin (tests/stoi_twin.py).

Cases at 10 kHz: row lengths 255, 256, 257 (no frame, no frame, one), 4096 (30 frames: no segment), 4097 and 4224 (31: one segment), 4225
(two), 5280 (the project's clip), 30000 (233 frames: the select kernel's second round of 256); silence at the start, at the end, in the
middle, and enough of it to leave 29 frames; one row and three rows that keep 41, 45 and 42 frames; a row stride past the row, overlapping
rows, est and ref 1, 2 and 3 elements off a 16-byte boundary; a NaN, an inf, a NaN past the last frame and a silent reference between
ordinary rows.  One case at 16 kHz goes through the device resampler first.

Counts must equal the twin's exactly.  The gate on the scores was set from a measurement, as the rule was fixed beforehand: the largest
|gpu - twin| over every finite row of these cases on one MI355X (profiles/stoi_parity.json, scripts/stoi_parity.py) was 1.22e-15
(MEASURED_MAX below); the gate is 8 x that, rounded up to a power of ten = 1e-14, and never more than 1e-9 -- three orders under the smallest change an
indexing error of one bin or one sample makes (tests/test_stoi_cpu.py).  The margin is for summation order and the last bit of cos and
of the twiddles, which vary with the data."""
import math

import numpy as np
import pytest
import torch

import maavss_amd
import stoi_twin as tw

pytestmark = pytest.mark.gpu

MEASURED_MAX = 1.23e-15        # profiles/stoi_parity.json, max_abs_diff over 42 finite scores (1.22e-15, at bad[0] estoi)
GATE = 1e-14                   # 8 x 1.23e-15 = 9.8e-15, rounded up to a power of ten


def _place(rows, stride, off):
    """rows [B, L] numpy f32 -> a device view [B, L] with row stride `stride` whose first element is `off` elements past a 256-byte
    boundary (torch's allocations start on one)."""
    b, n = rows.shape
    flat = np.zeros(off + (b - 1) * stride + n + 8, dtype=np.float32)
    for i in range(b):
        flat[off + i * stride:off + i * stride + n] = rows[i]
    dev = torch.from_numpy(flat).cuda()
    assert dev.data_ptr() % 256 == 0
    view = dev.as_strided((b, n), (stride, 1), off)
    assert view.data_ptr() % 16 == 4 * off % 16
    return view


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _records(label, got, est, ref):
    assert got.shape == (est.shape[0], 4)
    return [dict(label=f"{label}[{i}]", got=got[i], want=tw.stoi_row(est[i], ref[i])) for i in range(est.shape[0])]


def measure_10k():
    """Every 10 kHz case once -> [dict(label, got [4], want)]."""
    out = []
    for k, (name, n, _) in enumerate(tw.GPU_CASES):                     # one row each, 1, 2, 3 elements off a 16-byte boundary
        est, ref = (a[None] for a in tw.gpu_case(name))
        res = maavss_amd.stoi_metrics(_place(est, n + 5, 1 + k % 3), _place(ref, n + 9, 1 + (k + 1) % 3))
        assert res["stoi"].shape == (1,) and res["stoi"].dtype == torch.float64 and res["stoi"].is_cuda
        out += _records(name, _host(res["raw"]), est, ref)
    pairs = [tw.gpu_case(name) for name in tw.BATCH]                    # three rows of one call with different kept counts
    est, ref = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    out += _records("batch", _host(maavss_amd.stoi_metrics(_place(est, 6000 + 7, 2), _place(ref, 6000, 0))["raw"]), est, ref)
    o = tw.OVERLAP                                                      # overlapping rows: stride < n
    est_sig, ref_sig = (torch.from_numpy(s).cuda() for s in tw.overlap_signals())
    est, ref = tw.overlap_rows()
    got = maavss_amd.stoi_metrics(est_sig.as_strided((o["rows"], o["n"]), (o["stride"], 1), o["off_est"]),
                                  ref_sig.as_strided((o["rows"], o["n"]), (o["stride"], 1), o["off_ref"]))["raw"]
    out += _records("overlap", _host(got), est, ref)
    est, ref, kinds = tw.bad_rows()
    out += _records("bad", _host(maavss_amd.stoi_metrics(torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda())["raw"]), est, ref)
    # a one-dimensional slice at an odd offset, as Validator.add_recording passes clean[start:start + n]
    e1, r1 = (torch.from_numpy(a).cuda() for a in tw.gpu_case("L30000"))
    res = maavss_amd.stoi_metrics(e1[3:3 + 5280], r1[3:3 + 5280])
    out += _records("slice", _host(res["raw"]), _host(e1[3:3 + 5280])[None], _host(r1[3:3 + 5280])[None])
    return out


def measure_16k():
    """3 x 8448 at 16 kHz: the GPU's scores against the twin applied to the device-resampled rows (the resampler's own f32 error is
    bounded by its own tests)."""
    pairs = [tw.make_case(900 + i, 8448, 5.0) for i in range(3)]
    est, ref = (torch.from_numpy(np.stack([p[k] for p in pairs])).cuda() for k in (0, 1))
    got = _host(maavss_amd.stoi_metrics(est, ref, sr=16000)["raw"])
    down = maavss_amd.AudioTransform(10000)
    est10, ref10 = _host(down(est, 16000, batched=True)), _host(down(ref, 16000, batched=True))
    assert est10.shape == (3, 5280)
    for i in range(3):
        assert tw.margin_db(ref10[i]) >= 1e-6, "a resampled frame sits on the 40 dB decision: choose another seed"
    return _records("sr16000", got, est10, ref10)


def max_difference(records):
    """-> (the largest |gpu - twin| over the finite scores, its label)"""
    worst, where = 0.0, None
    for r in records:
        for c, key in enumerate(("stoi", "estoi")):
            if math.isfinite(r["want"][key]):
                d = abs(float(r["got"][c]) - r["want"][key])
                if d > worst:
                    worst, where = d, f"{r['label']} {key}"
    return worst, where


@pytest.fixture(scope="module")
def records():
    return measure_10k()


def test_kept_frames_and_segments_equal_the_twin_exactly(records):
    labels = [r["label"] for r in records]
    assert len(records) == len(tw.GPU_CASES) + 3 + 3 + 6 + 1 and len(set(labels)) == len(labels)
    for r in records:
        got, want = r["got"], r["want"]
        assert (got[2], got[3]) == (want["n_kept"], want["n_segments"]), (r["label"], got, want)
        assert math.isnan(got[0]) == math.isnan(want["stoi"]) and math.isnan(got[1]) == math.isnan(want["estoi"]), (r["label"], got, want)
    by = {r["label"]: r["got"] for r in records}
    assert [by[f"{n}[0]"][2] for n in ("L255", "L256", "L257", "L4096", "L4097", "L4224", "L4225", "L5280", "L30000")] == [0, 0, 1, 30, 31, 31, 32, 40, 233]
    assert by["silent_too_much[0]"][2] == 29 and math.isnan(by["silent_too_much[0]"][0])
    assert len({by[f"batch[{i}]"][2] for i in range(3)}) == 3
    # NaN in the bad rows only: the ordinary rows around them score
    kinds = tw.bad_rows()[2]
    for i, kind in enumerate(kinds):
        g = by[f"bad[{i}]"]
        if kind == "fine":
            assert math.isfinite(g[0]) and math.isfinite(g[1]) and g[3] == 10
        else:
            assert math.isnan(g[0]) and math.isnan(g[1]) and g[2] == 0 and g[3] == 0, (kind, g)


def test_scores_equal_the_twin_within_the_gate(records):
    finite = 0
    for r in records:
        for c, key in enumerate(("stoi", "estoi")):
            if math.isfinite(r["want"][key]):
                finite += 1
                print(f"{r['label']}: {key} {float(r['got'][c])!r} twin {r['want'][key]!r} |diff| {abs(float(r['got'][c]) - r['want'][key]):.3g}")
    worst, where = max_difference(records)
    print(f"largest |gpu - twin| {worst:.3g} at {where}; gate {GATE:g}")
    assert finite >= 2 * 18
    assert GATE <= 1e-9
    assert worst <= GATE, (worst, where)


def test_the_16_khz_case_goes_through_the_device_resampler():
    recs = measure_16k()
    for r in recs:
        print(f"{r['label']}: got {list(map(float, r['got']))} twin {r['want']}")
        assert (r["got"][2], r["got"][3]) == (r["want"]["n_kept"], r["want"]["n_segments"]) and r["want"]["n_segments"] > 0
    worst, where = max_difference(recs)
    print(f"largest |gpu - twin| {worst:.3g} at {where}")
    assert worst <= GATE, (worst, where)


def test_two_calls_give_identical_bytes():
    for name, b in (("L30000", 1), ("L5280", 3)):
        est, ref = tw.gpu_case(name)
        est, ref = (torch.from_numpy(np.stack([np.roll(a, 17 * i) for i in range(b)])).cuda() for a in (est, ref))
        first = maavss_amd.stoi_metrics(est, ref)["raw"].clone()
        torch.empty(1 << 20, device="cuda").fill_(float("nan"))          # another workspace content between the calls
        second = maavss_amd.stoi_metrics(est, ref)["raw"]
        torch.cuda.synchronize()
        assert torch.isfinite(first[:, :2]).all()
        assert first.view(torch.int64).equal(second.view(torch.int64)), "two runs differ"


def test_validator_accumulates_the_scores_and_waits_only_in_result():
    batches = tw.validator_batches()
    dev = [[torch.from_numpy(a).cuda() for a in batch] for batch in batches]
    val = maavss_amd.Validator(None, intelligibility_sr=10000)
    plain = maavss_amd.Validator(None)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")             # any blocking call of torch's before result() raises
    try:
        for est, ref, noisy in dev:
            val.add_waves(est, ref, noisy)
            plain.add_waves(est, ref, noisy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    res, res_plain = val.result(), plain.result()
    est_rows = [tw.stoi_row(e, r) for est, ref, _ in batches for e, r in zip(est, ref)]
    noisy_rows = [tw.stoi_row(q, r) for _, ref, noisy in batches for q, r in zip(noisy, ref)]
    assert sum(math.isnan(r["stoi"]) for r in est_rows) == 1 and not any(math.isnan(r["stoi"]) for r in noisy_rows)
    for key in ("stoi", "estoi"):
        e, q = [r[key] for r in est_rows], [r[key] for r in noisy_rows]
        fin = [v for v in e if math.isfinite(v)]
        gain = [a - b for a, b in zip(e, q) if math.isfinite(a)]
        assert res[key + "_n_finite"] == 4 and res[key + "_n_nan"] == 1
        assert res["noisy_" + key + "_n_finite"] == 5 and res["noisy_" + key + "_n_nan"] == 0
        assert res[key + "_improvement_n_finite"] == 4 and res[key + "_improvement_n_nan"] == 1
        print(f"{key}: {res[key]!r} twin {math.fsum(fin) / 4!r}; noisy {res['noisy_' + key]!r} twin {math.fsum(q) / 5!r}; "
              f"improvement {res[key + '_improvement']!r} twin {math.fsum(gain) / 4!r}")
        assert abs(res[key] - math.fsum(fin) / 4) <= GATE
        assert abs(res["noisy_" + key] - math.fsum(q) / 5) <= GATE
        assert abs(res[key + "_improvement"] - math.fsum(gain) / 4) <= 2 * GATE
        assert res[key + "_improvement"] > 0.05, "10 dB against 0 dB must be heard"
    # the option changes nothing else: the first accumulator has the same bytes, the other keys the same values
    assert val.acc.shape == plain.acc.shape == (51,) and val.acc_intel.shape == (30,) and plain.acc_intel is None
    assert val.acc.view(torch.int64).equal(plain.acc.view(torch.int64))
    assert set(res) - set(res_plain) == {k + s for k in ("stoi", "estoi", "noisy_stoi", "noisy_estoi", "stoi_improvement", "estoi_improvement")
                                         for s in ("", "_n_finite", "_n_nan")}
    for k, v in res_plain.items():
        assert res[k] == v or (v != v and res[k] != res[k]), k
    val.reset()
    again = val.result()
    assert again["stoi_n_finite"] == 0 and math.isnan(again["stoi"]) and again["n_clips"] == 0


def test_the_default_validator_reports_what_wave_metrics_gives():
    """Without the option the Validator is what it was: the keys of before, each mean the mean of wave_metrics' rows."""
    est, ref, noisy = (torch.from_numpy(a).cuda() for a in tw.validator_batches()[0])
    val = maavss_amd.Validator(None)
    val.add_waves(est, ref, noisy)
    res = val.result()
    assert not any("stoi" in k for k in res) and val.acc.numel() == 51 and val.acc_intel is None
    m, mn = maavss_amd.wave_metrics(est, ref), maavss_amd.wave_metrics(noisy, ref)
    for name in ("snr_db", "si_sdr_db", "seg_snr_db"):
        e, q = _host(m[name]), _host(mn[name])
        assert abs(res[name] - e.sum() / 3) <= 1e-12 and abs(res["noisy_" + name] - q.sum() / 3) <= 1e-12
        assert abs(res[name + "_improvement"] - (e - q).sum() / 3) <= 1e-12 and res[name + "_n_finite"] == 3
    assert res["n_clips"] == 3
