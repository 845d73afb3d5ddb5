"""csrc/bss_eval.hip on the GPU against the float64 twin (tests/bss_twin.py).

Cases (L, N, K): (1, 300, 1), (2, 64, 0), (33, 700, 1), (64, 1500, 2) with one other source all-zero (J = 2), (65, 1000, 1),
(512, 4000, 1), (512, 8448, 1) (the project's clip), (64, 70 000, 1) (35 correlation chunks, 69 fir chunks) and (512, 2048, 3) (2048
unknowns, the limit); three rows of one call with J = 3, 2 and 1; row strides past the row, overlapping rows, inputs 1, 2 and 3 elements
off a 16-byte boundary, other sources with a source stride that is not the row length; a NaN, an inf and a silent target between
ordinary rows; a one-dimensional slice at an odd offset.  Apart from these: 32 x 8448 with 512 taps against its rows one by one, and
1024 rows against the same rows in groups of 32 -- more workgroups than the device holds at once.

n_sources and status must equal the twin's exactly.  The gate on the scores (dB, absolute) and on the five sums (relative) was set from
a measurement, the rule fixed beforehand: the largest difference over every finite value of these cases on one MI355X
(profiles/bss_parity.json, scripts/bss_parity.py) is MEASURED_MAX; the gate is 8 x that, rounded up to a power of ten, and never more
than CEILING = one thousandth of the smallest score change that a filter one tap too short or a source one sample late makes on these
cases (tests/test_bss_cpu.py prints it).  The margin is for summation order, which varies with the data."""
import math

import numpy as np
import pytest
import torch

import maavss_amd
import bss_twin as tw

pytestmark = pytest.mark.gpu

MEASURED_MAX = 2.49e-14        # profiles/bss_parity.json, max_diff over 140 finite values (2.487e-14 dB, sir_db of L65; the sums: 6.8e-15)
GATE = 1e-12                   # 8 x 2.49e-14 = 2.0e-13, rounded up to a power of ten
CEILING = 7.4e-5               # the smallest off-by-one change tests/test_bss_cpu.py finds is 0.0749 dB (sir_db, a filter one tap shorter)


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


def _place_sources(oth, row_stride, src_stride, off):
    """oth [B, K, L] numpy f32 -> a device view [B, K, L] with strides (row_stride, src_stride, 1), `off` elements past a boundary"""
    b, k, n = oth.shape
    flat = np.zeros(off + (b - 1) * row_stride + (k - 1) * src_stride + n + 8, dtype=np.float32)
    for i in range(b):
        for j in range(k):
            o = off + i * row_stride + j * src_stride
            flat[o:o + n] = oth[i, j]
    dev = torch.from_numpy(flat).cuda()
    view = dev.as_strided((b, k, n), (row_stride, src_stride, 1), off)
    assert not view.is_contiguous() or b * k == 1
    return view


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _records(label, got, est, ref, oth, filt_len, want=None):
    assert got.shape == (est.shape[0], 10)
    return [dict(label=f"{label}[{i}]", got=got[i], want=want if want is not None else tw.bss_row(est[i], ref[i], oth[i], filt_len))
            for i in range(est.shape[0])]


def measure():
    """Every case once -> [dict(label, got [10], want)]."""
    out = []
    for k, (name, filt_len, n, nk, _, _) in enumerate(tw.GPU_CASES):     # one row each, 1, 2, 3 elements off a 16-byte boundary
        est, ref, oth = tw.gpu_case(name)
        others = _place_sources(oth[None], nk * (n + 7) + 3, n + 7, 1 + (k + 2) % 3) if nk else None
        res = maavss_amd.bss_eval_metrics(_place(est[None], n + 5, 1 + k % 3), _place(ref[None], n + 9, 1 + (k + 1) % 3), others, filt_len)
        assert res["sdr_db"].shape == (1,) and res["sdr_db"].dtype == torch.float64 and res["sdr_db"].is_cuda
        out += _records(name, _host(res["raw"]), est[None], ref[None], oth[None], filt_len, tw.gpu_case_want(name))
    b = tw.BATCH                                                        # three rows of one call with J = 3, 2, 1; strides past the row
    est, ref, oth = tw.batch_rows()
    got = maavss_amd.bss_eval_metrics(_place(est, b["n"] + 7, 2), _place(ref, b["n"], 3), _place_sources(oth, 2 * b["n"] + 13, b["n"] + 2, 1),
                                      b["filt_len"])["raw"]
    out += _records("batch", _host(got), est, ref, oth, b["filt_len"])
    o = tw.OVERLAP                                                      # overlapping rows: stride < n
    sig = [torch.from_numpy(s).cuda() for s in tw.overlap_signals()]
    est, ref, oth = tw.overlap_rows()
    got = maavss_amd.bss_eval_metrics(sig[0].as_strided((o["rows"], o["n"]), (o["stride"], 1), o["off_est"]),
                                      sig[1].as_strided((o["rows"], o["n"]), (o["stride"], 1), o["off_ref"]),
                                      sig[2].as_strided((o["rows"], 1, o["n"]), (o["stride"], 1, 1), o["off_oth"]), o["filt_len"])["raw"]
    out += _records("overlap", _host(got), est, ref, oth, o["filt_len"])
    est, ref, oth, _ = tw.bad_rows()
    got = maavss_amd.bss_eval_metrics(torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda(), torch.from_numpy(oth[:, 0]).cuda(), 33)["raw"]
    out += _records("bad", _host(got), est, ref, oth, 33)
    # a one-dimensional slice at an odd offset, as Validator.add_recording passes clean[start:start + n]
    e1, r1, o1 = (torch.from_numpy(a).cuda() for a in tw.gpu_case("L65"))
    res = maavss_amd.bss_eval_metrics(e1[3:3 + 900], r1[3:3 + 900], o1[:, 3:3 + 900], 65)
    out += _records("slice", _host(res["raw"]), _host(e1[3:903])[None], _host(r1[3:903])[None], _host(o1[:, 3:903])[None], 65)
    return out


def differences(records):
    """-> [(difference, label, column)]: |gpu - twin| in dB of every finite score, the relative difference of every finite non-zero sum"""
    out = []
    for r in records:
        if r["want"]["status"] != 0:
            continue
        for c, key in enumerate(tw.COLUMNS[:8]):
            w, g = r["want"][key], float(r["got"][c])
            if not math.isfinite(w) or w == 0.0:
                continue
            out.append((abs(g - w) if key in tw.SCORES else abs(g - w) / abs(w), r["label"], key))
    return out


@pytest.fixture(scope="module")
def records():
    return measure()


def test_live_sources_and_status_equal_the_twin_exactly(records):
    labels = [r["label"] for r in records]
    assert len(records) == len(tw.GPU_CASES) + 3 + 3 + 6 + 1 and len(set(labels)) == len(labels)
    for r in records:
        got, want = r["got"], r["want"]
        assert (got[8], got[9]) == (want["n_sources"], want["status"]), (r["label"], got, want)
        for c, key in enumerate(tw.COLUMNS[:8]):
            assert math.isnan(got[c]) == math.isnan(want[key]), (r["label"], key, got, want)
    by = {r["label"]: r["got"] for r in records}
    assert [by[f"{c[0]}[0]"][8] for c in tw.GPU_CASES] == [2, 1, 2, 2, 2, 2, 2, 2, 4]
    assert [by[f"batch[{i}]"][8] for i in range(3)] == [3, 2, 1]
    kinds = tw.bad_rows()[3]
    want_status = dict(fine=0, nan_est=1, inf_other=1, silent_target=2, nan_ref_tail=1)
    for i, kind in enumerate(kinds):
        g = by[f"bad[{i}]"]
        assert g[9] == want_status[kind], (kind, g)
        if kind == "fine":
            assert np.isfinite(g).all() and g[8] == 2
        else:
            assert np.isnan(g[:8]).all() and g[8] == 0, (kind, g)


def test_one_live_source_has_no_interference(records):
    """J = 1: S_ii is exactly 0, sir_db is +inf and sar_db equals sdr_db bit for bit."""
    rows = [r for r in records if r["want"]["status"] == 0 and r["want"]["n_sources"] == 1]
    assert {r["label"] for r in rows} == {"L2_alone[0]", "batch[2]"}
    for r in rows:
        g = r["got"]
        assert g[2] == 0.0 and g[6] == math.inf and g[7].tobytes() == g[5].tobytes() and g[3].tobytes() == g[1].tobytes(), (r["label"], g)


def test_scores_and_sums_equal_the_twin_within_the_gate(records):
    diffs = differences(records)
    for d, label, key in diffs:
        print(f"{label}: {key} differs by {d:.3g}")
    worst = max(diffs)
    print(f"largest difference {worst[0]:.3g} at {worst[1]} {worst[2]}; gate {GATE}, ceiling {CEILING}")
    assert len(diffs) >= 7 * 17
    assert GATE <= CEILING
    assert worst[0] <= GATE, worst


def test_two_calls_give_identical_bytes_and_rows_do_not_depend_on_the_batch():
    est, ref, oth = (torch.from_numpy(a).cuda() for a in tw.batch_rows())
    filt_len = tw.BATCH["filt_len"]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")             # the call only enqueues: any blocking call of torch's raises
    try:
        first = maavss_amd.bss_eval_metrics(est, ref, oth, filt_len)["raw"].clone()
        torch.empty(1 << 20, device="cuda").fill_(float("nan"))          # another workspace content between the calls
        second = maavss_amd.bss_eval_metrics(est, ref, oth, filt_len)["raw"]
        single = torch.cat([maavss_amd.bss_eval_metrics(est[i:i + 1], ref[i:i + 1], oth[i:i + 1], filt_len)["raw"] for i in range(3)])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(first[:, :6]).all()
    assert first.view(torch.int64).equal(second.view(torch.int64)), "two runs differ"
    assert first.view(torch.int64).equal(single.view(torch.int64)), "a row depends on the other rows of its call"


def test_a_batch_of_clips_equals_its_rows_one_by_one():
    """32 x 8448 with 512 taps and one other source, the benchmark's shape: 17 panel workgroups per row, more than are resident at
    once.  Every row of the batch has the bytes of a call of its own, and the last row the twin's scores."""
    est, ref, oth = tw.clip_batch()
    e, r, o = (torch.from_numpy(a).cuda() for a in (est, ref, oth))
    filt_len = tw.CLIP_BATCH["filt_len"]
    whole = maavss_amd.bss_eval_metrics(e, r, o, filt_len)["raw"].clone()
    single = torch.cat([maavss_amd.bss_eval_metrics(e[i:i + 1], r[i:i + 1], o[i:i + 1], filt_len)["raw"] for i in range(e.shape[0])])
    torch.cuda.synchronize()
    assert (whole[:, 9] == 0).all() and torch.isfinite(whole).all()
    differ = (whole.view(torch.int64) != single.view(torch.int64)).any(dim=1).nonzero().flatten().tolist()
    assert not differ, f"rows {differ} of the batch differ from their own calls"
    for i in tw.CLIP_BATCH["checked"]:
        want = tw.bss_row(est[i], ref[i], oth[i], filt_len)
        for c, key in enumerate(tw.COLUMNS[:8]):
            g = float(whole[i, c])
            assert (abs(g - want[key]) if key in tw.SCORES else abs(g - want[key]) / abs(want[key])) <= GATE, (i, key, g, want[key])


def test_more_workgroups_than_the_device_holds_at_once(monkeypatch):
    """1024 rows (overlapping windows of one signal), 66 unknowns each: three panel workgroups per row, 3072 in a launch, several times
    what is resident at once, so some start after others of their row have finished -- and must read what those read.  In groups of 32
    rows every workgroup of a launch is resident; both ways must give the same bytes, and the twin's scores on the rows checked."""
    import maavss_amd.bss as bss
    o = tw.MANY
    rows, n, filt_len = o["rows"], o["n"], o["filt_len"]
    e, r, oth = (torch.from_numpy(a).cuda().as_strided((rows, n), (o["stride"], 1), o["off"]) for a in tw.many_signals())
    whole = bss.bss_eval_metrics(e, r, oth, filt_len)["raw"].clone()
    monkeypatch.setattr(bss, "BSS_WORKSPACE_CAP", 32 * int(bss.query("maavss_bss_eval_ws_bytes", 1, n, 1, filt_len)))
    grouped = bss.bss_eval_metrics(e, r, oth, filt_len)["raw"]
    torch.cuda.synchronize()
    assert (whole[:, 9] == 0).all() and (whole[:, 8] == 2).all() and torch.isfinite(whole).all()
    assert whole.view(torch.int64).equal(grouped.view(torch.int64))
    for i in o["checked"]:
        want = tw.bss_row(*tw.many_row(i), filt_len)
        for c, key in enumerate(tw.COLUMNS[:8]):
            g = float(whole[i, c])
            assert (abs(g - want[key]) if key in tw.SCORES else abs(g - want[key]) / abs(want[key])) <= GATE, (i, key, g, want[key])


def test_the_grouping_under_the_workspace_cap_changes_nothing(monkeypatch):
    import maavss_amd.bss as bss
    est, ref, oth = (torch.from_numpy(a).cuda() for a in tw.batch_rows())
    whole = bss.bss_eval_metrics(est, ref, oth, 33)["raw"].clone()
    monkeypatch.setattr(bss, "BSS_WORKSPACE_CAP", 2 * int(bss.query("maavss_bss_eval_ws_bytes", 1, est.shape[1], 2, 33)))
    grouped = bss.bss_eval_metrics(est, ref, oth, 33)["raw"]
    torch.cuda.synchronize()
    assert whole.view(torch.int64).equal(grouped.view(torch.int64))
