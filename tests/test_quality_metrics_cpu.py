"""CPU-only part of the quality metrics (maavss_amd/quality.py, csrc/quality_metrics.hip): known answers of the float64 twin, the chunk
planner, exports and the pinned ABI version, the argument checks of the new entry points (every call below fails before any launch)
the Validator's refusals, result() on a known buffer and the launches add_waves enqueues."""
import inspect
import itertools
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import quality_twin as tw
from maavss_amd import _lib

CH = 4096          # the library's chunk length; test_chunk_length_is_the_librarys pins the two together


def test_chunk_length_is_the_librarys():
    import maavss_amd.quality as q
    assert q.wave_chunk() == CH == _lib.query("maavss_wave_metrics_chunk")


def test_twin_snr_of_noise_scaled_to_20_db():
    sign = np.where(np.arange(64) % 3 == 0, -1.0, 1.0)
    ref = (10.0 * sign).astype(np.float32)                     # Sxx = 100 L
    est = (ref + np.where(np.arange(64) % 2 == 0, 1.0, -1.0)).astype(np.float32)       # See = L
    r = tw.wave_row(est, ref, 16)
    assert r["sxx"] == 6400.0 and r["see"] == 64.0
    assert abs(r["snr_db"] - 20.0) <= 4 * tw.U53 * 20.0
    assert r["n_frames"] == 4 and abs(r["seg_snr_db"] - 20.0) <= 8 * tw.U53 * 20.0


def test_twin_scaled_orthogonal_and_silent_rows():
    rng = np.random.default_rng(3)
    ref = rng.standard_normal(100).astype(np.float32)
    r = tw.wave_row(2 * ref, ref, 10)                          # est = 2 ref: See = Sxx, alpha = 2 exactly, no residual
    assert r["snr_db"] == 0.0 and r["alpha"] == 2.0 and r["srr"] == 0.0 and r["si_sdr_db"] == math.inf
    r = tw.wave_row(ref, ref, 10)
    assert r["snr_db"] == math.inf and r["si_sdr_db"] == math.inf and r["seg_snr_db"] == 35.0
    ones = np.ones(8, dtype=np.float32)
    r = tw.wave_row(ones * np.array([1, -1] * 4, dtype=np.float32), ones, 4)           # est orthogonal to ref
    assert r["sxy"] == 0.0 and r["si_sdr_db"] == -math.inf
    r = tw.wave_row(ref, np.zeros(100, dtype=np.float32), 10)                          # silent reference
    assert all(math.isnan(r[k]) for k in ("snr_db", "si_sdr_db", "seg_snr_db")) and r["n_frames"] == 0
    bad = ref.copy()
    bad[7] = np.inf
    r = tw.wave_row(bad, ref, 10)
    assert all(math.isnan(r[k]) for k in ("sxx", "see", "srr", "snr_db", "si_sdr_db", "seg_snr_db")) and r["n_frames"] == 0


def test_twin_frames_clamp_at_minus_10_and_35_and_skip_silence():
    seg = 8
    ref = np.concatenate([np.ones(seg), np.ones(seg), np.zeros(seg), np.ones(seg), np.ones(3)]).astype(np.float32)
    est = ref.copy()
    est[seg:2 * seg] = 100.0                                   # frame 1: error 99 x the reference, -39.9 dB -> -10
    est[2 * seg:3 * seg] = 0.5                                 # frame 2: no reference energy, left out
    est[3 * seg:4 * seg] = 1.5                                 # frame 3: 10 log10(1 / 0.25) = 6.02 dB
    est[4 * seg:] = 7.0                                        # the trailing partial frame is dropped
    r = tw.wave_row(est, ref, seg)
    assert r["n_frames"] == 3
    assert abs(r["seg_snr_db"] - (35.0 - 10.0 + 10.0 * math.log10(4.0)) / 3.0) <= 1e-13
    assert math.isnan(tw.wave_row(est[:seg - 1], ref[:seg - 1], seg)["seg_snr_db"])    # no complete frame


def test_twin_lsd_of_a_scaled_spectrum_and_of_bins_under_the_floor():
    rng = np.random.default_rng(4)
    tgt = rng.standard_normal((2, 3, 5)).astype(np.float32)
    r = tw.spectrum_row(4 * tgt, tgt)                          # every power 16 x (exact in f32): 12.04 dB in every bin
    assert abs(r["lsd_db"] - 10.0 * math.log10(16.0)) <= 1e-12
    assert abs(r["sqerr"] - 9.0 * float((tgt.astype(np.float64) ** 2).sum())) <= 1e-9
    tiny = (1e-7 * tgt).astype(np.float32)                     # powers ~1e-14, under the floor in both operands
    assert tw.spectrum_row(tiny, 0.5 * tiny)["lsd_db"] == 0.0
    r = tw.spectrum_row(tiny, np.full_like(tgt, 1.0))          # floor against power 2: 10 log10(2e10) in every bin
    assert abs(r["lsd_db"] - 10.0 * math.log10(2e10)) <= 1e-12


@pytest.mark.parametrize("seg_len", [1, 7, 256, CH])
def test_plan_wave_chunks_covers_every_sample_once_in_whole_frames(seg_len):
    import maavss_amd
    for length in tw.wave_lengths(CH, seg_len) + [960000 if seg_len == 256 else 5 * CH + 1]:
        rows = maavss_amd.plan_wave_chunks(length, seg_len, CH)
        seen = np.zeros(length, dtype=np.int32)
        for k, (a, n) in enumerate(rows):
            assert 1 <= n <= CH and a % seg_len == 0, "a chunk starts inside a frame"
            assert n % seg_len == 0 or k == len(rows) - 1, "only the row's last chunk may hold a partial frame"
            seen[a:a + n] += 1
        assert np.all(seen == 1)
        assert [a for a, _ in rows] == sorted(a for a, _ in rows)
        # the library plans the same cut: its workspace is sized by the chunk count
        want = -(-48 * len(rows) // 256) * 256 + -(-8 * len(rows) // 256) * 256 + 256
        assert _lib.query("maavss_wave_metrics_ws_bytes", 1, length, seg_len) == want
    assert len(maavss_amd.plan_wave_chunks(960000, 256, CH)) == 235            # one 60 s recording: many workgroups
    for bad in (0, CH + 1):
        with pytest.raises(ValueError):
            maavss_amd.plan_wave_chunks(100, bad, CH)


def test_workspace_queries_answer_zero_for_invalid_arguments():
    for bad in ((0, 10, 4), (1, 0, 4), (1, 10, 0), (1, 10, CH + 1)):
        assert _lib.query("maavss_wave_metrics_ws_bytes", *bad) == 0
    assert _lib.query("maavss_spectrum_metrics_ws_bytes", 3, 8) == 512 and _lib.query("maavss_spectrum_metrics_ws_bytes", 0, 8) == 0
    sq = _lib.query("maavss_sqerr_rows_chunk")
    assert _lib.query("maavss_sqerr_rows_ws_bytes", 2, sq + 1) == 256 and _lib.query("maavss_sqerr_rows_ws_bytes", 2, 0) == 0


def test_new_symbols_are_exported_and_the_abi_version_is_still_401():
    import maavss_amd
    for name in ("Validator", "wave_metrics", "spectrum_metrics", "plan_wave_chunks", "quality"):
        assert hasattr(maavss_amd, name), name
    protos = _lib.parse_header()
    L = _lib.lib()
    for name in ("maavss_wave_metrics_chunk", "maavss_wave_metrics_ws_bytes", "maavss_wave_metrics", "maavss_spectrum_metrics_ws_bytes",
                 "maavss_spectrum_metrics", "maavss_sqerr_rows_chunk", "maavss_sqerr_rows_ws_bytes", "maavss_sqerr_rows",
                 "maavss_metric_add_sum", "maavss_metric_add_classes"):
        assert name in protos and hasattr(L.cdll, name), name
    assert _lib.header_abi_version() == 402 == L.cdll.maavss_version()
    sig = inspect.signature(maavss_amd.Validator.__init__).parameters
    assert (sig["loss_coeff"].default, sig["num_seq"].default, sig["seg_len"].default, sig["lsd_floor"].default) == (0.001, 1, 256, 1e-10)
    assert inspect.signature(maavss_amd.wave_metrics).parameters["seg_len"].default == 256
    assert inspect.signature(maavss_amd.spectrum_metrics).parameters["lsd_floor"].default == 1e-10


def _wave_args(**over):
    """A call of maavss_wave_metrics whose every argument passes (fake, aligned device addresses: never launched in these tests because
    one override makes a check fail)."""
    a = dict(est=4100, est_stride=50, ref=4104, ref_stride=3000, B=3, L=9000, seg_len=256, out=8192, ws=8192, ws_bytes=1 << 20, stream=None)
    a.update(over)
    return tuple(a[k] for k in ("est", "est_stride", "ref", "ref_stride", "B", "L", "seg_len", "out", "ws", "ws_bytes", "stream"))


@pytest.mark.parametrize("over,match", [
    (dict(est=None), "null pointer"),
    (dict(ref=None), "null pointer"),
    (dict(out=None), "null pointer"),
    (dict(ws=None), "null pointer"),
    (dict(B=0), "bad sizes"),
    (dict(L=0), "bad sizes"),
    (dict(L=-5), "bad sizes"),
    (dict(seg_len=0), "seg_len must be in 1..4096"),
    (dict(seg_len=CH + 1), "seg_len must be in 1..4096"),
    (dict(est_stride=-1), "rows would not be addressable"),
    (dict(ref_stride=-2500), "rows would not be addressable"),
    (dict(est=4101), "4-byte aligned"),
    (dict(out=8196), "8-byte aligned"),
    (dict(ws_bytes=64), "workspace of 64 bytes"),
])
def test_wave_metrics_refuses_bad_arguments_before_any_launch(over, match):
    with pytest.raises(_lib.MaavssError, match=match):
        _lib.call("maavss_wave_metrics", *_wave_args(**over))


def test_overlapping_rows_and_odd_offsets_pass_the_wave_metrics_checks():
    """stride < L (overlapping rows), stride 0 and a 4-byte-aligned offset are not refusals: with every pointer valid the call would
    launch, so the checks are shown to pass by the one that comes after them all."""
    for over in (dict(est_stride=50), dict(est_stride=0, ref_stride=0), dict(est=4100, ref=4108), dict(B=1, est_stride=-7, ref_stride=-7)):
        with pytest.raises(_lib.MaavssError, match="workspace of 8 bytes"):
            _lib.call("maavss_wave_metrics", *_wave_args(ws_bytes=8, **over))


@pytest.mark.parametrize("name,args,match", [
    ("maavss_spectrum_metrics", (None, 256, 1, 8, 257, 1e-10, 256, 256, 1 << 20, None), "null pointer"),
    ("maavss_spectrum_metrics", (256, 256, 0, 8, 257, 1e-10, 256, 256, 1 << 20, None), "bad sizes"),
    ("maavss_spectrum_metrics", (256, 256, 1, 8, 0, 1e-10, 256, 256, 1 << 20, None), "bad sizes"),
    ("maavss_spectrum_metrics", (256, 256, 1, 8, 257, 0.0, 256, 256, 1 << 20, None), "power floor must be positive"),
    ("maavss_spectrum_metrics", (256, 256, 1, 8, 257, -1e-10, 256, 256, 1 << 20, None), "power floor must be positive"),
    ("maavss_spectrum_metrics", (256, 256, 1, 8, 257, float("nan"), 256, 256, 1 << 20, None), "power floor must be positive"),
    ("maavss_spectrum_metrics", (256, 256, 1, 8, 257, 1e-10, 256, 256, 64, None), "workspace of 64 bytes"),
    ("maavss_sqerr_rows", (256, None, 2, 100, 256, 256, 1 << 20, None), "null pointer"),
    ("maavss_sqerr_rows", (256, 256, 2, 0, 256, 256, 1 << 20, None), "bad sizes"),
    ("maavss_sqerr_rows", (256, 258, 2, 100, 256, 256, 1 << 20, None), "4-byte aligned"),
    ("maavss_sqerr_rows", (256, 256, 2, 100, 256, 256, 8, None), "workspace of 8 bytes"),
    ("maavss_metric_add_sum", (None, 4, 1, 1.0, 256, None), "null pointer"),
    ("maavss_metric_add_sum", (256, 0, 1, 1.0, 256, None), "bad sizes"),
    ("maavss_metric_add_classes", (256, None, 4, 9, 3, None, None), "null pointer"),
    ("maavss_metric_add_classes", (256, None, 4, 2, 3, 256, None), "bad sizes"),
    ("maavss_metric_add_classes", (256, 260, 4, 9, 3, 256, None), "8-byte aligned"),
])
def test_other_entry_points_refuse_bad_arguments_before_any_launch(name, args, match):
    with pytest.raises(_lib.MaavssError, match=match):
        _lib.call(name, *args)


def test_validator_refuses_a_training_mode_model_and_cpu_tensors():
    import maavss_amd
    model = types.SimpleNamespace(training=True)
    val = maavss_amd.Validator(model)
    x = torch.zeros(1, 2, 8, 5)
    with pytest.raises(ValueError, match=r"training mode: call model.eval\(\) first"):
        val.add_windows(x, x, x, x)
    with pytest.raises(ValueError, match="training mode"):
        val.add_clips(x, x, x, x, 8, 8)
    with pytest.raises(ValueError, match="training mode"):
        val.add_recording(None, x, x, attn=x)
    model.training = False
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        val.add_windows(x, x, x, x)
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        val.add_waves(torch.zeros(2, 100), torch.zeros(2, 100))
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        maavss_amd.wave_metrics(torch.zeros(100), torch.zeros(100))
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        maavss_amd.spectrum_metrics(x, x)
    with pytest.raises(ValueError, match="seg_len must be in"):
        maavss_amd.wave_metrics(torch.zeros(100), torch.zeros(100), seg_len=CH + 1)
    with pytest.raises(ValueError, match="differ in shape"):
        maavss_amd.wave_metrics(torch.zeros(100), torch.zeros(99))
    with pytest.raises(ValueError, match="lsd_floor"):
        maavss_amd.spectrum_metrics(x, x, lsd_floor=0.0)
    # nothing was added: every quotient is NaN, every count zero, and a NaN loss is no improvement
    res = val.result()
    assert math.isnan(res["val_loss"]) and res["n_windows"] == 0 and res["n_clips"] == 0
    assert not val.improved(res)
    assert val.improved({"val_loss": 2.0}) and not val.improved({"val_loss": 2.0}) and val.improved({"val_loss": 1.5}) and val.best == 1.5


def test_nothing_in_quality_py_waits_for_the_device_before_result():
    """No synchronisation before Validator.result(): by structure, no .item() / .cpu() / .tolist() / synchronize in the module's code
    outside result()."""
    import maavss_amd.quality as q
    src = inspect.getsource(q)
    body = inspect.getsource(q.Validator.result)
    assert src.count(body) == 1
    rest = src.replace(body, "")
    pat = re.compile(r"\.item\(|\.cpu\(|\.tolist\(|\.numpy\(|synchronize|\.to\(")
    assert pat.search(body), "result() makes the one copy"
    assert len(re.findall(r"\.cpu\(", body)) == 1
    assert not pat.search(rest), pat.search(rest)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "validator_result.json")
OPTIONS = list(itertools.product((False, True), repeat=3))         # intelligibility_sr, bss_filter, audio_loss: on or off


def _validator(intel, bss, loss):
    import maavss_amd
    return maavss_amd.Validator(types.SimpleNamespace(training=False), loss_coeff=0.5, intelligibility_sr=16000 if intel else None,
                                bss_filter=32 if bss else None, audio_loss=maavss_amd.SpectralLoss(mix=0.25) if loss else None)


def known_buffer_results():
    """{"<intel><bss><loss>/<fill>": [[key, value], ...]}: result() of every option combination on a CPU buffer of 1, 2, ..., n and of
    zeros, in the order of its keys, a NaN as None.  tests/golden/validator_result.json holds what this returned at the commit
    before the Validator's family table (run there with that tree's package on the path); no library and no device is needed."""
    res = {}
    for opt in OPTIONS:
        for fill in ("arange", "zeros"):
            val = _validator(*opt)
            n = val._buf_len()
            val._buf = torch.arange(1, n + 1, dtype=torch.float64) if fill == "arange" else torch.zeros(n, dtype=torch.float64)
            out = val.result()
            res["%d%d%d/%s" % (*opt, fill)] = [[k, None if isinstance(v, float) and math.isnan(v) else v] for k, v in out.items()]
    return res


def test_result_of_a_known_buffer_is_what_it_was_before_the_family_table():
    want = json.load(open(GOLDEN))
    got = known_buffer_results()
    assert list(got) == list(want) and len(want) == 16
    for case in want:
        assert [k for k, _ in got[case]] == [k for k, _ in want[case]], case                       # the keys, in order
        for (k, a), (_, b) in zip(got[case], want[case]):
            assert type(a) is type(b) and a == b, (case, k, a, b)                                   # None stands for NaN; an int stays an int
    assert len(want["111/arange"]) == 118 and len(got["111/arange"]) == 118


# per family: the width of its raw tensor, the first accumulated column, the number of accumulated columns
FAMILY_SHAPE = {"wave": (9, 5, 3), "stoi": (4, 0, 2), "bss": (10, 5, 3)}


@pytest.mark.parametrize("with_noisy", (False, True))
@pytest.mark.parametrize("intel,bss,loss", OPTIONS)
def test_add_waves_enqueues_the_same_launches_in_the_same_order(monkeypatch, intel, bss, loss, with_noisy):
    import maavss_amd.quality as q
    B = 3
    est, ref, noisy, others = (torch.zeros(B, 64) for _ in range(4))
    log, made = [], {}

    def metric(family):
        def stub(x, r, *extra):
            assert r is ref and extra == {"wave": (256,), "stoi": (16000,), "bss": (others, 32)}[family]
            who = "est" if x is est else "noisy"
            assert x is (est if who == "est" else noisy)
            log.append(("metric", family, who))
            made[family, who] = torch.zeros(B, FAMILY_SHAPE[family][0], dtype=torch.float64)
            return {"raw": made[family, who]}
        return stub

    def where(p):
        """the tensor a pointer lies in, and its offset in f64 elements"""
        if p is None:
            return None
        for tag, t in list(made.items()) + [("acc", val._buf)]:
            if t.data_ptr() <= p < t.data_ptr() + 8 * t.numel():
                return tag, (p - t.data_ptr()) // 8
        raise AssertionError("a pointer into no known tensor")

    def call(name, vals, minus, rows, stride, cols, acc, stream):
        assert stream == 77
        log.append((name, where(vals), where(minus), rows, stride, cols, where(acc)))

    monkeypatch.setattr(q, "call", call)
    monkeypatch.setattr(q, "stream_ptr", lambda: 77)
    for family, name in (("wave", "wave_metrics"), ("stoi", "stoi_metrics"), ("bss", "bss_eval_metrics")):
        monkeypatch.setattr(q, name, metric(family))
    val = _validator(intel, bss, loss)
    val.add_waves(est, ref, noisy=noisy if with_noisy else None, others=others if bss else None)
    assert val._buf.shape == (51 + 30 * intel + 45 * bss + 3 * loss,) and val.acc.shape == (51,)

    # the first accumulator slot of each enabled family: after the six sums, then in the order wave, intelligibility, BSS
    first = {"wave": 6, "stoi": 51, "bss": 81 if intel else 51}
    want = []
    for family in ["wave"] + ["stoi"] * intel + ["bss"] * bss:
        width, col0, k = FAMILY_SHAPE[family]
        add = "maavss_metric_add_classes"
        want += [("metric", family, "est"),
                 (add, ((family, "est"), col0), None, B, width, k, ("acc", first[family]))]
        if with_noisy:
            want += [("metric", family, "noisy"),
                     (add, ((family, "noisy"), col0), None, B, width, k, ("acc", first[family] + 5 * k)),
                     (add, ((family, "est"), col0), ((family, "noisy"), col0), B, width, k, ("acc", first[family] + 10 * k))]
    assert log == want
