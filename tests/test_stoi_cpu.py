"""CPU-only part of the intelligibility scores (maavss_amd/stoi.py, csrc/stoi.hip): known answers of the float64 twin
(tests/stoi_twin.py), what makes the GPU comparison mean something (every GPU case far from the 40 dB mask decision, and an indexing
error of one bin or one sample visible in the twin's scores), the wrappers' refusals, the Validator's keys with and without the option,
and the argument checks of the entry points (every call below fails before any launch)."""
import inspect
import math
import types

import numpy as np
import pytest
import torch

import stoi_twin as tw
from maavss_amd import _lib

SNRS = (math.inf, 20.0, 10.0, 0.0, -10.0)

# the keys of Validator.result() before intelligibility_sr existed, with nothing added (noisy_* and *_improvement appear with data only)
KEYS_BEFORE = {"val_loss_stft", "lsd_db", "val_loss_attn", "n_windows", "val_loss", "n_clips"} | {
    name + suffix for name in ("snr_db", "si_sdr_db", "seg_snr_db") for suffix in ("", "_n_finite", "_n_posinf", "_n_neginf", "_n_nan")}
KEYS_NEW = {key + suffix for key in ("stoi", "estoi", "noisy_stoi", "noisy_estoi", "stoi_improvement", "estoi_improvement")
            for suffix in ("", "_n_finite", "_n_nan")}


@pytest.fixture(scope="module")
def gpu_rows():
    """every finite row the GPU test compares at 10 kHz, with the twin's result: [(label, est, ref, result)]"""
    rows = []
    for name, _, _ in tw.GPU_CASES:
        est, ref = tw.gpu_case(name)
        rows.append((name, est, ref))
    est, ref = tw.overlap_rows()
    rows += [(f"overlap{i}", est[i], ref[i]) for i in range(est.shape[0])]
    est, ref, kinds = tw.bad_rows()
    rows += [(f"bad{i}_{k}", est[i], ref[i]) for i, k in enumerate(kinds)]
    for b, (est, ref, noisy) in enumerate(tw.validator_batches()):
        rows += [(f"validator{b}_{i}", est[i], ref[i]) for i in range(est.shape[0])]
        rows += [(f"validator{b}_{i}_noisy", noisy[i], ref[i]) for i in range(est.shape[0])]
    return [(label, est, ref, tw.stoi_row(est, ref)) for label, est, ref in rows]


def test_band_edges_are_the_table_of_the_header():
    assert tw.LO == [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
    assert tw.HI == tw.LO[1:] + [219]
    assert np.abs(tw.W - np.hanning(258)[1:-1]).max() <= 8 * tw.EPS and tw.W.shape == (256,)
    assert tw.CLIP == 1.0 + 10.0 ** 0.75 == float.fromhex("0x1.a7e600b234626p+2")            # the constant csrc/stoi.hip spells out


def test_frame_and_segment_counts():
    assert [tw.nframes(n) for n in (1, 255, 256, 257, 384, 385, 4096, 4097, 4224, 4225, 5280, 30000)] == [0, 0, 0, 1, 1, 2, 30, 31, 31, 32, 40, 233]
    want = {"L255": (0, 0), "L256": (0, 0), "L257": (1, 0), "L4096": (30, 0), "L4097": (31, 1), "L4224": (31, 1), "L4225": (32, 2),
            "L5280": (40, 10), "L30000": (233, 203), "silent_too_much": (29, 0)}
    for name, (n_kept, n_seg) in want.items():
        r = tw.stoi_row(*tw.gpu_case(name))
        assert (r["n_kept"], r["n_segments"]) == (n_kept, n_seg), name
        assert math.isnan(r["stoi"]) == math.isnan(r["estoi"]) == (n_seg == 0), name
    # silence removes frames: fewer are kept than the row has, at the start, at the end and in the middle
    for name in ("silent_start", "silent_end", "silent_middle"):
        r = tw.stoi_row(*tw.gpu_case(name))
        assert 31 <= r["n_kept"] < tw.nframes(6000) == 45 and r["n_segments"] == r["n_kept"] - 30, (name, r)
    assert len({tw.stoi_row(*tw.gpu_case(name))["n_kept"] for name in tw.BATCH}) == 3, "the batch's rows must keep different frame counts"


def test_known_answers_equal_negated_and_zero_estimates():
    _, ref = tw.make_case(1, 8000, None)
    same, neg, zero = tw.stoi_row(ref, ref), tw.stoi_row(-ref, ref), tw.stoi_row(np.zeros_like(ref), ref)
    assert abs(same["stoi"] - 1.0) <= 1e-12 and abs(same["estoi"] - 1.0) <= 1e-12
    assert neg == same, "the measure is on magnitudes"
    assert zero["stoi"] == 0.0 and zero["estoi"] == 0.0 and zero["n_segments"] == same["n_segments"] > 0


def test_silent_reference_and_non_finite_samples_give_nan():
    est, ref = tw.make_case(2, 5280, 5.0)
    r = tw.stoi_row(est, np.zeros_like(ref))
    assert math.isnan(r["stoi"]) and math.isnan(r["estoi"]) and r["n_kept"] == 0 and r["n_segments"] == 0
    for bad in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            pair = [est.copy(), ref.copy()]
            pair[which][-1] = bad                              # past the last frame: still a non-finite sample of the row
            r = tw.stoi_row(*pair)
            assert math.isnan(r["stoi"]) and math.isnan(r["estoi"]) and r["n_kept"] == 0 and r["n_segments"] == 0


def test_scores_fall_monotonically_with_the_snr():
    rows = [tw.stoi_row(*tw.make_case(1, 30000, snr)) for snr in SNRS]
    for key in ("stoi", "estoi"):
        vals = [r[key] for r in rows]
        print(key, vals)
        assert all(a > b for a, b in zip(vals, vals[1:])), (key, vals)
        assert abs(vals[0] - 1.0) <= 1e-12 and vals[-1] < 0.3


def test_every_gpu_case_is_far_from_the_mask_decision():
    """The kernels sum E[k] in another order than the twin: a frame within rounding of the 40 dB threshold could fall either way.
    No case has one within 1e-6 dB (rounding is some 1e-14 dB)."""
    for name, refs in tw.all_gpu_refs().items():
        for i, ref in enumerate(refs):
            if np.isfinite(ref).all():
                m = tw.margin_db(ref)
                print(name, i, m)
                assert m >= 1e-6, (name, i, m)


def test_an_indexing_error_shows_in_the_twins_scores(gpu_rows):
    """So that the GPU gate (at most 1e-9) means something: band edges off by one bin, or est off by one sample, move both scores of
    every finite GPU case by more than 1e-6."""
    seen = 0
    for label, est, ref, want in gpu_rows:
        if want["n_segments"] == 0:
            continue
        seen += 1
        for what, other in (("bands + 1", tw.stoi_row(est, ref, band_shift=1)), ("bands - 1", tw.stoi_row(est, ref, band_shift=-1)),
                            ("est shifted", tw.stoi_row(np.roll(est, 1), ref))):
            for key in ("stoi", "estoi"):
                d = abs(other[key] - want[key])
                print(f"{label}: {what}: {key} moves by {d:.3g}")
                assert d > 1e-6, (label, what, key, d)
    assert seen >= 20


def test_wrappers_refuse_bad_arguments_before_the_device_is_touched():
    import maavss_amd
    assert maavss_amd.stoi_metrics is maavss_amd.stoi.stoi_metrics
    assert inspect.signature(maavss_amd.stoi_metrics).parameters["sr"].default == 10000
    x = torch.zeros(2, 5280)
    with pytest.raises(ValueError, match="float32 tensor"):
        maavss_amd.stoi_metrics(x.double(), x.double())
    with pytest.raises(ValueError, match="float32 tensor"):
        maavss_amd.stoi_metrics(x[None], x[None])
    with pytest.raises(ValueError, match="float32 tensor"):
        maavss_amd.stoi_metrics([0.0], [0.0])
    with pytest.raises(ValueError, match="is empty"):
        maavss_amd.stoi_metrics(x[:, :0], x[:, :0])
    with pytest.raises(ValueError, match="differ in shape"):
        maavss_amd.stoi_metrics(x, x[:, :-1])
    for sr in (0, -10000, 10000.0, True, None):
        with pytest.raises(ValueError, match="sr must be a positive integer"):
            maavss_amd.stoi_metrics(x, x, sr=sr)
    for sr in (10000, 16000):
        with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
            maavss_amd.stoi_metrics(x, x, sr=sr)
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        maavss_amd.stoi_metrics(x[0], x[0])
    for bad in (0, -1, 16000.0, True):
        with pytest.raises(ValueError, match="intelligibility_sr"):
            maavss_amd.Validator(None, intelligibility_sr=bad)
    val = maavss_amd.Validator(types.SimpleNamespace(training=False), intelligibility_sr=10000)
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        val.add_waves(x, x)


def test_validator_keys_without_and_with_the_option():
    import maavss_amd
    model = types.SimpleNamespace(training=False)
    sig = inspect.signature(maavss_amd.Validator.__init__).parameters
    assert sig["intelligibility_sr"].default is None
    res = maavss_amd.Validator(model).result()
    assert set(res) == KEYS_BEFORE, sorted(set(res) ^ KEYS_BEFORE)
    val = maavss_amd.Validator(model, intelligibility_sr=16000)
    res = val.result()
    assert set(res) == KEYS_BEFORE | KEYS_NEW, sorted(set(res) ^ (KEYS_BEFORE | KEYS_NEW))
    for key in KEYS_NEW:
        if key.endswith(("_n_finite", "_n_nan")):
            assert res[key] == 0, key
        else:
            assert math.isnan(res[key]), key
    assert val.acc is None and val.acc_intel is None, "no device memory before the first add"


def test_nothing_in_stoi_py_waits_for_the_device():
    """stoi_metrics only enqueues: by structure, no .item() / .cpu() / .tolist() / synchronize / .to() in the module (quality.py, where
    the Validator's one copy lives, is held to the same by tests/test_quality_metrics_cpu.py)."""
    import re
    import maavss_amd.stoi as st
    found = re.search(r"\.item\(|\.cpu\(|\.tolist\(|\.numpy\(|synchronize|\.to\(", inspect.getsource(st))
    assert not found, found


def test_new_symbols_are_in_the_header_and_the_library_and_the_abi_version_is_still_401():
    protos = _lib.parse_header()
    L = _lib.lib()
    for name in ("maavss_stoi_ws_bytes", "maavss_stoi"):
        assert name in protos and hasattr(L.cdll, name), name
    assert [n for _, n in protos["maavss_stoi"][1]] == ["est", "est_stride", "ref", "ref_stride", "rows", "n", "out", "ws", "ws_bytes", "stream"]
    assert _lib.header_abi_version() == 402 == L.cdll.maavss_version()


def _round256(b):
    return -(-b // 256) * 256


def test_workspace_query():
    for bad in ((0, 5280), (-1, 5280), (1, 0), (1, -3), (1, 1 << 31), (1 << 31, 5280)):
        assert _lib.query("maavss_stoi_ws_bytes", *bad) == 0, bad
    for rows, n in ((1, 1), (1, 256), (3, 257), (2, 4096), (2, 4097), (32, 5280), (1, 600000)):
        nf = tw.nframes(n)
        nfc, mcap = max(nf, 1), max(nf - 1, 0)
        scap = max(mcap - 29, 0)
        want = (_round256(8 * 768) + _round256(8 * rows * nfc) + 2 * _round256(4 * rows * nfc) + _round256(8 * rows)
                + _round256(8 * rows * 30 * mcap) + _round256(16 * rows * scap))
        assert _lib.query("maavss_stoi_ws_bytes", rows, n) == want, (rows, n)
    assert _lib.query("maavss_stoi_ws_bytes", 1, (1 << 31) - 1) > 0


def _args(**over):
    """A call of maavss_stoi whose every argument passes (fake, aligned device addresses: never launched in these tests because one
    override makes a check fail)."""
    a = dict(est=4100, est_stride=50, ref=4104, ref_stride=6000, rows=3, n=5280, out=8192, ws=8192, ws_bytes=1 << 24, stream=None)
    a.update(over)
    return tuple(a[k] for k in ("est", "est_stride", "ref", "ref_stride", "rows", "n", "out", "ws", "ws_bytes", "stream"))


@pytest.mark.parametrize("over,match", [
    (dict(est=None), "stoi: null pointer"),
    (dict(ref=None), "stoi: null pointer"),
    (dict(out=None), "stoi: null pointer"),
    (dict(ws=None), "stoi: null pointer"),
    (dict(rows=0), "stoi: bad sizes"),
    (dict(rows=-2), "stoi: bad sizes"),
    (dict(n=0), "stoi: bad sizes"),
    (dict(n=-5), "stoi: bad sizes"),
    (dict(n=1 << 31), "stoi: n = 2147483648 is beyond the kernels' index range"),
    (dict(rows=1 << 20, n=1 << 30), "stoi: .* more workgroups than one launch takes"),
    (dict(est_stride=-1), "stoi: row strides .* rows would not be addressable"),
    (dict(ref_stride=-2500), "stoi: row strides .* rows would not be addressable"),
    (dict(est=4101), "stoi: est and ref must be 4-byte aligned"),
    (dict(ref=4106), "stoi: est and ref must be 4-byte aligned"),
    (dict(out=8196), "stoi: out and workspace must be 8-byte aligned"),
    (dict(ws=8196), "stoi: out and workspace must be 8-byte aligned"),
    (dict(ws_bytes=64), "stoi: workspace of 64 bytes"),
    (dict(ws_bytes=0), "stoi: workspace of 0 bytes"),
])
def test_stoi_refuses_bad_arguments_before_any_launch(over, match):
    with pytest.raises(_lib.MaavssError, match=match):
        _lib.call("maavss_stoi", *_args(**over))


def test_overlapping_rows_and_odd_offsets_pass_the_checks():
    """stride < n (overlapping rows), stride 0, a 4-byte-aligned offset and any stride with one row are not refusals: with every pointer
    valid the call would launch, so the checks are shown to pass by the one that comes after them all."""
    for over in (dict(est_stride=50), dict(est_stride=0, ref_stride=0), dict(est=4100, ref=4108), dict(rows=1, est_stride=-7, ref_stride=-7)):
        with pytest.raises(_lib.MaavssError, match="stoi: workspace of 8 bytes"):
            _lib.call("maavss_stoi", *_args(ws_bytes=8, **over))
