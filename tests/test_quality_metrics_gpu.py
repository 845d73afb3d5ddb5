"""csrc/quality_metrics.hip on the GPU against the float64 twin (tests/quality_twin.py, where the bounds are derived).

Wave metrics: row lengths 1, 63, 64, 65, around seg_len, around the chunk length and three chunks with a partial frame; seg_len 7 (eight
lanes per frame, eight frames per wave step) and 256 (a wave per frame); one and three rows; a row stride past the row, overlapping
rows, est and ref 1, 2 and 3 elements off a 16-byte boundary; a silent reference, est == ref, a NaN, an inf and an estimate 90 dB above
its error.  Spectrum metrics: F 1, 5, 129, 257 (under, at and past one wave of lanes), T 1 and 8 (frames across workgroups), bins under
the floor in one or both operands."""
import math

import numpy as np
import pytest
import torch

import maavss_amd
import quality_twin as tw
from maavss_amd import quality

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("seg_len", tw.SEG_LENS)
def test_wave_metrics_equal_the_twin(seg_len, b):
    ch = quality.wave_chunk()
    rng = np.random.default_rng(100 * seg_len + b)
    lengths = tw.wave_lengths(ch, seg_len)
    assert {1, 63, 64, 65, seg_len - 1, seg_len, seg_len + 1, ch - 1, ch, ch + 1, 2 * ch + seg_len // 2 + 3} <= set(lengths)
    for k, n in enumerate(lengths):
        pairs = [tw.make_wave(rng, n, "noisy") for _ in range(b)]
        est, ref = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        off_e, off_r = 1 + k % 3, 1 + (k + 1) % 3                    # 1, 2, 3 elements off a 16-byte boundary, never the same two
        got = _host(maavss_amd.wave_metrics(_place(est, n + 5, off_e), _place(ref, n + 9, off_r), seg_len)["raw"])
        assert got.shape == (b, 9)
        for i in range(b):
            tw.check_wave_row(got[i], tw.wave_row(est[i], ref[i], seg_len), n, label=f"seg {seg_len} B {b} L {n} row {i}:")


@pytest.mark.parametrize("seg_len", tw.SEG_LENS)
def test_wave_metrics_of_overlapping_rows_and_a_one_dimensional_slice(seg_len):
    ch = quality.wave_chunk()
    rng = np.random.default_rng(7 + seg_len)
    n, stride = ch + seg_len + 3, 100                                # rows overlap: stride < L
    ref_sig = (0.3 * rng.standard_normal(2 * stride + n + 3)).astype(np.float32)
    est_sig = (ref_sig + 0.05 * rng.standard_normal(ref_sig.size)).astype(np.float32)
    ref_dev, est_dev = torch.from_numpy(ref_sig).cuda(), torch.from_numpy(est_sig).cuda()
    ref_rows, est_rows = ref_dev.as_strided((3, n), (stride, 1), 3), est_dev.as_strided((3, n), (stride, 1), 1)
    got = _host(maavss_amd.wave_metrics(est_rows, ref_rows, seg_len)["raw"])
    for i in range(3):
        want = tw.wave_row(est_sig[1 + i * stride:1 + i * stride + n], ref_sig[3 + i * stride:3 + i * stride + n], seg_len)
        tw.check_wave_row(got[i], want, n, label=f"overlap seg {seg_len} row {i}:")
    # a plain slice at an arbitrary offset, as Validator.add_recording passes clean[start:start + n]
    res = maavss_amd.wave_metrics(est_dev[2:2 + n], ref_dev[2:2 + n], seg_len)
    assert res["snr_db"].shape == (1,) and res["snr_db"].dtype == torch.float64 and res["snr_db"].is_cuda
    tw.check_wave_row(_host(res["raw"])[0], tw.wave_row(est_sig[2:2 + n], ref_sig[2:2 + n], seg_len), n, label=f"slice seg {seg_len}:")


@pytest.mark.parametrize("seg_len", tw.SEG_LENS)
def test_wave_metrics_content_kinds(seg_len):
    ch = quality.wave_chunk()
    n = 2 * ch + seg_len // 2 + 3
    rng = np.random.default_rng(11)
    pairs = [tw.make_wave(rng, n, kind) for kind in tw.KINDS]
    est, ref = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    got = _host(maavss_amd.wave_metrics(torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda(), seg_len)["raw"])
    want = [tw.wave_row(est[i], ref[i], seg_len) for i in range(len(tw.KINDS))]
    for i, kind in enumerate(tw.KINDS):
        tw.check_wave_row(got[i], want[i], n, label=f"{kind} seg {seg_len}:")
    k = {kind: i for i, kind in enumerate(tw.KINDS)}
    snr, si, seg, frames = got[:, 5], got[:, 6], got[:, 7], got[:, 8]
    assert all(math.isnan(v[k["zeros_ref"]]) for v in (snr, si, seg)) and frames[k["zeros_ref"]] == 0
    assert snr[k["equal"]] == math.inf and si[k["equal"]] == math.inf and seg[k["equal"]] == 35.0 and frames[k["equal"]] == n // seg_len
    assert np.isnan(got[k["nan"], :8]).all() and np.isnan(got[k["inf"], :8]).all()
    hq = want[k["high_quality"]]
    assert 85.0 < hq["si_sdr_db"] < 95.0, "the case must sit where Syy - Sxy^2 / Sxx has lost its digits"
    cancelled = hq["syy"] - hq["sxy"] ** 2 / hq["sxx"]
    assert abs(cancelled - hq["srr"]) > 100 * ((n - 1) * tw.U53 * hq["srr"] + 4 * tw.U53 * math.sqrt(hq["syy"] * hq["srr"])), \
        "the cancelled form must miss the gate the kernel passes"


def test_two_runs_give_identical_bytes_and_a_long_row_is_right():
    g = torch.Generator(device="cuda").manual_seed(5)
    for b, n in ((1, 960000), (32, 8448)):
        ref = 0.3 * torch.randn(b, n, device="cuda", generator=g)
        est = ref + 0.03 * torch.randn(b, n, device="cuda", generator=g)
        first = maavss_amd.wave_metrics(est, ref)["raw"].clone()
        second = maavss_amd.wave_metrics(est, ref)["raw"]
        torch.cuda.synchronize()
        assert first.view(torch.int64).equal(second.view(torch.int64)), "two runs differ"
        # both sums are some order of f64 additions of the same non-negative terms: each within (n - 1) u S of the exact sum
        x, e = ref.double(), est.double() - ref.double()
        for col, t in ((0, x * x), (3, e * e)):
            want = t.sum(1)
            assert ((first[:, col] - want).abs() <= 2 * (n - 1) * tw.U53 * want).all(), col
        assert (first[:, 8] == n // 256).all()
    pred, tgt = torch.randn(3, 2, 8, 257, device="cuda", generator=g), torch.randn(3, 2, 8, 257, device="cuda", generator=g)
    first = maavss_amd.spectrum_metrics(pred, tgt)["raw"].clone()
    second = maavss_amd.spectrum_metrics(pred, tgt)["raw"]
    torch.cuda.synchronize()
    assert first.view(torch.int64).equal(second.view(torch.int64))


def _spectrum_case(rng, b, t, f):
    """normal values; every third bin of tgt and every fourth of pred scaled under the floor (both in every twelfth)"""
    pred = rng.standard_normal((b, 2, t, f)).astype(np.float32)
    tgt = (pred + 0.2 * rng.standard_normal((b, 2, t, f))).astype(np.float32)
    tgt[..., ::3] *= np.float32(1e-7)
    pred[..., ::4] *= np.float32(1e-7)
    return pred, tgt


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("t", [1, 8])
@pytest.mark.parametrize("f", [1, 5, 129, 257])
def test_spectrum_metrics_equal_the_twin(f, t, b):
    rng = np.random.default_rng(1000 * f + 10 * t + b)
    pred, tgt = _spectrum_case(rng, b, t, f)
    p64 = pred.astype(np.float64)
    power = p64[:, 0] ** 2 + p64[:, 1] ** 2
    assert (power < 1e-10).any() and (f < 5 or (power > 1e-10).any())
    res = maavss_amd.spectrum_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda())
    got = _host(res["raw"])
    n = 2 * t * f
    for i in range(b):
        want = tw.spectrum_row(pred[i], tgt[i])
        err, bound = abs(got[i, 0] - want["sqerr"]), (n - 1) * tw.U53 * want["sqerr"]
        print(f"F {f} T {t} row {i}: sqerr {got[i, 0]:.17g} |err| {err:.3g} bound {bound:.3g}; lsd {got[i, 1]!r} twin {want['lsd_db']!r}")
        assert err <= bound
        assert abs(got[i, 1] - want["lsd_db"]) <= tw.LSD_TOL
    # another floor moves the floored bins only
    got2 = _host(maavss_amd.spectrum_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda(), lsd_floor=1e-6)["raw"])
    for i in range(b):
        assert abs(got2[i, 1] - tw.spectrum_row(pred[i], tgt[i], 1e-6)["lsd_db"]) <= tw.LSD_TOL and got2[i, 0] == got[i, 0]


def test_spectrum_metrics_keep_a_nan():
    pred = torch.randn(2, 2, 3, 5, device="cuda")
    tgt = pred.clone()
    pred[1, 0, 2, 4] = float("nan")
    got = _host(maavss_amd.spectrum_metrics(pred, tgt)["raw"])
    assert got[0, 0] == 0.0 and got[0, 1] == 0.0 and np.isnan(got[1]).all()


@pytest.mark.parametrize("b", [1, 3])
def test_squared_error_rows_equal_the_twin(b):
    sq = int(maavss_amd._lib.query("maavss_sqerr_rows_chunk"))
    rng = np.random.default_rng(b)
    # 63 .. 65 and 255 .. 257: an empty wave, a partly filled fourth wave; around sq: the last short chunk (the kernel is pass 2's, without alpha)
    for n in (1, 63, 64, 65, 255, 256, 257, sq - 1, sq, sq + 1, 2 * sq + 3, 2 * sq + 5):
        pred = rng.standard_normal((b, n)).astype(np.float32)
        tgt = (pred + 0.1 * rng.standard_normal((b, n))).astype(np.float32)
        got = _host(quality.sqerr_rows(torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda()))
        for i in range(b):
            d = pred[i].astype(np.float64) - tgt[i].astype(np.float64)
            want = math.fsum((d * d).tolist())
            assert abs(got[i] - want) <= (n - 1) * tw.U53 * want, (n, i, got[i], want)


def test_validator_counts_the_classes_of_the_wave_metrics_exactly():
    n, seg = 1500, 256
    rng = np.random.default_rng(21)
    pairs = [tw.make_wave(rng, n, kind) for kind in ("noisy", "equal", "zeros_ref", "nan")]
    ones = np.ones(n, dtype=np.float32)
    pairs.append((ones * np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.float32), ones))        # est orthogonal to ref
    est, ref = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want = [tw.wave_row(est[i], ref[i], seg) for i in range(5)]
    assert want[4]["si_sdr_db"] == -math.inf
    val = maavss_amd.Validator(None, seg_len=seg)
    val.add_waves(torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda())
    val.add_waves(torch.from_numpy(est[:2]).cuda(), torch.from_numpy(ref[:2]).cuda())              # the accumulator adds up
    res = val.result()
    rows = list(range(5)) + [0, 1]
    assert res["n_clips"] == 7 and res["n_windows"] == 0 and math.isnan(res["val_loss"])
    for name in ("snr_db", "si_sdr_db", "seg_snr_db"):
        vals = [want[i][name] for i in rows]
        for kl in ("finite", "posinf", "neginf", "nan"):
            assert res[f"{name}_n_{kl}"] == sum(tw.klass(v) == kl for v in vals), (name, kl)
        fin = [v for v in vals if tw.klass(v) == "finite"]
        assert abs(res[name] - math.fsum(fin) / len(fin)) <= tw.DB_TOL, name
    assert "noisy_snr_db" not in res and "snr_db_improvement" not in res
    val.reset()
    assert val.result()["n_clips"] == 0
