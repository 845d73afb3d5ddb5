"""What can be held without a GPU about the BSS-eval scores (csrc/bss_eval.hip, maavss_amd/bss.py): the float64 twin (tests/bss_twin.py)
against an independent formulation, the conditions the GPU cases have to meet for the GPU gate to mean something, the smallest score
change an off-by-one error makes on them (the ceiling of that gate), every refusal, the ABI, and the Validator without the option."""
import importlib.util
import inspect
import math
import os
import types

import numpy as np
import pytest
import scipy.linalg
import scipy.signal
import torch

import bss_twin as tw
from maavss_amd import _lib

EPS = 2.0 ** -52
COND_MAX = 1e6


def all_rows():
    """label -> (est, ref, others [K, n], L): every row the GPU test compares without a status"""
    rows = {name: tw.gpu_case(name) + (tw.case_filter(name),) for name, *_ in tw.GPU_CASES}
    est, ref, oth = tw.batch_rows()
    rows.update({f"batch{i}": (est[i], ref[i], oth[i], tw.BATCH["filt_len"]) for i in range(3)})
    est, ref, oth = tw.overlap_rows()
    rows.update({f"overlap{i}": (est[i], ref[i], oth[i], tw.OVERLAP["filt_len"]) for i in range(3)})
    est, ref, oth, kinds = tw.bad_rows()
    rows.update({f"bad{i}": (est[i], ref[i], oth[i], 33) for i, kind in enumerate(kinds) if kind == "fine"})
    rows.update({f"many{i}": tw.many_row(i) + (tw.MANY["filt_len"],) for i in tw.MANY["checked"]})
    est, ref, oth = tw.clip_batch()
    rows.update({f"clip{i}": (est[i], ref[i], oth[i], tw.CLIP_BATCH["filt_len"]) for i in tw.CLIP_BATCH["checked"]})
    for b, (est, ref, noisy, oth) in enumerate(tw.validator_batches()):
        for i in range(est.shape[0]):
            if np.isfinite(est[i]).all():
                rows[f"validator{b}_{i}"] = (est[i], ref[i], oth[i], tw.VALIDATOR_FILTER)
            rows[f"validator{b}_{i}_noisy"] = (noisy[i], ref[i], oth[i], tw.VALIDATOR_FILTER)
    return rows


def _corr(a, b, n_lags):
    """r[d] = sum_m a[m] b[m + d] for d in -(n_lags - 1) .. n_lags - 1 -> (r[0:], r[0], r[-1], ...): the non-negative and non-positive lags"""
    n = a.shape[0]
    full = scipy.signal.correlate(b, a, mode="full")
    return full[n - 1:n - 1 + n_lags], full[n - 1::-1][:n_lags]


def independent_row(est, ref, others, filt_len):
    """The same definition by another route: scipy.signal.correlate for the lags, scipy.linalg.toeplitz blocks for the Gram matrix,
    numpy.linalg.solve (LU) for the coefficients, numpy.convolve for the projections."""
    live = tw.live_sources(ref, others)
    e = np.asarray(est, dtype=np.float64)
    ez = np.concatenate([e, np.zeros(filt_len - 1)])

    def project(srcs):
        g = np.block([[scipy.linalg.toeplitz(*_corr(a, b, filt_len)) for b in srcs] for a in srcs])
        rhs = np.concatenate([_corr(a, e, filt_len)[0] for a in srcs])
        c = np.linalg.solve(g, rhs)
        return sum(np.convolve(s, c[j * filt_len:(j + 1) * filt_len]) for j, s in enumerate(srcs))

    p_t = project(live[:1])
    p = project(live) if len(live) > 1 else p_t
    s_tt, s_ee, s_ii = float((p_t ** 2).sum()), float(((ez - p_t) ** 2).sum()), float(((p - p_t) ** 2).sum())
    s_aa, s_pp = float(((ez - p) ** 2).sum()), float((p ** 2).sum())
    return dict(sdr_db=tw._db(s_tt, s_ee), sir_db=tw._db(s_tt, s_ii), sar_db=tw._db(s_pp, s_aa))


def test_lag_matrix_and_known_answers():
    a = tw.lag_matrix(np.array([1.0, 2.0, 3.0]), 2)
    assert a.tolist() == [[1, 0], [2, 1], [3, 2], [0, 3]]
    rng = np.random.default_rng(1)
    s, o = rng.standard_normal(400).astype(np.float32), rng.standard_normal(400).astype(np.float32)
    # a filtered target alone is all target: no distortion within rounding; with the other source added, all of the error is interference
    s[-8:] = 0.0                                # so that the filtered target ends inside the row, as its projection may not be cut off
    h = np.array([0.7, -0.2, 0.1])
    filt = np.convolve(s.astype(np.float64), h)[:400]
    r = tw.bss_row((filt + 0.5 * o).astype(np.float32), s, [o], 8)
    assert r["status"] == 0 and r["n_sources"] == 2 and r["sar_db"] > 100 and 0 < r["sir_db"] < 20 and abs(r["sdr_db"] - r["sir_db"]) < 1e-3
    # SI-SDR punishes the same short filter on the target; the projection forgives it
    r = tw.bss_row(filt.astype(np.float32), s, [], 8)
    assert r["sdr_db"] > 100 and r["sir_db"] == math.inf and r["n_sources"] == 1
    alpha = float(filt @ s) / float(s.astype(np.float64) @ s)
    assert 10 * math.log10((alpha * alpha * float(s.astype(np.float64) @ s)) / float(((filt - alpha * s) ** 2).sum())) < 15


def test_one_live_source_and_the_statuses():
    est, ref, oth = tw.make_case(5, 8, 200, 2, (0, 1))
    r = tw.bss_row(est, ref, oth, 8)
    assert r["n_sources"] == 1 and r["status"] == 0 and r["s_ii"] == 0.0 and r["sir_db"] == math.inf
    assert np.float64(r["sar_db"]).tobytes() == np.float64(r["sdr_db"]).tobytes()
    assert r == tw.bss_row(est, ref, [], 8)                              # an all-zero source is left out exactly
    bad = est.copy()
    bad[7] = np.inf
    for row in (tw.bss_row(bad, ref, oth, 8), tw.bss_row(est, ref, [bad], 8)):
        assert row["status"] == 1 and row["n_sources"] == 0 and all(math.isnan(row[k]) for k in tw.SUMS + tw.SCORES)
    row = tw.bss_row(est, np.zeros_like(ref), oth, 8)
    assert row["status"] == 2 and math.isnan(row["sdr_db"])
    assert tw.bss_row(bad, np.zeros_like(ref), oth, 8)["status"] == 1      # a non-finite sample comes first
    row = tw.bss_row(est, ref, [np.zeros_like(ref), -ref], 8)            # a rank-deficient Gram matrix: whatever the arithmetic gives
    assert row["status"] in (0, 3) and row["n_sources"] == 2


def test_the_twin_equals_an_independent_formulation():
    """Both are float64; what separates them is the solver (Cholesky against LU), the order of the correlation sums and an FFT in scipy's
    correlate for the long rows.  First-order bound: a relative coefficient error of cond eps = 1e6 x 2.2e-16 moves a projection by as
    much, a ratio of sums by a few times that, a score by 4.34 dB times it: 1e-9 dB (the residual is stationary at the least-squares
    solution, so what is seen is far smaller)."""
    worst = 0.0
    for label, (est, ref, oth, filt_len) in all_rows().items():
        want, got = tw.bss_row(est, ref, oth, filt_len), independent_row(est, ref, oth, filt_len)
        for key in tw.SCORES:
            if math.isfinite(want[key]):
                d = abs(want[key] - got[key])
                worst = max(worst, d)
                assert d <= 1e-9, (label, key, want[key], got[key])
            else:
                assert want[key] == got[key] == math.inf and key == "sir_db"
    print(f"largest |twin - independent| {worst:.3g} dB")


def test_every_gpu_case_is_well_conditioned_and_scores_in_range():
    """The GPU gate compares two f64 computations with different summation orders: that is only a statement about the kernels when the
    Gram matrix is well conditioned (<= 1e6), the scores are not rounding residue ([-30, 80] dB) and no pivot comes near 0."""
    for label, (est, ref, oth, filt_len) in all_rows().items():
        g = tw.gram(ref, oth, filt_len)
        ev = np.linalg.eigvalsh(g)
        cond = ev[-1] / ev[0]
        piv = np.diag(np.linalg.cholesky(g)) ** 2
        row = tw.bss_row(est, ref, oth, filt_len)
        print(f"{label}: {g.shape[0]} unknowns, cond {cond:.3g}, smallest pivot / largest diagonal {piv.min() / np.diag(g).max():.3g}, "
              f"sdr {row['sdr_db']:.2f} sir {row['sir_db']:.2f} sar {row['sar_db']:.2f}")
        assert ev[0] > 0 and cond <= COND_MAX, (label, cond)
        assert piv.min() / np.diag(g).max() >= 1.0 / COND_MAX, label
        assert row["status"] == 0
        for key in tw.SCORES:
            assert -30.0 <= row[key] <= 80.0 or (row[key] == math.inf and key == "sir_db" and row["n_sources"] == 1), (label, key, row[key])
    assert tw.gram(*tw.gpu_case("L512_limit")[1:], 512).shape == (2048, 2048)


def off_by_one_sensitivity():
    """-> (the smallest |change| in dB of any finite score of any GPU case when the filter is one tap shorter, the target one sample late
    or the first other source one sample late, where).  sdr_db is a function of the estimate and the target alone, so a late other source
    is looked for in sir_db and sar_db only."""
    smallest, where = math.inf, None
    for name, filt_len, n, k, zero, _ in tw.GPU_CASES:
        est, ref, oth = tw.gpu_case(name)
        base = tw.gpu_case_want(name)
        late = lambda s: np.concatenate([np.zeros(1, dtype=s.dtype), s[:-1]])
        variants = {"target one sample late": tw.bss_row(est, late(ref), oth, filt_len)}
        if filt_len > 1:
            variants["filter one tap shorter"] = tw.bss_row(est, ref, oth, filt_len - 1)
        if k > 0:
            variants["other source one sample late"] = tw.bss_row(est, ref, [late(oth[0])] + list(oth[1:]), filt_len)
        for what, row in variants.items():
            for key in tw.SCORES:
                if math.isfinite(base[key]) and not (key == "sdr_db" and what == "other source one sample late"):
                    d = abs(row[key] - base[key])
                    if d < smallest:
                        smallest, where = d, f"{name}, {what}, {key}"
    return smallest, where


def _gpu_test_module():
    spec = importlib.util.spec_from_file_location("test_bss_gpu_constants", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_bss_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_off_by_one_sensitivity_sets_the_ceiling_of_the_gpu_gate():
    smallest, where = off_by_one_sensitivity()
    print(f"smallest score change of an off-by-one error: {smallest:.3g} dB ({where}); a thousandth of it: {smallest / 1000:.3g}")
    g = _gpu_test_module()
    assert smallest > 0
    assert g.CEILING <= smallest / 1000.0, "the ceiling named in tests/test_bss_gpu.py is not under a thousandth of the sensitivity"
    assert g.GATE <= g.CEILING
    assert 8.0 * g.MEASURED_MAX <= g.GATE < 80.0 * g.MEASURED_MAX and abs(math.log10(g.GATE) - round(math.log10(g.GATE))) < 1e-9


def test_wrapper_refuses_bad_arguments_before_the_device_is_touched():
    import maavss_amd
    assert maavss_amd.bss_eval_metrics is maavss_amd.bss.bss_eval_metrics
    sig = inspect.signature(maavss_amd.bss_eval_metrics).parameters
    assert list(sig) == ["est", "ref", "others", "filt_len"] and sig["filt_len"].default == 512 and sig["others"].default is None
    x = torch.zeros(2, 2048)                    # CPU tensors: a call that got past the checks would raise MaavssError, not ValueError
    bad = [
        dict(filt_len=0), dict(filt_len=513), dict(filt_len=-1), dict(filt_len=2.0), dict(filt_len=True),
        dict(others=torch.zeros(2, 4, 2048), filt_len=8),                # K = 4
        dict(est=torch.zeros(2, 1023), ref=torch.zeros(2, 1023), others=torch.zeros(2, 1023)),         # N = 1023 < 2 x 512
        dict(filt_len=512, others=torch.zeros(2, 3, 2048)[:, :, :2047]), # length mismatch
        dict(others=torch.zeros(3, 2048), filt_len=8), dict(others=torch.zeros(2, 2048, dtype=torch.float64), filt_len=8),
        dict(others=torch.zeros(2048), filt_len=8), dict(others=np.zeros((2, 2048), dtype=np.float32), filt_len=8),
        dict(ref=torch.zeros(2, 2047), filt_len=8), dict(ref=torch.zeros(2, 2048, dtype=torch.float64), filt_len=8),
        dict(est=torch.zeros(2, 2048, dtype=torch.float16), filt_len=8), dict(est=torch.zeros(2, 2, 2048), filt_len=8),
        dict(est=torch.zeros(0, 2048), ref=torch.zeros(0, 2048), filt_len=8),
    ]
    for over in bad:
        args = dict(est=x, ref=x, others=None, filt_len=512)
        args.update(over)
        with pytest.raises(ValueError):
            maavss_amd.bss_eval_metrics(**args)
    with pytest.raises(ValueError, match="fewer than"):
        maavss_amd.bss_eval_metrics(torch.zeros(511), torch.zeros(511))
    with pytest.raises(_lib.MaavssError, match="MI355X only"):           # every check passed: N = (K + 1) L exactly, K = 3, L = 512
        maavss_amd.bss_eval_metrics(x, x, torch.zeros(2, 3, 2048), 512)


def test_library_refuses_bad_arguments_before_any_launch():
    ok = dict(est=4096, est_stride=700, ref=8192, ref_stride=700, others=12288, others_row_stride=1400, others_src_stride=700, K=2, rows=2,
              n=700, L=33, out=4096, ws=8192, ws_bytes=1 << 40, stream=None)
    for over, match in ((dict(est=None), "null"), (dict(others=None), "no other sources"), (dict(K=4), "K = 4"), (dict(K=-1), "K = -1"),
                        (dict(L=0), "filter length"), (dict(L=513), "filter length"), (dict(n=98), "fewer than"), (dict(rows=0), "rows"),
                        (dict(rows=65536), "rows"), (dict(n=1 << 31), "index range"), (dict(est_stride=-1), "strides"),
                        (dict(others_row_stride=-1), "strides"), (dict(others_src_stride=-1), "source stride"), (dict(est=4098), "4-byte"),
                        (dict(others=12290), "4-byte"), (dict(out=4100), "8-byte"), (dict(ws_bytes=1000), "workspace of 1000 bytes")):
        args = dict(ok)
        args.update(over)
        with pytest.raises(_lib.MaavssError, match=match):
            _lib.call("maavss_bss_eval", *args.values())
    for badq in ((0, 700, 1, 33), (1, 65, 1, 33), (1, 700, 4, 33), (1, 700, 1, 0), (1, 700, 1, 513), (1, 1 << 31, 1, 33), (65536, 700, 1, 33)):
        assert _lib.query("maavss_bss_eval_ws_bytes", *badq) == 0, badq
    one, two = (_lib.query("maavss_bss_eval_ws_bytes", r, 8448, 1, 512) for r in (1, 2))
    assert 1088 * 1024 * 8 < one < 1088 * 1024 * 8 + (1 << 20) and one < two <= 2 * one
    assert 2112 * 2048 * 8 < _lib.query("maavss_bss_eval_ws_bytes", 1, 2048, 3, 512) < 36 << 20


def test_new_symbols_are_in_the_header_and_the_library_and_the_abi_version_is_still_401():
    protos = _lib.parse_header()
    L = _lib.lib()
    for name in ("maavss_bss_eval_ws_bytes", "maavss_bss_eval"):
        assert name in protos and hasattr(L.cdll, name), name
    assert [n for _, n in protos["maavss_bss_eval"][1]] == ["est", "est_stride", "ref", "ref_stride", "others", "others_row_stride",
                                                            "others_src_stride", "K", "rows", "n", "L", "out", "ws", "ws_bytes", "stream"]
    assert _lib.header_abi_version() == 402 == L.cdll.maavss_version()


def test_validator_keys_and_buffer_without_and_with_the_option():
    import maavss_amd
    from maavss_amd import quality
    model = types.SimpleNamespace(training=False)
    sig = inspect.signature(maavss_amd.Validator.__init__).parameters
    assert list(sig)[-2:] == ["intelligibility_sr", "bss_filter"] and sig["bss_filter"].default is None
    assert list(inspect.signature(maavss_amd.Validator.add_waves).parameters) == ["self", "est", "ref", "noisy", "others"]
    assert list(inspect.signature(maavss_amd.Validator.add_recording).parameters)[-1] == "others"
    plain, val, both = maavss_amd.Validator(model), maavss_amd.Validator(model, bss_filter=33), maavss_amd.Validator(model, intelligibility_sr=10000, bss_filter=512)
    assert (plain._buf_len(), val._buf_len(), both._buf_len()) == (51, 96, 126) and quality._ACC_LEN == 51
    res, res_bss = plain.result(), val.result()
    assert len(res) == 21 and not any(k.startswith(("sdr", "sir", "sar", "noisy_s")) for k in res)
    new = {k + s for n in ("sdr_db", "sir_db", "sar_db") for k in (n, "noisy_" + n, n + "_improvement")
           for s in ("", "_n_finite", "_n_posinf", "_n_neginf", "_n_nan")}
    assert set(res_bss) - set(res) == new and len(new) == 45 and set(res) <= set(res_bss)
    assert math.isnan(res_bss["sir_db"]) and res_bss["sir_db_n_finite"] == 0
    assert set(both.result()) - set(res_bss) == {k + s for k in ("stoi", "estoi", "noisy_stoi", "noisy_estoi", "stoi_improvement", "estoi_improvement")
                                                 for s in ("", "_n_finite", "_n_nan")}
    for badf in (0, 513, 2.0, True, "512"):
        with pytest.raises(ValueError, match="bss_filter"):
            maavss_amd.Validator(model, bss_filter=badf)
    with pytest.raises(ValueError, match="without bss_filter"):
        plain.add_waves(torch.zeros(2, 700), torch.zeros(2, 700), others=torch.zeros(2, 700))


def test_nothing_in_bss_py_waits_for_the_device():
    """bss_eval_metrics only enqueues: by structure, no .item() / .cpu() / .tolist() / synchronize / .to() in the module."""
    import re
    import maavss_amd.bss as bss
    src = inspect.getsource(bss)
    assert not re.search(r"\.item\(|\.cpu\(|\.tolist\(|synchronize|\.to\(|\.numpy\(", src)
