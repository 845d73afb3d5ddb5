"""Validator(bss_filter=...) on the GPU: the third additive accumulator of BSS-eval SDR, SIR and SAR (maavss_amd/bss.py) against the
float64 twin (tests/bss_twin.py), and the Validator without the option, which must be what it was."""
import math
import types

import numpy as np
import pytest
import torch

import maavss_amd
import bss_twin as tw
from test_bss_gpu import GATE

pytestmark = pytest.mark.gpu

KEYS = tw.SCORES


def _mean(vals):
    fin = [v for v in vals if math.isfinite(v)]
    return math.fsum(fin) / len(fin), len(fin)


def test_add_waves_accumulates_the_scores_over_ragged_batches_and_waits_only_in_result():
    batches = tw.validator_batches()
    dev = [[torch.from_numpy(a).cuda() for a in batch] for batch in batches]
    val = maavss_amd.Validator(None, bss_filter=tw.VALIDATOR_FILTER)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")             # any blocking call of torch's before result() raises
    try:
        for est, ref, noisy, oth in dev:
            val.add_waves(est, ref, noisy, others=oth)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    res = val.result()
    f = tw.VALIDATOR_FILTER
    est_rows = [tw.bss_row(e, r, o, f) for est, ref, _, oth in batches for e, r, o in zip(est, ref, oth)]
    noisy_rows = [tw.bss_row(q, r, o, f) for _, ref, noisy, oth in batches for q, r, o in zip(noisy, ref, oth)]
    assert [r["status"] for r in est_rows] == [0, 0, 0, 0, 1] and all(r["status"] == 0 for r in noisy_rows)
    for key in KEYS:
        e, q = [r[key] for r in est_rows], [r[key] for r in noisy_rows]
        gain = [a - b for a, b in zip(e, q)]             # per clip; NaN where the estimate has a status
        for name, vals, n_fin, tol in ((key, e, 4, GATE), ("noisy_" + key, q, 5, GATE), (key + "_improvement", gain, 4, 2 * GATE)):
            want, count = _mean(vals)                   # a difference of two scores carries the rounding of both: twice the gate
            print(f"{name}: {res[name]!r} twin {want!r}")
            assert count == n_fin and res[name + "_n_finite"] == n_fin and res[name + "_n_nan"] == 5 - n_fin
            assert res[name + "_n_posinf"] == 0 and res[name + "_n_neginf"] == 0
            assert abs(res[name] - want) <= tol, (name, res[name], want)
    assert res["sir_db_improvement"] > 15 and res["sdr_db_improvement"] > 15, "a tenth of the leakage must be seen"
    assert abs(res["sar_db_improvement"]) < 5
    assert val.acc.shape == (51,) and val.acc_intel is None and val.acc_bss.shape == (45,)
    assert val.acc_bss.data_ptr() == val.acc.data_ptr() + 51 * 8, "one allocation: result() makes one copy"
    val.reset()
    again = val.result()
    assert again["sir_db_n_finite"] == 0 and math.isnan(again["sir_db"]) and again["n_clips"] == 0


def test_the_improvement_is_the_mean_of_the_per_clip_differences():
    est, ref, noisy, oth = (torch.from_numpy(a).cuda() for a in tw.validator_batches()[0])
    val = maavss_amd.Validator(None, bss_filter=tw.VALIDATOR_FILTER)
    val.add_waves(est, ref, noisy, others=oth)
    res = val.result()
    m = maavss_amd.bss_eval_metrics(est, ref, oth, tw.VALIDATOR_FILTER)
    mn = maavss_amd.bss_eval_metrics(noisy, ref, oth, tw.VALIDATOR_FILTER)
    for key in KEYS:
        e, q = m[key].cpu().numpy(), mn[key].cpu().numpy()
        assert abs(res[key] - e.sum() / 3) <= 1e-12 and abs(res["noisy_" + key] - q.sum() / 3) <= 1e-12
        assert abs(res[key + "_improvement"] - (e - q).sum() / 3) <= 1e-12 and res[key + "_improvement_n_finite"] == 3
    # without another source every clip's sir_db is +inf: counted, not averaged; inf - inf is NaN
    alone = maavss_amd.Validator(None, bss_filter=tw.VALIDATOR_FILTER)
    alone.add_waves(est, ref, noisy)
    res = alone.result()
    assert res["sir_db_n_posinf"] == 3 and res["sir_db_n_finite"] == 0 and math.isnan(res["sir_db"]) and res["sir_db_improvement_n_nan"] == 3
    assert res["sdr_db_n_finite"] == 3 and res["sdr_db"] == res["sar_db"]


class _Cut:
    """An enhancer that returns samples [start, start + n) of its input, scaled: add_recording has to measure that span."""

    def __init__(self, model, start, n):
        self.model, self.start, self.n = model, start, n

    def __call__(self, noisy, frames=None, attn=None):
        return 0.5 * noisy[self.start:self.start + self.n] + 0.5 * noisy[self.start + 1:self.start + self.n + 1], self.start


def test_add_recording_measures_the_span_the_estimate_covers():
    model = types.SimpleNamespace(training=False)
    est, ref, oth = tw.gpu_case("L65")
    noisy, clean, others = (torch.from_numpy(a).cuda() for a in (est, ref, oth))
    start, n = 37, 801
    enh = _Cut(model, start, n)
    wave, _ = enh(noisy)
    for given in (others, others[0]):                   # [K, L] and [L]
        val = maavss_amd.Validator(model, bss_filter=33)
        val.add_recording(enh, noisy, clean, others=given)
        res = val.result()
        want = tw.bss_row(wave.cpu().numpy(), ref[start:start + n], oth[:, start:start + n], 33)
        want_noisy = tw.bss_row(est[start:start + n], ref[start:start + n], oth[:, start:start + n], 33)
        for key in KEYS:
            print(f"{key}: {res[key]!r} twin {want[key]!r}; noisy {res['noisy_' + key]!r} twin {want_noisy[key]!r}")
            assert abs(res[key] - want[key]) <= GATE and abs(res["noisy_" + key] - want_noisy[key]) <= GATE
            assert abs(res[key + "_improvement"] - (want[key] - want_noisy[key])) <= 2 * GATE
        assert res["n_clips"] == 1 and res["sir_db_n_finite"] == 1
    with pytest.raises(ValueError, match="cover"):
        maavss_amd.Validator(model, bss_filter=33).add_recording(enh, noisy, clean, others=others[:, :start + n - 1])


def test_without_the_option_the_validator_is_what_it_was():
    """bss_filter=None: the result dict and .acc are bit-identical to a Validator built without the argument, for the same calls."""
    dev = [[torch.from_numpy(a).cuda() for a in batch] for batch in tw.validator_batches()]
    plain, none, with_bss = maavss_amd.Validator(None), maavss_amd.Validator(None, bss_filter=None), maavss_amd.Validator(None, bss_filter=33)
    for est, ref, noisy, oth in dev:
        plain.add_waves(est, ref, noisy)
        none.add_waves(est, ref, noisy)
        with_bss.add_waves(est, ref, noisy, others=oth)
    res, res_none, res_bss = plain.result(), none.result(), with_bss.result()
    assert plain.acc.shape == none.acc.shape == (51,) and none.acc_bss is None and none._buf.numel() == 51
    assert plain.acc.view(torch.int64).equal(none.acc.view(torch.int64)) and plain.acc.view(torch.int64).equal(with_bss.acc.view(torch.int64))
    assert list(res) == list(res_none) and not any(k.startswith(("sdr", "sir", "sar")) for k in res)
    for k, v in res.items():
        assert np.float64(res_none[k]).tobytes() == np.float64(v).tobytes(), k
        assert res_bss[k] == v or (v != v and res_bss[k] != res_bss[k]), k
