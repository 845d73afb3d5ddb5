"""maavss_amd.Reverb.measure and make_room_rirs(calibrate=) on the GPU against the float64 twins (tests/rir_measure_twin.py,
tests/room_twin.py).  energy is a sum of exact squares in one stated order: the twin's bits.  The crossings are comparisons of such
sums: the twin's (tests/test_rir_measure_cpu.py holds every case's margins), and a time within the derived bound -- some 1e-12 of a
sample -- cannot belong to another crossing.  Times and dB figures go through log10 and gate on the bounds the twin derives.  Every
measure call runs under torch's sync debug mode "error"."""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

import rir_measure_twin as mt
import room_twin as rw
from maavss_amd import Reverb

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def nosync():
    torch.cuda.set_sync_debug_mode("error")                  # any blocking call of torch's raises
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


@functools.lru_cache(maxsize=None)
def _case(name):
    """A case's table and the twin's rows, computed once and left unchanged."""
    table, sr, direct_ms = mt.CASES[name]()
    table.setflags(write=False)
    return table, sr, direct_ms, mt.measure(table, sr, direct_ms)


def _raw(got):
    """measure's dict -> f64 [n, 6] on the host, in FIGURES' order."""
    assert tuple(got) == mt.FIGURES and all(v.dtype == torch.float64 and v.is_cuda and v.dim() == 1 for v in got.values())
    return np.stack([got[name].cpu().numpy() for name in mt.FIGURES], axis=1)


def _hold(got, rows, sr):
    """got f64 [n, 6] against the twin's rows: energy bit for bit, the rest within the derived bounds, every figure printed first."""
    assert got.shape == (len(rows), 6)
    for r, row in enumerate(rows):
        for c, name in enumerate(mt.FIGURES):
            want, bound = getattr(row, name), row.bound[name]
            print(f"row {r} {name}: got {got[r, c]!r} twin {want!r} diff {abs(got[r, c] - want):.3e} bound {bound:.3e}")
        assert np.float64(got[r, 0]).tobytes() == np.float64(row.energy).tobytes() or (math.isnan(row.energy) and math.isnan(got[r, 0])), (r, "energy")
        for c, name in enumerate(mt.FIGURES):
            assert mt.same_or_within(float(got[r, c]), getattr(row, name), row.bound[name]), (r, name, got[r, c], getattr(row, name), row.bound[name])
        # the crossing the -10 dB time implies is the twin's: the time lies in the twin's own sample interval [j - 1, j]
        frac = row.t[1] - math.floor(row.t[1]) if math.isfinite(row.t[1]) else math.nan
        if row.j[1] is not None and 1e-6 < frac < 1.0 - 1e-6:
            assert math.floor(got[r, 1] * sr / 6.0) == row.j[1] - 1, (r, "edt's crossing")


@pytest.mark.parametrize("name", list(mt.CASES))
def test_every_figure_against_the_twin(name):
    table, sr, direct_ms, rows = _case(name)
    rv = Reverb(table.shape[1], sr=sr)
    dev = torch.from_numpy(np.array(table)).cuda()
    with nosync():
        got = rv.measure(dev, direct_ms=direct_ms)
        again = rv.measure(dev, direct_ms=direct_ms)
    got, again = _raw(got), _raw(again)
    assert got.tobytes() == again.tobytes(), "two runs give identical bytes"
    _hold(got, rows, sr)


def test_a_row_measured_alone_has_the_bytes_it_has_in_the_table():
    table, sr, direct_ms, _ = _case("k8200")
    special, _, _, _ = _case("special")
    rv = Reverb(8, sr=sr)
    for t in (table, special):
        dev = torch.from_numpy(np.array(t)).cuda()
        with nosync():
            whole = rv.measure(dev, direct_ms=direct_ms)
            alone = [rv.measure(dev[r:r + 1], direct_ms=direct_ms) for r in range(t.shape[0])]
            swapped = rv.measure(dev.flip(0).contiguous(), direct_ms=direct_ms)
        whole, swapped = _raw(whole), _raw(swapped)
        for r in range(t.shape[0]):
            assert _raw(alone[r])[0].tobytes() == whole[r].tobytes() == swapped[t.shape[0] - 1 - r].tobytes(), r


def test_a_strided_table_is_read_where_it_lies_and_out_is_written_nowhere_else():
    table, sr, direct_ms, rows = _case("k8193")
    n, k = table.shape
    ld, lead = k + 11, 5
    room = torch.full((lead + n * ld,), float("nan"), device="cuda")                 # a NaN read from the padding would spoil a row
    view = room.as_strided((n, k), (ld, 1), lead)
    view.copy_(torch.from_numpy(np.array(table)))
    rv = Reverb(k, sr=sr)
    with nosync():
        got = rv.measure(view, direct_ms=direct_ms)
    _hold(_raw(got), rows, sr)
    # the entry point itself, into the middle of a buffer of sentinels
    from maavss_amd import _lib, reverb as reverb_mod
    import ctypes
    sentinel = -1234.5
    out = torch.full((7 + 6 * n + 7,), sentinel, device="cuda", dtype=torch.float64)
    levels = (ctypes.c_double * 4)(*reverb_mod.thresholds())
    with nosync():
        _lib.call("maavss_rir_measure", view.data_ptr(), n, k, ld, float(sr), mt.k_direct(direct_ms, sr), mt.k_early(sr), ctypes.addressof(levels), 4,
                  out[7:].data_ptr(), _lib.stream_ptr())
    host = out.cpu().numpy()
    assert (host[:7] == sentinel).all() and (host[7 + 6 * n:] == sentinel).all(), "the doubles around out are untouched"
    assert host[7:7 + 6 * n].tobytes() == _raw(got).tobytes()


def test_the_current_table_is_the_default_and_make_rirs_keeps_its_drr():
    """Rows from make_rirs: measured where they lie, against the twin on their own bytes; direct_ms = 0 gives back the requested DRR
    within the bound tests/test_reverb_gpu.py already holds the stored taps to."""
    import reverb_twin as cw
    k_taps, sr = 3000, 16000
    rt60, drr, pre = [0.05, 0.1, 0.08, 0.03], [0.0, 12.0, -3.0, 6.0], [1, 16, 80, 40]
    rv = Reverb(k_taps, sr=sr)
    with nosync():
        rirs = rv.make_rirs(4, seed=9, rt60=rt60, drr_db=drr, predelay=torch.tensor(pre))
        got = rv.measure()
        direct = rv.measure(direct_ms=0.0)
    host = rirs.cpu().numpy()
    _hold(_raw(got), mt.measure(host, sr, 2.5), sr)
    _hold(_raw(direct), mt.measure(host, sr, 0.0), sr)
    for r in range(4):
        assert abs(float(direct["drr_db"][r]) - drr[r]) <= cw.drr_bound_db(k_taps), r


@pytest.mark.parametrize("name", ["s5", "two_sizes", "near"])
def test_rows_from_make_room_rirs(name):
    _, k, h, r, sr, rooms = next(c for c in rw.CASES if c[0] == name)
    rv = Reverb(k, sr=sr)
    with nosync():
        rirs = rv.make_room_rirs([x[0] for x in rooms], [x[1] for x in rooms], [x[2] for x in rooms], beta=[x[3] for x in rooms])
        got = rv.measure()
    _hold(_raw(got), mt.measure(rirs.cpu().numpy(), sr, 2.5), sr)


# ---- calibration ---------------------------------------------------------------------------------------------------------------------------
def test_calibration_makes_rt60_the_measured_t20():
    dims, mic, sources = [r[0] for r in mt.CAL_ROOMS], [r[1] for r in mt.CAL_ROOMS], [r[2] for r in mt.CAL_ROOMS]
    target = np.array(mt.CAL_TARGETS)
    kd, ke = mt.k_direct(2.5, mt.CAL_SR), mt.k_early(mt.CAL_SR)

    def twin_t20(table):
        return np.array([mt.measure_row(h, mt.CAL_SR, kd, ke).t20 for h in table]).reshape(3, 2).mean(axis=1)

    rv = Reverb(mt.CAL_TAPS, sr=mt.CAL_SR)
    plain = rv.make_room_rirs(dims, mic, sources, rt60=list(mt.CAL_TARGETS)).cpu().numpy()
    assert rv.room_beta is None and rv.calibration_rounds is None
    off = np.abs(twin_t20(plain) - target) / target
    print("uncalibrated T20", twin_t20(plain), "requested", target)
    assert bool((off > mt.CAL_TOL).all()), "Eyring's nominal coefficient is more than tol off in every room"

    rirs = rv.make_room_rirs(dims, mic, sources, rt60=list(mt.CAL_TARGETS), calibrate="t20", tol=mt.CAL_TOL, max_iter=mt.CAL_MAX_ITER)
    print("rounds", rv.calibration_rounds, "beta", rv.room_beta[:, 0].tolist(), "measured", rv.room_measured.tolist())
    assert rirs is rv.rirs and rv.sources_per_room == 2 and tuple(rirs.shape) == (6, mt.CAL_TAPS)
    assert rv.room_converged.dtype == torch.bool and rv.room_converged.tolist() == [True] * 3
    assert 1 <= rv.calibration_rounds <= mt.CAL_MAX_ITER
    assert tuple(rv.room_beta.shape) == (3, 6) and rv.room_beta.dtype == torch.float64 and not rv.room_beta.is_cuda
    assert bool((rv.room_beta == rv.room_beta[:, :1]).all()) and bool(((rv.room_beta > 0) & (rv.room_beta < 1)).all())
    want = rw.table_of([(d, m, s, tuple(b.tolist())) for d, m, s, b in zip(dims, mic, sources, rv.room_beta)], mt.CAL_TAPS, mt.CAL_SR,
                       table=Reverb.kernel_table().numpy())
    got = rirs.cpu().numpy()
    assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), "reverb.rirs is the twin's response at room_beta, bit for bit"
    found = twin_t20(want)
    print("calibrated T20", found)
    assert bool((np.abs(found - target) <= mt.CAL_TOL * target).all())
    assert bool((np.abs(rv.room_measured.numpy() - found) <= 1e-9).all()), "what the device measured is what the twin measures"
    # the same bytes as the explicit call, which forgets nothing it should keep
    again = Reverb(mt.CAL_TAPS, sr=mt.CAL_SR).make_room_rirs(dims, mic, sources, beta=rv.room_beta)
    assert torch.equal(again, rirs)


def test_calibration_with_a_short_stored_table_and_a_room_that_cannot_converge():
    """measure_len is independent of rir_len; max_iter = 1 leaves Eyring's coefficient, flagged, and raises nothing."""
    dims, mic, sources = [r[0] for r in mt.CAL_ROOMS], [r[1] for r in mt.CAL_ROOMS], [r[2] for r in mt.CAL_ROOMS]
    rv = Reverb(300, sr=mt.CAL_SR)
    rirs = rv.make_room_rirs(dims, mic, sources, rt60=list(mt.CAL_TARGETS), calibrate="t20", max_iter=1)
    assert tuple(rirs.shape) == (6, 300) and rv.calibration_rounds == 1 and rv.room_converged.tolist() == [False] * 3
    assert torch.allclose(rv.room_beta, Reverb.eyring_beta(dims, list(mt.CAL_TARGETS)), rtol=1e-12, atol=0.0)      # through x = -1 / ln(beta) and back
    assert torch.equal(rirs, Reverb(300, sr=mt.CAL_SR).make_room_rirs(dims, mic, sources, beta=rv.room_beta))
    target = torch.tensor(mt.CAL_TARGETS, dtype=torch.float64)
    assert bool(torch.isfinite(rv.room_measured).all()) and bool(((rv.room_measured - target).abs() > mt.CAL_TOL * target).all())
