"""CPU-only: the float64 twin of the room-acoustic figures (tests/rir_measure_twin.py) held to things it does not restate -- another
order of the same sums, room_twin's T20, the closed form of an exponential decay, the DRR make_rirs promises -- the margins that make
its decisions the kernel's, the calibration rule run on the twins, and every refusal of Reverb.measure, of make_room_rirs'
calibration arguments and of the entry point, none of which touches a device."""
import functools
import math

import numpy as np
import pytest
import torch

import reverb_twin as cw
import rir_measure_twin as mt
import room_twin as rw
from maavss_amd import Reverb, _lib
from maavss_amd import reverb as reverb_mod


@functools.lru_cache(maxsize=None)
def _case(name):
    table, sr, direct_ms = mt.CASES[name]()
    table.setflags(write=False)
    return table, sr, direct_ms, mt.measure(table, sr, direct_ms)


def _finite(h):
    return bool(np.isfinite(h).all())


def test_the_package_and_the_twin_agree_on_names_levels_and_thresholds():
    assert reverb_mod.FIGURES == mt.FIGURES and reverb_mod.LEVELS_DB == mt.LEVELS_DB
    assert reverb_mod.thresholds() == mt.THRESHOLDS                      # the same bits: the kernel compares against what the twin does
    assert set(reverb_mod.CALIBRATE) == {"t20", "t30", "edt"}
    protos = _lib.parse_header()
    assert "maavss_rir_measure" in protos and len(protos["maavss_rir_measure"][1]) == 11 and _lib.header_abi_version() == 402
    rv = Reverb(8, sr=16000, device="cpu")
    for ms in (0.0, 1.0, 2.5, 7.77):
        assert rv.check_measure(torch.zeros(2, 8), ms)[1:] == (mt.k_direct(ms, 16000), mt.k_early(16000))
    assert mt.k_direct(0.0, 16000) == 1 and mt.k_early(16000) == 800


@pytest.mark.parametrize("name", list(mt.CASES))
def test_backward_energy_against_cumsum(name):
    """np.cumsum over the reversed squares adds the same non-negative terms in another order: within 2 gamma(K - 1)."""
    table, _, _, rows = _case(name)
    k_taps = table.shape[1]
    for h, row in zip(table, rows):
        if not _finite(h):
            assert math.isnan(row.energy)
            continue
        x = h.astype(np.float64)
        want = np.cumsum((x * x)[::-1])[::-1]
        assert row.e.shape == want.shape and bool((np.diff(row.e) <= 0).all()), "E never grows"
        assert bool((np.abs(row.e - want) <= 2.0 * mt.gamma(k_taps - 1) * mt.SLACK * want).all())
        assert row.energy == row.e[0]


@pytest.mark.parametrize("name", list(mt.CASES))
def test_every_case_keeps_its_crossings_away_from_the_thresholds(name):
    """E[j] and E[j - 1] of every crossing lie MARGIN x 2 gamma(K - 1) E[0] or more from E[0] c: no order of the additions, and no
    last-bit difference in E[0] c, can move a crossing, so the decisions the GPU tests see are the twin's."""
    table, _, _, rows = _case(name)
    for r, (h, row) in enumerate(zip(table, rows)):
        if _finite(h):
            for level, distance in mt.margins(row, table.shape[1]):
                assert distance >= mt.MARGIN, (name, r, level, distance)


def test_early_energy_is_exact_where_the_direct_path_stands_alone():
    table, sr, _, _ = _case("k8200")
    for h in table:
        row = mt.measure_row(h, sr, 1, mt.k_early(sr))
        assert row.early_d == float(np.float64(h[0]) ** 2) and row.late_d == row.e[1]
        x = h.astype(np.float64)
        exact = math.fsum((x * x)[:800])
        assert abs(row.early_e - exact) <= mt.gamma(799) * exact * mt.SLACK
    assert mt.early_energy(table[0], 0) == 0.0 and mt.early_energy(table[0], 10 ** 6) > 0.0


ROOMS = [(rw.SMALL, 3000), (rw.MID5, 2500), (rw.NEAR, 3500)]


@pytest.mark.parametrize("room", range(len(ROOMS)))
def test_t20_against_room_twin_on_image_source_rows(room):
    """room_twin.t20 adds with np.cumsum and compares in dB: another order of the same sums, so within time_bound with order_db_err."""
    (dims, mic, srcs, beta), k_taps = ROOMS[room]
    sr = 16000
    for src in srcs[:2]:
        h = rw.response(dims, mic, src, beta, k_taps, sr).h
        row = mt.measure_row(h, sr, mt.k_direct(2.5, sr), mt.k_early(sr), err=lambda d: mt.order_db_err(d, k_taps))
        assert all(d >= mt.MARGIN for _, d in mt.margins(row, k_taps))
        want = rw.t20(h, sr)
        assert math.isfinite(want) and abs(row.t20 - want) <= row.bound["t20"], (row.t20, want, row.bound["t20"])
        assert row.bound["t20"] < 1e-9


@pytest.mark.parametrize("rt60,sr,k_taps", [(0.2, 16000, 8192), (0.05, 16000, 2048), (0.3, 44100, 30000)])
def test_a_pure_exponential_has_one_decay_time(rt60, sr, k_taps):
    """h[k] = exp(-lam k), lam = ln(1000) / (rt60 sr): E[k] is A (exp(-2 lam k) - exp(-2 lam K)), a straight line in dB of slope
    g = 20 lam / ln 10 per sample but for the cut's term 10 log10(1 - exp(-2 lam (K - k))), and a straight line's interpolated crossing
    is exact: EDT = T20 = T30 = rt60.  What moves a crossing: the cut, at most eps / (1 - eps) relative in E[k] with
    eps = exp(-2 lam (K - j35)) (j35 the -35 dB sample, below 36 / g); the f32 rounding of the taps, 2^-23 (1 + 2^-24) relative in
    every square and so in every E[k] and in E[0].  A curve within eta dB of the line crosses a level within eta / g samples of it
    (E never grows), eta = (10 / ln 10) (eps / (1 - eps) + 2 * 2^-23 * 1.001) + 1e-12 for the f64 roundings; EDT has no lower
    crossing to subtract but starts from d[0] = 0 exactly: 6 eta / (g sr); T20 and T30: two crossings, 3 * 2 eta / (g sr) and
    2 * 2 eta / (g sr)."""
    lam = math.log(1000.0) / (rt60 * sr)
    h = np.exp(-lam * np.arange(k_taps, dtype=np.float64)).astype(np.float32)
    row = mt.measure_row(h, sr, 1, mt.k_early(sr))
    g = 20.0 * lam / math.log(10.0)
    eps = math.exp(-2.0 * lam * (k_taps - 36.0 / g))
    eta = 10.0 / math.log(10.0) * (eps / (1.0 - eps) + 2.0 * 2.0 ** -23 * 1.001) + 1e-12
    assert abs(row.edt - rt60) <= 6.0 * eta / (g * sr)
    assert abs(row.t20 - rt60) <= 6.0 * eta / (g * sr)
    assert abs(row.t30 - rt60) <= 4.0 * eta / (g * sr)
    assert 6.0 * eta / (g * sr) < 1e-5 * rt60


@pytest.mark.parametrize("drr", [-3.0, 0.0, 7.5, 20.0])
def test_drr_of_a_noise_room_at_direct_ms_0_is_the_request(drr):
    """make_rirs' definition (reverb_twin.rir): h[0] = 1 and the stored tail holds 10^(-drr / 10).  direct_ms = 0 sets tap 0 alone
    against E[1]: early is exactly 1, and the tail in this twin's order lies within gamma(K) of reverb_twin's fsum, inside the
    (K + 16) 2^-51 that reverb_twin.drr_bound_db already allows the sum."""
    rng = np.random.default_rng(int(drr * 10) + 50)
    k_taps, k0, sr = 3000, 17, 16000
    h, _, _ = cw.rir(rng.standard_normal(k_taps).astype(np.float32), cw.lam_of(0.1, sr), 10.0 ** (drr / 10.0), k0)
    row = mt.measure_row(h, sr, mt.k_direct(0.0, sr), mt.k_early(sr))
    assert row.early_d == 1.0
    assert abs(row.drr_db - drr) <= cw.drr_bound_db(k_taps)
    assert abs(row.drr_db - cw.drr_db(h, 1)) <= cw.drr_bound_db(k_taps)


# ---- the calibration rule on the twins ---------------------------------------------------------------------------------------------------
def twin_t20(beta, taps=mt.CAL_TAPS):
    """Per room of CAL_ROOMS: the mean over its sources of the twin's T20 of the twin's response with `beta` on all six walls."""
    out = []
    for (dims, mic, srcs), b in zip(mt.CAL_ROOMS, beta):
        rows = [mt.measure_row(rw.response(dims, mic, s, (float(b),) * 6, taps, mt.CAL_SR).h, mt.CAL_SR, mt.k_direct(2.5, mt.CAL_SR),
                               mt.k_early(mt.CAL_SR)) for s in srcs]
        out.append(float(np.mean([r.t20 for r in rows])))
    return np.array(out)


def test_the_calibration_rule_converges_on_the_twin():
    target = torch.tensor(mt.CAL_TARGETS, dtype=torch.float64)
    beta0 = Reverb.eyring_beta([r[0] for r in mt.CAL_ROOMS], target)[:, 0]
    nominal = twin_t20(beta0.numpy())
    assert bool((np.abs(nominal - target.numpy()) > mt.CAL_TOL * target.numpy()).all()), "Eyring's coefficient is more than tol off in every room"
    search = reverb_mod.Calibration(beta0, target, mt.CAL_TOL)
    assert torch.equal(search.beta(), torch.exp(-1.0 / (-1.0 / torch.log(beta0))))
    for _ in range(mt.CAL_MAX_ITER):
        if search.update(torch.from_numpy(twin_t20(search.beta().numpy()))):
            break
    assert bool(search.converged.all()) and search.rounds <= mt.CAL_MAX_ITER
    found = twin_t20(reverb_mod.Calibration.beta_of(search.best_x).numpy())
    assert bool((np.abs(found - target.numpy()) <= mt.CAL_TOL * target.numpy()).all())
    assert np.array_equal(found, search.best_t.numpy())


def test_the_calibration_rule_brackets_and_flags():
    """A decay time that is not smooth in x: the plain step would jump between the two sides for ever; the bracket's midpoints settle.
    A room that cannot be brought inside tol keeps its best coefficient and is flagged."""
    def figure(x):                                           # T = x below 1, x + 0.3 above: no x gives T in (1, 1.3)
        return torch.where(x < 1.0, x, x + 0.3)

    search = reverb_mod.Calibration(torch.exp(-1.0 / torch.tensor([0.5, 0.5])), torch.tensor([0.9, 1.15]), 0.01)
    for _ in range(12):
        if search.update(figure(-1.0 / torch.log(search.beta()))):
            break
    assert search.converged.tolist() == [True, False] and search.rounds == 12
    assert abs(float(search.best_t[0]) - 0.9) <= 0.009
    assert 0.0 < float(search.lo[1]) < 1.0 <= float(search.hi[1]) and float(search.hi[1]) - float(search.lo[1]) < 0.01
    assert 0.15 / 1.15 <= float(search.best_err[1]) <= 0.151 / 1.15, "the best coefficient seen is kept: T just below 1 or just above 1.3"
    # a NaN (the level not reached inside the measured taps) counts as too slow a decay: x shrinks
    nan = reverb_mod.Calibration(torch.exp(-1.0 / torch.tensor([2.0], dtype=torch.float64)), torch.tensor([0.5]), 0.01)
    x0 = float(nan.x[0])
    assert abs(x0 - 2.0) < 1e-12
    assert not nan.update(torch.tensor([math.nan])) and float(nan.x[0]) == 0.5 * x0 and float(nan.hi[0]) == x0 and not bool(nan.converged[0])
    assert not nan.update(torch.tensor([0.25])) and float(nan.lo[0]) == 0.5 * x0      # the step 1.0 * 0.5 / 0.25 = 2 is not inside (1, 2): the midpoint
    assert float(nan.x[0]) == 0.5 * (0.5 * x0 + x0)


# ---- refusals: nothing below touches a device --------------------------------------------------------------------------------------------
def test_measure_refuses_before_any_device_work():
    rv = Reverb(64, sr=16000, device="cpu")
    good = torch.zeros(3, 64)

    def refuse(match, rirs=good, **kw):
        with pytest.raises(ValueError, match=match):
            rv.measure(rirs, **kw)

    refuse("no room responses yet", rirs=None)
    refuse("float32", rirs=good.double())
    refuse("float32", rirs=[[1.0]])
    refuse(r"\[n, K\]", rirs=torch.zeros(64))
    refuse(r"\[n, K\]", rirs=torch.zeros(2, 3, 4))
    refuse(r"\[n, K\]", rirs=torch.zeros(0, 4))
    refuse("unit last stride", rirs=torch.zeros(3, 128)[:, ::2])
    refuse("unit last stride", rirs=torch.zeros(64, 3).t())
    refuse("row stride of at least", rirs=torch.zeros(100).as_strided((3, 64), (10, 1)))
    refuse("at most", rirs=torch.zeros(1, 32769))
    refuse("direct_ms", direct_ms=-0.1)
    refuse("direct_ms", direct_ms=math.nan)
    refuse("direct_ms", direct_ms=math.inf)
    refuse("direct_ms", direct_ms="2")
    refuse("direct_ms", direct_ms=True)
    with pytest.raises(ValueError, match="is on cpu, this Reverb on cuda"):
        Reverb(64).measure(good)
    # what passes reaches the device call, which has no CPU fallback
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        rv.measure(good)
    assert rv.check_measure(torch.zeros(200).as_strided((3, 64), (68, 1)), 0.0)[1] == 1


def test_calibration_arguments_are_refused_before_any_device_work():
    rv = Reverb(512, sr=16000, device="cpu")
    dims, mic, src = [[4.0, 3.5, 2.5]], [[1.7, 1.9, 1.2]], [[[2.9, 0.8, 1.4]]]

    def refuse(match, **kw):
        args = dict(rt60=[0.2], calibrate="t20")
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            rv.make_room_rirs(dims, mic, src, **args)
        assert rv.rirs is None and rv.room_beta is None

    refuse("calibrate must be None or one of", calibrate="t60")
    refuse("give rt60 and no beta", rt60=None, beta=[[0.5] * 6])
    refuse("give rt60 and no beta", beta=[[0.5] * 6])
    refuse("tol must be", tol=0.0)
    refuse("tol must be", tol=math.nan)
    refuse("max_iter", max_iter=0)
    refuse("measure_len", measure_len=0)
    refuse("measure_len", measure_len=2.5)
    refuse("at most 32768", measure_len=40000)
    refuse("at most 32768", rt60=[3.0])                                  # 0.75 * 3 s * 16 kHz = 36000 taps
    refuse("finite and positive", rt60=[0.0])
    refuse("rt60 must be a number or hold 1", rt60=[0.2, 0.3])
    # the scratch table's lattice box, not only the stored table's: 512 taps fit this corridor, the 3072 a T20 of 0.25 s asks for do not
    corridor = dict(dims=[[0.1, 0.1, 0.1]], mic=[[0.05, 0.05, 0.05]], sources=[[[0.07, 0.05, 0.05]]])
    rv.check_rooms(corridor["dims"], corridor["mic"], corridor["sources"], rt60=[0.25])
    with pytest.raises(ValueError, match="for 3072 taps, above the cap"):
        rv.make_room_rirs(corridor["dims"], corridor["mic"], corridor["sources"], rt60=[0.25], calibrate="t20")
    assert rv.check_calibration(dims, [0.15, 0.25], None, "t20", 0.02, 12, None) == 3072
    assert rv.check_calibration(dims, 0.15, None, "t20", 0.02, 12, None) == 2048
    assert rv.check_calibration(dims, 0.25, None, "t30", 0.02, 12, None) == 4096 and rv.check_calibration(dims, 0.25, None, "edt", 0.02, 12, None) == 2048
    assert rv.check_calibration(dims, 0.25, None, "edt", 0.02, 12, 700) == 700
    # what passes reaches the device call, which has no CPU fallback; nothing is kept
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        rv.make_room_rirs(dims, mic, src, rt60=[0.2], calibrate="t20")
    assert rv.rirs is None and rv.room_beta is None and rv.calibration_rounds is None


def test_the_entry_point_refuses_from_its_arguments_alone():
    """maavss_rir_measure checks its arguments and the host thresholds before the launch: the device pointers below are never touched."""
    good = np.array(mt.THRESHOLDS, dtype=np.float64)

    def call(match, thr=good, n_thr=4, rows=2, k=300, ld=300, sr=16000.0, kd=41, ke=800, dev=256, out=256):
        with pytest.raises(_lib.MaavssError, match=match):
            _lib.call("maavss_rir_measure", dev, rows, k, ld, sr, kd, ke, None if thr is None else thr.ctypes.data, n_thr, out, None)

    call("null pointer", dev=None)
    call("null pointer", thr=None)
    call("null pointer", out=None)
    call("n_rows", rows=0)
    call("n_rows", rows=(1 << 19) + 1)
    call(r"K = 0 must be in \[1, 32768\]", k=0)
    call("K = 32769 must be in", k=32769, ld=40000)
    call("must be at least K", ld=299)
    call("sr = .* must be positive", sr=0.0)
    call("sr = .* must be positive", sr=math.nan)
    call("must not be negative", kd=-1)
    call("must not be negative", ke=-1)
    call("n_thresholds = 3", n_thr=3)
    call(r"thresholds\[0\]", thr=np.array([1.0, 0.1, 0.01, 0.001]))
    call(r"thresholds\[2\]", thr=np.array([0.3, 0.1, 0.1, 0.001]))
    call(r"thresholds\[3\]", thr=np.array([0.3, 0.1, 0.01, 0.0]))
    call(r"thresholds\[1\]", thr=np.array([0.3, math.nan, 0.01, 0.001]))
    call("aligned", dev=258)
    call("aligned", out=260)
