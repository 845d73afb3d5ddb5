"""maavss_amd.Reverb without a device: the float64 twin (tests/reverb_twin.py) against an independent formulation of the convolution,
the envelope and the DRR it defines, the formulas it holds the drawn normals to, the seeded samplers, and every refusal of Reverb and
of ClipPipeline(reverb=) -- all raised before any device work."""
import math

import numpy as np
import pytest
import torch

import reverb_twin as tw
import maavss_amd
from maavss_amd import ClipBank, Reverb, _lib

K = 96


def _reverb(k=K, rooms=4, **kw):
    rv = Reverb(k, device="cpu", **kw)
    if rooms:
        rv.rirs = torch.zeros(rooms, k)            # what make_rirs leaves behind; the checks only look at its shape
    return rv


def test_exported():
    assert maavss_amd.Reverb is maavss_amd.reverb.Reverb is Reverb
    protos = _lib.parse_header()
    assert "maavss_reverb" in protos and "maavss_rir_synth" in protos and _lib.header_abi_version() == 402


# ---- the twin --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_taps,length,lead", [(1, 7, 0), (2, 5, 3), (65, 300, 0), (257, 100, 40), (257, 100, 400)])
def test_twin_convolution_against_numpy_convolve(k_taps, length, lead):
    rng = np.random.default_rng(k_taps * 1000 + length)
    src = rng.standard_normal(lead + length + 5).astype(np.float32)
    h = (rng.standard_normal((2, k_taps)) * np.exp(-0.02 * np.arange(k_taps))).astype(np.float32)
    got = tw.reverb(src, [lead, lead + 5], [0, 5], length, h, [1, 0])
    for b, (s0, fl, r) in enumerate(((lead, 0, 1), (lead + 5, 5, 0))):
        x = src[fl:s0 + length].astype(np.float64)
        full = np.convolve(h[r].astype(np.float64), x)[s0 - fl:s0 - fl + length]
        mass = np.convolve(np.abs(h[r]).astype(np.float64), np.abs(x))[s0 - fl:s0 - fl + length]
        bound = k_taps * 2.0 ** -52 * mass + np.spacing(np.abs(full).astype(np.float32)).astype(np.float64)      # + one f32 rounding
        assert got.dtype == np.float32 and np.all(np.abs(got[b].astype(np.float64) - full) <= bound)


def test_twin_leaves_terms_below_the_floor_out():
    # an inf in front of the floor must not reach the output, not even as inf * 0
    src = np.array([np.inf, 1.0, 2.0, 3.0], dtype=np.float32)
    h = np.array([[1.0, 0.0, 0.5]], dtype=np.float32)
    out = tw.reverb(src, [1], [1], 3, h, [0])
    assert out.tolist() == [[1.0, 2.0, 3.5]]
    heard = tw.reverb(src, [1], [0], 3, h, [0])[0]                              # as history: inf * 0.0 at lag 1, inf * 0.5 at lag 2
    assert np.isnan(heard[0]) and heard[1] == np.inf and heard[2] == 3.5


def test_twin_envelope_falls_60_db_per_rt60():
    sr, rt60 = 16000, 0.25
    env = tw.envelope(tw.lam_of(rt60, sr), 12000)
    step = int(rt60 * sr)
    db = 20.0 * np.log10(env[:-step] / env[step:])
    assert np.all(np.abs(db - 60.0) <= 1e-12 * 60.0)
    g1 = tw.rir(np.ones(12000, dtype=np.float32), tw.lam_of(rt60, sr), 1.0, 1)[1]
    assert np.all(np.abs(20.0 * np.log10(g1[1:-step] / g1[1 + step:]) - 60.0) <= 1e-12 * 60.0)


@pytest.mark.parametrize("drr", [-3.0, 0.0, 7.5, 20.0])
def test_twin_drr_is_the_request(drr):
    rng = np.random.default_rng(5)
    k0 = 23
    h, exact, s = tw.rir(rng.standard_normal(3000).astype(np.float32), tw.lam_of(0.1, 16000), 10.0 ** (drr / 10.0), k0)
    assert s > 0 and h[0] == 1.0 and not h[1:k0].any() and h.dtype == np.float32
    assert abs(tw.drr_db(exact, k0) - drr) <= 1e-12
    assert abs(tw.drr_db(h, k0) - drr) <= tw.drr_bound_db(3000)


def test_twin_zero_energy_tail():
    for noise, k0 in ((np.zeros(40, dtype=np.float32), 3), (np.ones(40, dtype=np.float32), 40), (np.ones(40, dtype=np.float32), 77)):
        h, _, s = tw.rir(noise, 0.01, 2.0, k0)
        assert s == 0.0 and h.tolist() == [1.0] + [0.0] * 39 and not np.signbit(h).any()


def test_twin_tail_energy_is_a_sum():
    rng = np.random.default_rng(9)
    for n in (1, 5, 1023, 1024, 1025, 5000):
        sq = rng.standard_normal(n) ** 2
        assert abs(tw.tail_energy(sq) - math.fsum(sq)) <= n * 2.0 ** -52 * math.fsum(sq)


def test_normal_statistics_formulas_hold_for_numpy_normals():
    rows, k_taps, k0, lam, drr = 16, 4096, 32, tw.lam_of(2048 / 16000, 16000), 4.0
    rng = np.random.default_rng(11)
    expect = tw.normal_stats_expect(rows, k_taps, lam, k0)
    inside = 0
    for _ in range(8):
        rirs = np.stack([tw.rir(rng.standard_normal(k_taps).astype(np.float32), lam, drr, k0)[0] for _ in range(rows)])
        got = tw.normal_stats(rirs, lam, drr, k0)
        assert all(abs(g - e) <= 6.0 * se for g, (e, se) in zip(got, expect)), (got, expect)
        inside += all(abs(g - e) <= 2.0 * se for g, (e, se) in zip(got, expect))
    assert inside >= 4, "the standard errors are not far too wide either: most draws lie within two of them"
    # and a wrong generator is seen: variance 1.3, or neighbours correlated
    bad = np.stack([tw.rir((rng.standard_normal(k_taps) * math.sqrt(1.3)).astype(np.float32), lam, drr, k0)[0] for _ in range(rows)])
    assert abs(tw.normal_stats(bad, lam, drr, k0)[1] - expect[1][0]) <= 6.0 * expect[1][1], "the scale of g is normalised away ..."
    g = rng.standard_normal((rows, k_taps + 1))
    corr = np.stack([tw.rir((g[r, 1:] + 0.5 * g[r, :-1]).astype(np.float32), lam, drr, k0)[0] for r in range(rows)])
    assert abs(tw.normal_stats(corr, lam, drr, k0)[2]) > 6.0 * expect[2][1], "... correlation is not"


# ---- the samplers ----------------------------------------------------------------------------------------------------------------------
def test_sample_draw_order_and_ranges():
    rv = _reverb(rt60=(0.2, 0.8), drr_db=(-2.0, 12.0), predelay_ms=(1.0, 5.0))
    rt, drr, pre = rv.sample(50, torch.Generator().manual_seed(3))
    u = torch.rand(3, 50, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    assert rt.dtype == drr.dtype == torch.float64 and pre.dtype == torch.int32
    assert torch.equal(rt, 0.2 + (0.8 - 0.2) * u[0]) and torch.equal(drr, -2.0 + 14.0 * u[1])
    assert torch.equal(pre, ((1.0 + 4.0 * u[2]) * 16.0).round().to(torch.int32))
    assert 0.2 <= rt.min() and rt.max() <= 0.8 and 16 <= pre.min() and pre.max() <= 80
    assert Reverb(8, predelay_ms=(0.0, 0.0), device="cpu").sample(3, torch.Generator().manual_seed(0))[2].tolist() == [1, 1, 1]
    fixed = Reverb(8, rt60=(0.5, 0.5), drr_db=(3.0, 3.0), device="cpu").sample(2, torch.Generator().manual_seed(0))
    assert fixed[0].tolist() == [0.5, 0.5] and fixed[1].tolist() == [3.0, 3.0]


def test_sample_index_is_one_randint():
    rv = _reverb(rooms=7)
    idx = rv.sample_index(40, torch.Generator().manual_seed(8))
    assert idx.dtype == torch.int32 and idx.shape == (40,)
    assert torch.equal(idx, torch.randint(0, 7, (40,), generator=torch.Generator().manual_seed(8), dtype=torch.int32))
    assert torch.equal(rv.check((40, 100), None, seed=8), idx), "the default rooms of a call are sample_index's from its seed"
    with pytest.raises(ValueError, match="call make_rirs first"):
        _reverb(rooms=0).sample_index(4, torch.Generator())


def test_check_params_forms_the_kernel_table():
    rv = _reverb()
    p = rv.check_params(2, torch.tensor([0.25, 0.5]), 6.0, torch.tensor([3, 40], dtype=torch.int32))
    assert p.dtype == torch.float64 and p.shape == (2, 3) and p.is_contiguous()
    assert p[:, 0].tolist() == [math.log(1000.0) / (0.25 * 16000), math.log(1000.0) / (0.5 * 16000)]
    assert p[:, 1].tolist() == [10.0 ** 0.6] * 2 and p[:, 2].tolist() == [3.0, 40.0]
    assert p[0, 0].item() == tw.lam_of(0.25, 16000)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,match", [
    (dict(rir_len=0), "rir_len must be a positive integer"), (dict(rir_len=2.0), "rir_len must be a positive integer"),
    (dict(rir_len=32769), "at most 32768"), (dict(rir_len=8, sr=0), "sr must be a positive number"),
    (dict(rir_len=8, rt60=(0.5, 0.2)), "rt60 must be a finite positive range"), (dict(rir_len=8, rt60=(0.0, 0.2)), "rt60 must be a finite positive range"),
    (dict(rir_len=8, drr_db=(0.0, math.inf)), "drr_db must be a finite range"), (dict(rir_len=8, drr_db=(math.nan, 1.0)), "drr_db must be a finite range"),
    (dict(rir_len=8, predelay_ms=(5.0, 1.0)), "predelay_ms must be a finite range"), (dict(rir_len=8, predelay_ms=(-1.0, 1.0)), "must not be negative"),
])
def test_constructor_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        Reverb(device="cpu", **kw)


def test_make_rirs_refusals_come_before_any_device_work():
    rv = _reverb(rooms=0)
    for kw, match in ((dict(n=0), "n must be a positive integer"), (dict(n=(1 << 19) + 1), "at most 524288"), (dict(n=2, seed=-1), "seed must be"),
                      (dict(n=2, rt60=0.0), "rt60 must be finite and positive"), (dict(n=2, rt60=[0.1, math.inf]), "rt60 must be finite and positive"),
                      (dict(n=2, rt60=[0.1, 0.2, 0.3]), "rt60 must be a number or hold 2 values"), (dict(n=2, drr_db=math.nan), "drr_db must be finite"),
                      (dict(n=2, drr_db=4000.0), "drr_db must be finite"), (dict(n=2, predelay=0), "at least 1 sample"),
                      (dict(n=2, predelay=1.5), "predelay must hold integers"),
                      (dict(n=2, noise=torch.zeros(2, K - 1)), "noise must be a float32"), (dict(n=2, noise=torch.zeros(2, K, dtype=torch.float64)), "noise must be a float32"),
                      (dict(n=2, noise=torch.zeros(K, 2).t()), "noise must be a float32"), (dict(n=2, noise=torch.zeros(1, K).expand(2, K)), "noise must be a float32")):
        with pytest.raises(ValueError, match=match):
            rv.make_rirs(**kw)
    assert rv.rirs is None
    with pytest.raises(_lib.MaavssError, match="MI355X only"):
        rv.make_rirs(2)                                # everything is in order: only the device is missing
    assert rv.rirs is None


def test_call_refusals_come_before_any_device_work():
    rv = _reverb(rooms=3)
    audio = torch.zeros(10, 50)[2:6]                     # 100 samples of storage in front of the first row
    ok = torch.tensor([0, 2, 1, 0], dtype=torch.int32)
    assert torch.equal(rv.check(audio, ok, lead=100), ok)
    for args, kw, match in (((torch.zeros(50),), {}, "audio must be float32"), ((torch.zeros(4, 50, dtype=torch.float64),), {}, "audio must be float32"),
                            ((torch.zeros(50, 4).t(),), {}, "audio must be float32"), ((torch.zeros(0, 50),), {}, "at least one clip"),
                            ((audio, ok[:3]), {}, r"rir_index must be an int32 \[4\]"), ((audio, ok.long()), {}, r"rir_index must be an int32 \[4\]"),
                            ((audio, torch.tensor([0, 3, 1, 0], dtype=torch.int32)), {}, r"must be in \[0, 3\), got \[0, 3\]"),
                            ((audio, torch.tensor([0, -1, 1, 0], dtype=torch.int32)), {}, r"must be in \[0, 3\)"),
                            ((audio, ok), dict(lead=-1), "lead must be a non-negative integer"), ((audio, ok), dict(lead=1.0), "lead must be"),
                            ((audio, ok), dict(lead=101), "lead=101: only 100 samples"), (((4, 50), ok), dict(lead=1), "lead needs the tensor")):
        with pytest.raises(ValueError, match=match):
            rv.check(*args, **kw)
        if isinstance(args[0], torch.Tensor):
            with pytest.raises(ValueError, match=match):
                rv(*args, **kw)
    with pytest.raises(ValueError, match="call make_rirs first"):
        _reverb(rooms=0)(audio)
    with pytest.raises(_lib.MaavssError, match="MI355X only"):
        rv(audio, ok, lead=100)


def _cpu_bank():
    bank = ClipBank(16, 5, 2, 8, 66, capacity_frames=64, capacity_samples=40000, device="cpu")
    g = torch.Generator().manual_seed(0)
    for frames in (9, 7):
        bank.add_recording(torch.rand(8000, generator=g), maps=torch.rand(frames, 4, generator=g))
    return bank


def test_bank_clips_refusals_and_floor():
    bank, rv = _cpu_bank(), _reverb(rooms=2)
    assert len(bank) == 5
    _, start = bank.check_indices([4, 0, 3, 2])
    floor = maavss_amd.reverb.bank_floor(bank, [4, 0, 3, 2])
    first = [bank.recordings[bank.locate(i)[0]][1] for i in (4, 0, 3, 2)]
    assert floor.dtype == torch.int64 and floor.tolist() == first and bool((floor <= start).all())
    assert torch.equal(maavss_amd.reverb.bank_floor(bank, torch.tensor([4, 0, 3, 2], dtype=torch.int32)), floor)
    n = bank.clip_samples
    for args, kw, match in ((([5],), {}, "clip indices must be in"), (([],), {}, "indices is empty"),
                            (([0, 1], torch.tensor([0, 2], dtype=torch.int32)), {}, r"must be in \[0, 2\)"),
                            (([0, 1],), dict(out=torch.zeros(2, n - 1)), "out must be a float32"),
                            (([0, 1],), dict(out=torch.zeros(2, n, dtype=torch.float64)), "out must be a float32"),
                            (([0, 1],), dict(out=torch.zeros(1, n).expand(2, n)), "out must be a float32")):
        with pytest.raises((ValueError, IndexError), match=match):
            rv.bank_clips(bank, *args, **kw)
    with pytest.raises(_lib.MaavssError, match="MI355X only"):
        rv.bank_clips(bank, [0, 1])


def test_pipeline_argument_checks():
    st = maavss_amd.STFT(512, 66, device="cpu")
    rv = _reverb(rooms=3)
    with pytest.raises(ValueError, match="reverb_target must be 'wet' or 'dry'"):
        maavss_amd.ClipPipeline(None, st, 5, reverb=rv, reverb_target="both")
    with pytest.raises(ValueError, match="reverb_target='dry' together with mixer= is not built"):
        maavss_amd.ClipPipeline(None, st, 5, reverb=rv, reverb_target="dry", mixer=maavss_amd.Mixer(st))
    if not torch.cuda.is_available():
        return                                            # the constructor makes a side stream: the rest needs one
    pipe = maavss_amd.ClipPipeline(None, st, 5)
    with pytest.raises(ValueError, match="rir_index needs a ClipPipeline built with reverb="):
        pipe.check_reverb((4, 100), 0, torch.zeros(4, dtype=torch.int32))


def test_pipeline_check_reverb_draws_the_rooms_of_the_serial_call():
    pipe = object.__new__(maavss_amd.ClipPipeline)        # check_reverb reads self.reverb alone
    pipe.reverb = None
    assert pipe.check_reverb((4, 100), 0, None) is None
    with pytest.raises(ValueError, match="rir_index needs a ClipPipeline built with reverb="):
        pipe.check_reverb((4, 100), 0, torch.zeros(4, dtype=torch.int32))
    pipe.reverb = rv = _reverb(rooms=5)
    assert torch.equal(pipe.check_reverb((6, 100), 21, None), rv.sample_index(6, torch.Generator().manual_seed(21)))
    given = torch.tensor([4, 0, 4], dtype=torch.int32)
    assert torch.equal(pipe.check_reverb(torch.zeros(3, 100), 21, given), given)
    with pytest.raises(ValueError, match=r"must be in \[0, 5\)"):
        pipe.check_reverb((3, 100), 21, torch.tensor([4, 5, 0], dtype=torch.int32))
    with pytest.raises(ValueError, match="audio must be float32"):
        pipe.check_reverb(torch.zeros(3, 100, dtype=torch.float64), 21, None)
