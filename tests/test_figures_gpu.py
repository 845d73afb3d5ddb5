"""csrc/figures.hip on the GPU against the float64 twin (tests/figures_twin.py).

viridis_image, stft_panels and filmstrip_image are held to the twin byte for byte: the colour index is three f64 operations, each
rounded on its own on both sides (the file is compiled without contraction), and the scale-and-clip of the filmstrip is three f32
operations.  Shapes: 1x1, 3x5, 129x65, 257x64 (more than one workgroup) and 33x8385, whose pixel count is no multiple of the four
pixels a thread stores; strided, transposed, zero-stride and batched views; a sentinel in front of and behind the output.

specgram_planes differs from the twin by the transform's rounding, the order of the window sum and the last bit of cos, log10, hypot and
atan2.  The cases (figures_twin.gpu_cases: lengths 100 .. 8448 with five (nfft, noverlap) pairs, a silent stretch, a NaN sample,
overlapping rows at an odd 4-byte offset) have seeds chosen so that no decision lies within M = 1e-5 of a boundary
(tests/test_figures_cpu.py).  The gates were set from a measurement, as the rule was fixed beforehand: the largest |gpu - twin| over every
finite element of these cases on one MI355X (profiles/figures_parity.json, scripts/figures_parity.py), times 8, rounded up to a power of
ten; they had to come out at or below M / 10 = 1e-6 in LUT-index units and in radians, and did (MEASURED_* below).  Segment counts,
the places of -inf and NaN, and every pixel whose twin value is at least M from a colour boundary must equal the twin's exactly."""
import functools

import numpy as np
import pytest
import torch

import figures_twin as tw
import maavss_amd

pytestmark = pytest.mark.gpu

MEASURED_MAG_DB = 6.39e-11         # profiles/figures_parity.json: max_mag_db_abs_diff (6.382e-11 dB, at L1000_n64_o63)
MEASURED_PHASE_RAD = 2.88e-13      # max_phase_rad_abs_diff (2.878e-13 rad, at L8448_n64_o63)
MEASURED_INDEX = 1.52e-10          # the larger of max_mag_index_diff (1.516e-10) and max_phase_index_diff (6.77e-13)
GATE_MAG_DB = 1e-9                 # 8 x 6.39e-11 = 5.1e-10, rounded up to a power of ten
GATE_PHASE_RAD = 1e-11             # 8 x 2.88e-13 = 2.3e-12
GATE_INDEX = 1e-8                  # 8 x 1.52e-10 = 1.2e-9
assert GATE_INDEX <= tw.M / 10 and GATE_PHASE_RAD <= tw.M / 10


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _place(rows, stride, off):
    """rows [B, L] numpy f32 -> a device view [B, L] with row stride `stride` whose first element is `off` elements past a 256-byte
    boundary."""
    b, n = rows.shape
    flat = np.zeros(off + (b - 1) * stride + n + 8, dtype=np.float32)
    for i in range(b):
        flat[off + i * stride:off + i * stride + n] = rows[i]
    dev = torch.from_numpy(flat).cuda()
    assert dev.data_ptr() % 256 == 0
    return dev.as_strided((b, n), (stride, 1), off)


# ---- viridis_image ----------------------------------------------------------------------------------------------------------------------

SHAPES = ((1, 1), (3, 5), (129, 65), (257, 64), (33, 8385))


def _image(shape, dtype, seed=0):
    x = np.random.default_rng(seed).standard_normal(shape)
    return x.astype(dtype)


def _check(x_dev, x_host, **kw):
    got = _host(maavss_amd.viridis_image(x_dev, **kw))
    want = tw.viridis_image(x_host, **kw)
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.shape, want.shape)
    differing = int((got != want).any(axis=-1).sum())
    assert differing == 0, f"{differing} of {want.shape[0] * want.shape[1]} pixels differ"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_viridis_image_is_the_twin_byte_for_byte(shape, dtype):
    x = _image(shape, dtype, seed=shape[1])
    _check(torch.from_numpy(x).cuda(), x)
    _check(torch.from_numpy(x).cuda(), x, vmin=-1.0, vmax=1.0)                          # fixed range, values beyond both ends
    _check(torch.from_numpy(x).cuda(), x, transpose=True, flip_rows=True, scale=(2, 3))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_viridis_image_takes_views_as_they_are(dtype):
    big = _image((2 * 129 + 1, 3 * 65 + 2), dtype, seed=5)
    dev = torch.from_numpy(big).cuda()
    _check(dev[1::2, 2::3], big[1::2, 2::3])                                              # element strides 2 x 3
    _check(dev.t(), big.T)                                                                 # a transposed view: column stride = a row
    _check(dev.t()[::3], big.T[::3], flip_rows=True)
    _check(dev[1::2, 2::3], big[1::2, 2::3], transpose=True, scale=(1, 2))
    _check(dev[3:4].expand(7, -1), np.broadcast_to(big[3:4], (7, big.shape[1])))          # stride 0
    _check(dev[:, 4:5].expand(-1, 6), np.broadcast_to(big[:, 4:5], (big.shape[0], 6)), vmin=0.0)      # one end fixed, one autoscaled
    _check(dev[1::2, 2::3], big[1::2, 2::3], vmax=0.5)
    stft = _image((3, 2, 24, 129), np.float32, seed=6)
    if dtype == np.float32:
        _check(torch.from_numpy(stft).cuda()[1, 0], stft[1, 0], transpose=True)           # y_stft[b, 0] needs no copy


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_viridis_image_special_images(dtype):
    g = np.random.default_rng(9)
    bad = g.standard_normal((33, 41)).astype(dtype)
    bad[3, 4], bad[10, 0], bad[32, 40], bad[0, :3] = np.nan, np.inf, -np.inf, np.nan
    _check(torch.from_numpy(bad).cuda(), bad)
    _check(torch.from_numpy(bad).cuda(), bad, vmin=-1.0, vmax=1.0, scale=(2, 3))
    got = _host(maavss_amd.viridis_image(torch.from_numpy(bad).cuda()))
    assert not got[3, 4].any() and not got[10, 0].any() and not got[32, 40].any() and (got[5, 5, 3] == 255)
    const = np.full((5, 7), -2.25, dtype=dtype)
    _check(torch.from_numpy(const).cuda(), const)
    assert (_host(maavss_amd.viridis_image(torch.from_numpy(const).cuda()))[..., :3] == tw.lut()[0]).all()
    none = np.array([[np.nan, np.inf], [-np.inf, np.nan], [np.nan, np.nan]], dtype=dtype)
    _check(torch.from_numpy(none).cuda(), none)
    assert not _host(maavss_amd.viridis_image(torch.from_numpy(none).cuda())).any()
    ramp = np.linspace(0.0, 1.0, 256 * 8 + 1, dtype=np.float64)[None, :].astype(dtype)    # the boundaries k / 256 themselves
    _check(torch.from_numpy(ramp).cuda(), ramp)
    _check(torch.from_numpy(ramp).cuda(), ramp, vmin=0.0, vmax=1.0)


@pytest.mark.parametrize("shape,scale", [((3, 5), (1, 1)), ((33, 8385), (1, 1)), ((129, 65), (2, 3)), ((1, 1), (1, 1))])
def test_viridis_image_leaves_a_sentinel_around_its_output(shape, scale):
    x = _image(shape, np.float32, seed=3)
    h, w = shape[0] * scale[0], shape[1] * scale[1]
    total = h * w * 4
    for lead in (64, 68):                                                                  # 16-byte aligned (wide stores), and 4 bytes off
        flat = torch.full((lead + total + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        out = flat[lead:lead + total].view(h, w, 4)
        res = maavss_amd.viridis_image(torch.from_numpy(x).cuda(), scale=scale, out=out)
        assert res is out
        got = _host(flat)
        assert (got[:lead] == 0xAB).all() and (got[lead + total:] == 0xAB).all()
        assert np.array_equal(got[lead:lead + total].reshape(h, w, 4), tw.viridis_image(x, scale=scale))


def test_viridis_image_batch_equals_single_calls():
    x = _image((5, 37, 53), np.float64, seed=11)
    x[1] *= 100.0
    x[2, 4, 4] = np.nan
    x[3] = 2.0
    x[4] = np.nan
    dev = torch.from_numpy(x).cuda()
    got = _host(maavss_amd.viridis_image(dev, scale=(1, 2)))
    assert got.shape == (5, 37, 106, 4)
    for i in range(5):
        assert np.array_equal(got[i], _host(maavss_amd.viridis_image(dev[i], scale=(1, 2))))
        assert np.array_equal(got[i], tw.viridis_image(x[i], scale=(1, 2)))
    every_other = _host(maavss_amd.viridis_image(dev[::2]))                              # batch stride of two images
    assert np.array_equal(every_other, np.stack([tw.viridis_image(x[i]) for i in (0, 2, 4)]))


# ---- specgram_planes and specgram_images ------------------------------------------------------------------------------------------------

def _compare(name, got_mag, got_phase, got_imgs, x, nfft, nov):
    want_mag, want_phase = tw.specgram_planes(x, nfft, nov)
    row = dict(case=name, segments=int(got_mag.shape[1]), segments_equal=bool(got_mag.shape == want_mag.shape == got_phase.shape))
    if not row["segments_equal"]:
        return row
    want_imgs = tw.specgram_images(x, nfft, nov)
    for key, unit, got, want, gi, wi in (("mag", "db", got_mag, want_mag, got_imgs[0], want_imgs[0]),
                                         ("phase", "rad", got_phase, want_phase, got_imgs[1], want_imgs[1])):
        fin = np.isfinite(want)
        same_kind = np.array_equal(fin, np.isfinite(got)) and np.array_equal(np.isnan(want), np.isnan(got)) and np.array_equal(want[~fin & ~np.isnan(want)], got[~fin & ~np.isnan(want)])
        diff = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
        lo, hi = tw.finite_range(want)
        differ = (gi != wi).any(axis=-1)
        undecided = tw.boundary_margin(want) < tw.M
        row.update({f"{key}_nonfinite_equal": bool(same_kind), f"{key}_{unit}_abs_diff": diff,
                    f"{key}_index_diff": 256.0 * diff / (hi - lo) if hi > lo else 0.0, f"{key}_pixels": int(want.size),
                    f"{key}_pixels_differing": int(differ.sum()), f"{key}_decided_pixels_differing": int((differ & ~undecided).sum()),
                    f"{key}_undecided": int(undecided.sum())})
    return row


@functools.lru_cache(maxsize=None)
def measure_planes():
    """Every spectrogram case once -> a list of dicts (scripts/figures_parity.py writes them out)."""
    rows = []
    for k, (name, x, nfft, nov) in enumerate(tw.gpu_cases()):
        wave = _place(x[None], len(x) + 5, 1 + k % 3)                                      # 1, 2, 3 elements off a 16-byte boundary
        mag, phase = maavss_amd.specgram_planes(wave, nfft, nov)
        assert mag.dtype == phase.dtype == torch.float64 and mag.is_cuda and mag.shape[0] == 1 and tuple(mag.shape) == tuple(phase.shape)
        imgs = maavss_amd.specgram_images(wave, nfft, nov)
        rows.append(_compare(name, _host(mag)[0], _host(phase)[0], [_host(i)[0] for i in imgs], x, nfft, nov))
    o = tw.OVERLAP                                                                         # overlapping rows from an odd 4-byte offset
    sig = torch.from_numpy(tw.overlap_signal()).cuda()
    wave = sig.as_strided((o["rows"], o["n"]), (o["stride"], 1), o["off"])
    assert wave.data_ptr() % 8 == 4
    mag, phase = maavss_amd.specgram_planes(wave, o["nfft"], o["noverlap"])
    imgs = [_host(i) for i in maavss_amd.specgram_images(wave, o["nfft"], o["noverlap"])]
    mag, phase = _host(mag), _host(phase)
    for r, x in enumerate(tw.overlap_rows()):
        rows.append(_compare(f"overlap{r}", mag[r], phase[r], [i[r] for i in imgs], x, o["nfft"], o["noverlap"]))
    one = maavss_amd.specgram_planes(sig[o["off"]:o["off"] + o["n"]], o["nfft"], o["noverlap"])      # a [L] wave is one row
    assert np.array_equal(_host(one[0])[0], mag[0]) and np.array_equal(_host(one[1])[0], phase[0])
    return rows


def test_specgram_segment_counts_and_nonfinite_places_equal_the_twins():
    rows = measure_planes()
    assert len(rows) == len(tw.LENGTHS) * len(tw.PARAMS) + 2 + tw.OVERLAP["rows"]
    for r in rows:
        assert r["segments_equal"], r
        assert r["mag_nonfinite_equal"] and r["phase_nonfinite_equal"], r
    by = {r["case"]: r for r in rows}
    assert by["L100_n256_o128"]["segments"] == 1 and by["L383_n256_o128"]["segments"] == 1 and by["L384_n256_o128"]["segments"] == 2
    assert by["L8448_n64_o63"]["segments"] == 8385


def test_specgram_planes_are_within_the_measured_gate_of_the_twin():
    rows = measure_planes()
    worst = {k: max(rows, key=lambda r: r[k]) for k in ("mag_db_abs_diff", "phase_rad_abs_diff", "mag_index_diff", "phase_index_diff")}
    for k, r in worst.items():
        print(f"largest {k}: {r[k]:.3e} at {r['case']}")
    for r in rows:
        assert r["mag_db_abs_diff"] <= GATE_MAG_DB, r
        assert r["phase_rad_abs_diff"] <= GATE_PHASE_RAD, r
        assert r["mag_index_diff"] <= GATE_INDEX and r["phase_index_diff"] <= GATE_INDEX, r


def test_specgram_images_equal_the_twins_on_every_decided_pixel():
    rows = measure_planes()
    print("pixels differing from the twin:", sum(r["mag_pixels_differing"] + r["phase_pixels_differing"] for r in rows),
          "of", sum(r["mag_pixels"] + r["phase_pixels"] for r in rows))
    for r in rows:
        for key in ("mag", "phase"):
            assert r[f"{key}_decided_pixels_differing"] == 0, r
            assert r[f"{key}_undecided"] <= tw.undecided_cap(r[f"{key}_pixels"]), r
            assert r[f"{key}_pixels_differing"] <= r[f"{key}_undecided"], r


def test_specgram_special_rows():
    silent, nan = (tw.special_row(k) for k in ("silent", "nan"))
    mag, phase = (_host(p) for p in maavss_amd.specgram_planes(torch.from_numpy(np.stack([silent, nan])).cuda(), 256, 128))
    assert np.isneginf(mag[0][:, 4:7]).all() and (phase[0][:, 4:7] == 0).all() and np.isfinite(mag[0][:, [3, 7]]).all()
    assert np.isnan(mag[1][:, 4:6]).all() and np.isnan(phase[1][:, 4:6]).all()
    assert np.isfinite(mag[1][:, [3, 6]]).all() and np.isfinite(phase[1][:, [3, 6]]).all()
    imgs = [_host(i) for i in maavss_amd.specgram_images(torch.from_numpy(np.stack([silent, nan])).cuda(), 256, 128, scale=(1, 2))]
    assert imgs[0].shape == (2, 129, 2 * 14, 4) and not imgs[0][0][:, 8:14].any() and (imgs[0][0][:, 6:8, 3] == 255).all()
    assert not imgs[0][1][:, 8:12].any() and not imgs[1][1][:, 8:12].any() and (imgs[1][0][..., 3] == 255).all()


def test_specgram_two_runs_give_the_same_bytes():
    x = torch.from_numpy(np.stack([tw.tone_noise(8448, 5), tw.tone_noise(8448, 6)])).cuda()
    a = [_host(p) for p in maavss_amd.specgram_planes(x, 512, 128)]
    b = [_host(p) for p in maavss_amd.specgram_planes(x, 512, 128)]
    assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


# ---- the reference's composites -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 8, 257), (2, 32, 129)], ids=lambda s: "x".join(map(str, s)))
def test_stft_panels_are_the_twins(shape):
    g = np.random.default_rng(shape[1])
    batch = g.standard_normal((3, 2, shape[1] + 5, shape[2])).astype(np.float32)          # the panels are slices of a batch: no copy is made
    batch[1, 1] *= 30.0
    out_b = (0.1 * g.standard_normal((3,) + shape)).astype(np.float32)
    y_dev, yh_dev = torch.from_numpy(batch).cuda()[1, :, 2:2 + shape[1]], torch.from_numpy(out_b).cuda()[2]
    assert not y_dev.is_contiguous()
    got = _host(maavss_amd.stft_panels(y_dev, yh_dev))
    want = tw.stft_panels(batch[1, :, 2:2 + shape[1]], out_b[2])
    assert got.shape == (4, shape[2], shape[1], 4) and np.array_equal(got, want)
    assert np.array_equal(_host(y_dev), batch[1, :, 2:2 + shape[1]])


def _film_inputs(t, h, w, seed, kind="random"):
    g = np.random.default_rng(seed)
    y = g.random((1, t, h, w)).astype(np.float32)
    yh = (g.random((1, t, h, w)) * 1.4 - 0.2).astype(np.float32)                           # some below 0: clipped
    video = g.random((3, t, h, w)).astype(np.float32)
    if kind == "zero":
        y[:] = 0.0                                                                         # max 0: s = 1e7 and zeros stay zeros
    if kind == "above_one":
        y *= 7.5                                                                           # values above 1 before scaling
        video *= 255.0
    return y, yh, video


@pytest.mark.parametrize("with_video", [True, False], ids=["video", "no_video"])
@pytest.mark.parametrize("t,h,w,kind", [(1, 8, 8, "random"), (4, 8, 8, "zero"), (4, 16, 24, "random"), (1, 16, 24, "above_one"),
                                         (4, 224, 224, "above_one"), (1, 224, 224, "zero"), (3, 5, 7, "random")],
                         ids=lambda v: str(v))
def test_filmstrip_image_is_the_twin_byte_for_byte(t, h, w, kind, with_video):
    y, yh, video = _film_inputs(t, h, w, seed=t * 1000 + h + w, kind=kind)
    if not with_video:
        video = None
    dev = [None if a is None else torch.from_numpy(a).cuda() for a in (y, yh, video)]
    got = _host(maavss_amd.filmstrip_image(*dev))
    want = tw.filmstrip_image(y, yh, video)
    assert got.shape == ((3 if with_video else 2) * h, t * w, 4) and got.dtype == np.uint8
    differing = int((got != want).any(axis=-1).sum())
    assert differing == 0, f"{differing} pixels differ"
    for a, d in zip((y, yh, video), dev):                                                  # the reference scales its arguments in place; this does not
        assert a is None or np.array_equal(_host(d), a)
    if kind == "zero":
        rows = slice(h, 2 * h) if with_video else slice(0, h)
        assert (got[rows, :, :3] == tw.lut()[128]).all()


# ---- CallbackFigures and save_png -------------------------------------------------------------------------------------------------------

T, W, FFT, HPF, S, B = 8, 128, 256, 8, 3, 2                                                # the small shape of tests/test_enhance_gpu.py


@functools.lru_cache(maxsize=None)
def _callback_setup():
    from oracle import avse_ref_cpu as orc
    hop, _, t_a = maavss_amd.calc_hop_size(T, HPF, 30, 16000)
    shapes = ([B, 2, t_a, FFT // 2 + 1], [B, 1, T, W, W], HPF)
    model = maavss_amd.AV_Fusion_Model_Frames(*shapes)
    model.load_state_dict(orc.seeded_state_dict(orc.AVFusionFramesRef(*shapes), 11), strict=True)
    model = model.cuda().train()
    stft = maavss_amd.STFT(FFT, hop, device="cuda")
    g = torch.Generator().manual_seed(31)
    t_tot = T + S - 1
    audio = (0.3 * torch.randn(B, HPF * hop * t_tot, generator=g)).clamp(-1, 1).cuda()
    x_stft, y_stft = stft(audio, seed=1)
    attn = torch.rand(B, 1, t_tot, W, W, generator=g).cuda()
    video = torch.rand(B, 3, t_tot, W, W, generator=g).cuda()
    step = maavss_amd.TrainStep(model, lr=1e-4, loss_coeff=0.001, num_seq=S)
    _, out_stft, out_attn = step.sliding_window_step(x_stft, y_stft, attn, attn, T, HPF, collect=True)
    torch.cuda.synchronize()
    return stft, hop, y_stft, out_stft, attn, out_attn, video


def test_callback_figures_launch_only_and_equal_the_single_functions():
    stft, hop, y_stft, out_stft, attn, out_attn, video = _callback_setup()
    figures = maavss_amd.CallbackFigures(stft, scale=(1, 2))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first = figures(y_stft, out_stft, attn, out_attn, video=video, clip=1)
        second = figures(y_stft, out_stft, attn, out_attn, video=video, clip=1)
        plain = figures(y_stft, out_stft, attn, out_attn, clip=0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    keys = ("stft", "input_mag", "input_phase", "output_mag", "output_phase", "attention_frames", "audio_input", "audio_output")
    assert tuple(first) == keys and tuple(plain) == keys
    rows, mid, n_wave = HPF * S, (S - 1) // 2, hop * (HPF * S - 1)
    n_seg = tw.segments(n_wave, 256, 128)
    want_shapes = dict(stft=(4, FFT // 2 + 1, rows, 4), attention_frames=(3 * W, S * W, 4), audio_input=(n_wave,), audio_output=(n_wave,))
    want_shapes.update({k: (129, 2 * n_seg, 4) for k in ("input_mag", "input_phase", "output_mag", "output_phase")})
    for k in keys:
        assert first[k].is_cuda and tuple(first[k].shape) == want_shapes[k], (k, tuple(first[k].shape))
        assert first[k].dtype == (torch.float32 if k.startswith("audio") else torch.uint8), k
        assert torch.equal(first[k], second[k]), k                                         # two calls: identical bytes
    assert tuple(plain["attention_frames"].shape) == (2 * W, S * W, 4)
    # the single functions on the tensors the reference cuts (train_avse_frames.py:195-200)
    y = y_stft[1, :, mid * HPF:mid * HPF + rows]
    a, v = attn[1, :, mid:mid + S], video[1, :, mid:mid + S]
    assert torch.equal(first["stft"], maavss_amd.stft_panels(y, out_stft[1]))
    assert torch.equal(first["attention_frames"], maavss_amd.filmstrip_image(a, out_attn[1], v))
    waves = stft.inverse(torch.stack((y, out_stft[1])))
    assert torch.equal(first["audio_input"], waves[0]) and torch.equal(first["audio_output"], waves[1])
    for name, wave in (("input", first["audio_input"]), ("output", first["audio_output"])):
        mag, phase = maavss_amd.specgram_images(wave, scale=(1, 2))
        assert torch.equal(first[f"{name}_mag"], mag) and torch.equal(first[f"{name}_phase"], phase)
    # and against the twin, from the waveform on: decided pixels equal
    x = _host(first["audio_input"])
    want = tw.specgram_images(x, scale=(1, 2))
    planes = tw.specgram_planes(x)
    for got, img, plane in zip((first["input_mag"], first["input_phase"]), want, planes):
        decided = np.repeat(tw.boundary_margin(plane) >= tw.M, 2, axis=1)
        assert np.array_equal(_host(got)[decided], img[decided])
    assert np.array_equal(_host(first["stft"]), tw.stft_panels(_host(y), _host(out_stft[1])))


def test_save_png_round_trips_through_pil(tmp_path):
    from PIL import Image
    stft, hop, y_stft, out_stft, attn, out_attn, video = _callback_setup()
    figs = maavss_amd.CallbackFigures(stft)(y_stft, out_stft, attn, out_attn, video=video)
    paths = maavss_amd.save_png(figs, str(tmp_path / "figures"), 7)
    assert sorted(p.split("/")[-1] for p in paths) == sorted(f"{k}_000007.png" for k in figs if not k.startswith("audio"))
    for p in paths:
        key = p.split("/")[-1][:-len("_000007.png")]
        back = np.asarray(Image.open(p))
        want = _host(figs[key])
        if want.ndim == 4:                                                                 # the four STFT panels side by side
            want = np.concatenate(list(want), axis=1)
        assert back.dtype == np.uint8 and np.array_equal(back, want), key
