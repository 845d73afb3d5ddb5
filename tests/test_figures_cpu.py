"""CPU-only: the float64 twin of csrc/figures.hip (tests/figures_twin.py) held to matplotlib itself, the committed colour table held to
matplotlib's, the conditions the GPU tests' inputs have to meet, and the entry points' argument checks.

The twin restates include/maavss.h; what it is compared with here is what the reference's callback ends in (utilities.py:336-350
plt.imshow(...), :316 imshow(..., vmin=-1, vmax=1), :398 / :409 Axes.specgram(..., mode=...)): cm.viridis(Normalize(vmin, vmax)(...),
bytes=True), matplotlib.mlab.specgram and the image Axes.specgram makes."""
import ctypes

import numpy as np
import pytest
from matplotlib import cm, mlab
from matplotlib.colors import Normalize
from matplotlib.figure import Figure

import figures_twin as tw
from maavss_amd import _lib


def _mpl_colour(x, vmin=None, vmax=None):
    with np.errstate(all="ignore"):
        return cm.viridis(Normalize(vmin, vmax)(np.ma.masked_invalid(np.asarray(x).astype(np.float64))), bytes=True)


def test_committed_lut_is_matplotlibs_viridis():
    want = (np.asarray(cm.viridis.colors) * 255).astype(np.uint8)
    got = tw.read_lut()
    assert got.shape == (256, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want)


def _images():
    g = np.random.default_rng(0)
    out = {"random_f64": g.standard_normal((37, 53)), "random_f32": g.standard_normal((129, 65)).astype(np.float32),
           "wide_range": g.standard_normal((16, 16)) * 1e6, "one_pixel": np.array([[3.5]]), "constant": np.full((5, 7), -2.25, dtype=np.float32),
           "all_nan": np.full((4, 6), np.nan), "two_values": np.array([[0.0, 1.0], [1.0, 0.0]])}
    bad = g.standard_normal((33, 41))
    bad[3, 4], bad[10, 0], bad[32, 40], bad[0, :3] = np.nan, np.inf, -np.inf, np.nan
    out["non_finite"] = bad
    out["all_non_finite"] = np.array([[np.nan, np.inf], [-np.inf, np.nan]])
    ramp = np.linspace(0.0, 1.0, 256 * 8 + 1)[None, :]                                 # every boundary k / 256 is hit exactly
    out["ramp"] = ramp
    return out


@pytest.mark.parametrize("name", sorted(_images()))
def test_twin_colouring_is_matplotlibs_autoscaled(name):
    x = _images()[name]
    assert np.array_equal(tw.viridis_image(x), _mpl_colour(x))


@pytest.mark.parametrize("name", ["random_f64", "random_f32", "non_finite", "ramp", "constant"])
def test_twin_colouring_is_matplotlibs_with_a_fixed_range(name):
    x = _images()[name] * 1.7                                                          # values below -1 and above 1: the end colours
    got = tw.viridis_image(x, vmin=-1.0, vmax=1.0)
    assert np.array_equal(got, _mpl_colour(x, -1.0, 1.0))
    finite = np.isfinite(x)
    assert np.array_equal(got[finite & (x < -1)][:, :3], np.broadcast_to(tw.lut()[0], (int((finite & (x < -1)).sum()), 3)))
    assert np.array_equal(got[finite & (x > 1)][:, :3], np.broadcast_to(tw.lut()[255], (int((finite & (x > 1)).sum()), 3)))


def test_twin_special_images_are_as_the_definition_states():
    assert np.array_equal(tw.viridis_image(np.array([[np.nan, 1.0, np.inf, -np.inf]]))[0, [0, 2, 3]], np.zeros((3, 4), dtype=np.uint8))
    assert np.array_equal(tw.viridis_image(np.full((2, 2), 7.0)), np.broadcast_to(np.append(tw.lut()[0], 255).astype(np.uint8), (2, 2, 4)))
    assert not tw.viridis_image(np.full((3, 3), np.nan)).any()
    img = tw.viridis_image(np.array([[0.0, 0.5, 1.0]]))
    assert np.array_equal(img[0, :, :3], tw.lut()[[0, 128, 255]]) and (img[..., 3] == 255).all()
    x = np.arange(6.0).reshape(2, 3)
    assert np.array_equal(tw.viridis_image(x, transpose=True, flip_rows=True, scale=(2, 3)),
                          np.repeat(np.repeat(tw.viridis_image(x.T[::-1]), 2, axis=0), 3, axis=1))


CASES = tw.gpu_cases()
ROWS = [(name, x, nfft, nov) for name, x, nfft, nov in CASES] + [(f"overlap{r}", row, tw.OVERLAP["nfft"], tw.OVERLAP["noverlap"])
                                                                 for r, row in enumerate(tw.overlap_rows())]


def _close(got, want, tol):
    """Equal where either is non-finite (same infinities, NaN where NaN), within tol elsewhere."""
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    assert np.array_equal(np.isnan(want), np.isnan(got)) and np.array_equal(want[~fin & ~np.isnan(want)], got[~fin & ~np.isnan(got)])
    return float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0


@pytest.mark.filterwarnings("ignore:Only one segment is calculated")      # a signal no longer than nfft: the case is wanted
@pytest.mark.parametrize("case", ROWS, ids=[c[0] for c in ROWS])
def test_twin_planes_are_mlab_specgrams(case):
    name, x, nfft, nov = case
    mag, phase = tw.specgram_planes(x, nfft, nov)
    n = tw.segments(len(x), nfft, nov)
    assert mag.shape == phase.shape == (nfft // 2 + 1, n)
    with np.errstate(all="ignore"):
        m_ref = mlab.specgram(x.astype(np.float64), NFFT=nfft, noverlap=nov, mode="magnitude")[0]
        p_ref = mlab.specgram(x.astype(np.float64), NFFT=nfft, noverlap=nov, mode="phase")[0]
        m_ref = 20.0 * np.log10(m_ref)[::-1]
    err_m, err_p = _close(mag, m_ref, 1e-12), _close(phase, p_ref[::-1], 1e-12)
    print(f"{name}: |twin - mlab| mag {err_m:.2e} dB, phase {err_p:.2e} rad")
    assert err_m <= 1e-12 and err_p <= 1e-12


@pytest.mark.filterwarnings("ignore:Only one segment is calculated")      # a signal no longer than nfft: the case is wanted
@pytest.mark.parametrize("case", ROWS, ids=[c[0] for c in ROWS])
def test_twin_images_are_the_images_axes_specgram_makes(case):
    name, x, nfft, nov = case
    got = tw.specgram_images(x, nfft, nov)
    ax = Figure().subplots()
    for img, mode in zip(got, ("magnitude", "phase")):
        with np.errstate(all="ignore"):
            im = ax.specgram(x.astype(np.float64), NFFT=nfft, noverlap=nov, mode=mode)[3]
            want = im.cmap(im.norm(im.get_array()), bytes=True)
        differing = int((img != want).any(axis=-1).sum())
        print(f"{name} {mode}: {differing} of {want.shape[0] * want.shape[1]} pixels differ")
        assert differing == 0


@pytest.mark.parametrize("case", ROWS, ids=[c[0] for c in ROWS])
def test_gpu_case_inputs_keep_their_decisions_a_margin_away(case):
    """What lets the GPU tests ask for equal decisions: every unwrap decision at least M from pi, and at most max(2, pixels / 32768)
    pixels of a plane within M (LUT-index units) of a colour boundary.  The seeds in figures_twin.py were chosen for this."""
    name, x, nfft, nov = case
    m = tw.case_margins(x, nfft, nov)
    print(f"{name}: unwrap margin {m['unwrap']:.3e}, undecided pixels mag {m['mag']}, phase {m['phase']}")
    assert m["unwrap"] >= tw.M
    for key in ("mag", "phase"):
        assert m[key][0] <= tw.undecided_cap(m[key][1]), (key, m[key])


def test_special_rows_hold_what_they_are_for():
    rows = tw.special_rows()
    mag, phase = tw.specgram_planes(rows["silent"], 256, 128)
    assert np.isneginf(mag[:, 4]).all() and (phase[:, 4] == 0).all() and np.isfinite(mag[:, 2]).all() and np.isfinite(mag[:, 7]).all()
    mag, phase = tw.specgram_planes(rows["nan"], 256, 128)
    nan_cols = np.isnan(mag).all(axis=0)
    assert np.array_equal(np.nonzero(nan_cols)[0], [4, 5]) and np.array_equal(np.isnan(phase).all(axis=0), nan_cols)
    assert np.isfinite(mag[:, ~nan_cols]).all()


def test_twin_composites():
    g = np.random.default_rng(3)
    y, yh = g.standard_normal((2, 8, 17)).astype(np.float32), g.standard_normal((2, 8, 17)).astype(np.float32)
    panels = tw.stft_panels(y, yh)
    assert panels.shape == (4, 17, 8, 4)
    assert np.array_equal(panels[1], _mpl_colour(y[1].T)) and np.array_equal(panels[2], _mpl_colour(yh[0].T))
    a, ah, v = g.random((1, 4, 6, 10)).astype(np.float32) * 3, g.random((1, 4, 6, 10)).astype(np.float32), g.random((3, 4, 6, 10)).astype(np.float32)
    keep = [t.copy() for t in (a, ah, v)]
    strip = tw.filmstrip_image(a, ah, v)
    assert strip.shape == (18, 40, 4) and all(np.array_equal(k, t) for k, t in zip(keep, (a, ah, v)))
    # the reference's own arithmetic, float32 in place, and imshow's mapping of it
    ya = a.copy()
    ya *= np.float32(1) / (ya.max() + np.float32(1e-7))
    ya = np.clip(ya, 0.0, 1.0)
    assert np.array_equal(strip[6:12, 10:20], _mpl_colour(ya[0, 1], -1.0, 1.0))
    vv = v.copy()
    vv *= np.float32(1) / (vv.max() + np.float32(1e-7))
    vv = np.clip(vv, 0.0, 1.0)
    rgb = cm.ScalarMappable().to_rgba(np.moveaxis(vv[:, 2], 0, -1), bytes=True)
    assert np.array_equal(strip[0:6, 20:30], rgb)
    assert (strip[6:, :, :3] != tw.lut()[0]).any() and tw.filmstrip_image(a, ah).shape == (12, 40, 4)
    zero = tw.filmstrip_image(np.zeros((1, 1, 2, 2), np.float32), ah[:, :1, :2, :2])
    assert np.array_equal(zero[:2, :, :3], np.broadcast_to(tw.lut()[128], (2, 2, 3)))      # zeros stay zeros: the middle of the map


def test_figure_entry_points_validate_their_arguments_before_touching_the_device():
    """As tests/test_abi_cpu.py does it: every call fails its argument check (fake non-null pointers are never dereferenced)."""
    p = 256
    with pytest.raises(_lib.MaavssError, match="viridis_range: null pointer"):
        _lib.call("maavss_viridis_range", None, 0, 1, 4, 4, 0, 4, 1, p, None)
    with pytest.raises(_lib.MaavssError, match="viridis_range: null pointer"):
        _lib.call("maavss_viridis_range", p, 0, 1, 4, 4, 0, 4, 1, None, None)
    with pytest.raises(_lib.MaavssError, match="viridis_image: null pointer"):
        _lib.call("maavss_viridis_image", p, 0, 1, 4, 4, 0, 4, 1, p, 0, 0.0, 0.0, 0, 0, 1, 1, None, None)
    with pytest.raises(_lib.MaavssError, match="null pointer .the range"):
        _lib.call("maavss_viridis_image", p, 0, 1, 4, 4, 0, 4, 1, None, 1, 0.0, 0.0, 0, 0, 1, 1, p, None)
    for h, w, n in ((0, 4, 1), (4, 0, 1), (4, 4, 0)):
        with pytest.raises(_lib.MaavssError, match="zero-sized image"):
            _lib.call("maavss_viridis_range", p, 0, n, h, w, 0, 4, 1, p, None)
        with pytest.raises(_lib.MaavssError, match="zero-sized image"):
            _lib.call("maavss_viridis_image", p, 0, n, h, w, 0, 4, 1, p, 0, 0.0, 0.0, 0, 0, 1, 1, p, None)
    with pytest.raises(_lib.MaavssError, match="dtype 2"):
        _lib.call("maavss_viridis_range", p, 2, 1, 4, 4, 0, 4, 1, p, None)
    with pytest.raises(_lib.MaavssError, match="strides"):
        _lib.call("maavss_viridis_range", p, 0, 1, 4, 4, 0, -4, 1, p, None)
    with pytest.raises(_lib.MaavssError, match="scale"):
        _lib.call("maavss_viridis_image", p, 0, 1, 4, 4, 0, 4, 1, p, 0, 0.0, 0.0, 0, 0, 0, 1, p, None)
    with pytest.raises(_lib.MaavssError, match="vmin <= vmax"):
        _lib.call("maavss_viridis_image", p, 0, 1, 4, 4, 0, 4, 1, None, 3, 1.0, -1.0, 0, 0, 1, 1, p, None)
    with pytest.raises(_lib.MaavssError, match="index range"):
        _lib.call("maavss_viridis_image", p, 0, 1 << 20, 1 << 20, 1 << 20, 0, 4, 1, p, 0, 0.0, 0.0, 0, 0, 1, 1, p, None)
    with pytest.raises(_lib.MaavssError, match="specgram: null pointer"):
        _lib.call("maavss_specgram", None, 0, 1, 1000, 256, 128, p, p, None)
    for nfft in (100, 255, 16, 2048, 0, -256):
        with pytest.raises(_lib.MaavssError, match="power of two in 32 .. 1024"):
            _lib.call("maavss_specgram", p, 0, 1, 1000, nfft, 0, p, p, None)
        assert _lib.query("maavss_specgram_segments", 1, 1000, nfft, 0) == 0
    for nov in (256, 300, -1):
        with pytest.raises(_lib.MaavssError, match=r"noverlap = -?\d+ must be in \[0, nfft = 256\)"):
            _lib.call("maavss_specgram", p, 0, 1, 1000, 256, nov, p, p, None)
    with pytest.raises(_lib.MaavssError, match="bad sizes"):
        _lib.call("maavss_specgram", p, 0, 0, 1000, 256, 128, p, p, None)
    with pytest.raises(_lib.MaavssError, match="4-byte aligned"):
        _lib.call("maavss_specgram", p + 2, 0, 1, 1000, 256, 128, p, p, None)
    with pytest.raises(_lib.MaavssError, match="more workgroups"):
        _lib.call("maavss_specgram", p, 0, 1 << 20, 1 << 20, 64, 63, p, p, None)
    for length, nfft, nov in ((100, 256, 128), (256, 256, 128), (383, 256, 128), (384, 256, 128), (8448, 64, 63), (1000, 1024, 512)):
        assert _lib.query("maavss_specgram_segments", 1, length, nfft, nov) == tw.segments(length, nfft, nov)
    with pytest.raises(_lib.MaavssError, match="filmstrip: null pointer"):
        _lib.call("maavss_filmstrip", p, None, None, 4, 8, 8, p, p, None)
    with pytest.raises(_lib.MaavssError, match="zero-sized image"):
        _lib.call("maavss_filmstrip", p, p, None, 4, 0, 8, p, p, None)
    assert isinstance(ctypes.c_double(0.0).value, float)


def test_python_side_refuses_bad_arguments_before_any_device_work():
    import torch
    import maavss_amd
    x = torch.zeros(4, 4)
    with pytest.raises(ValueError, match="scale"):
        maavss_amd.viridis_image(x, scale=(0, 1))
    with pytest.raises(ValueError, match="float32 or float64"):
        maavss_amd.viridis_image(x.to(torch.int32))
    with pytest.raises(ValueError, match="above vmax"):
        maavss_amd.viridis_image(x, vmin=1.0, vmax=0.0)
    with pytest.raises(ValueError, match="empty"):
        maavss_amd.viridis_image(torch.zeros(0, 4))
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        maavss_amd.viridis_image(x)
    with pytest.raises(ValueError, match="power of two"):
        maavss_amd.specgram_planes(torch.zeros(1000), nfft=100)
    with pytest.raises(ValueError, match="noverlap"):
        maavss_amd.specgram_planes(torch.zeros(1000), nfft=256, noverlap=256)
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        maavss_amd.specgram_planes(torch.zeros(1000))
    with pytest.raises(ValueError, match=r"\[2, T_a, F\]"):
        maavss_amd.stft_panels(torch.zeros(3, 8, 9), torch.zeros(3, 8, 9))
    with pytest.raises(ValueError, match=r"\[1, T, H, W\]"):
        maavss_amd.filmstrip_image(torch.zeros(2, 4, 8, 8), torch.zeros(2, 4, 8, 8))
