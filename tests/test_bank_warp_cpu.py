"""The crop-and-flip of the clip bank's maps on the host: tests/bank_warp_twin.py held to the three properties its definition
(include/maavss.h, maavss_bank_warp_maps) promises -- the whole-frame box is the identity, flip alone the mirror image, a
patch-aligned box torch's bilinear interpolation of the cropped patches -- every refusal of the Python layer on a bank of CPU tensors,
and the draw order of BankCrop and of ClipPipeline.submit_clips."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import bank_warp_twin as ww
import maavss_amd
from maavss_amd import BankCrop, ClipBank, VideoTransform, _lib

HPS = (1, 2, 3, 8, 17, 28)


def _map(hp, seed):
    return np.random.default_rng(seed).random((hp, hp), dtype=np.float32)


def _aligned_boxes(hp, n, rng):
    out = []
    for _ in range(n):
        h, w = int(rng.integers(1, hp + 1)), int(rng.integers(1, hp + 1))
        out.append((8 * int(rng.integers(0, hp - h + 1)), 8 * int(rng.integers(0, hp - w + 1)), 8 * h, 8 * w))
    return out


def _any_boxes(hp, n, rng):
    s, out = 8 * hp, []
    for _ in range(n):
        h, w = int(rng.integers(1, s + 1)), int(rng.integers(1, s + 1))
        out.append((int(rng.integers(0, s - h + 1)), int(rng.integers(0, s - w + 1)), h, w))
    return out


@pytest.mark.parametrize("hp", HPS)
def test_whole_frame_is_the_identity_and_flip_the_mirror_image_exactly(hp):
    m, s = _map(hp, hp), 8 * hp
    if hp > 1:
        m[0, 0] = 0.0                                                 # +0 stays +0 (alone it would make the frame maximum 0)
    same = ww.warp_frame(m, (0, 0, s, s), frame_norm=False)
    assert same.view(np.uint32).tolist() == m.view(np.uint32).tolist()
    mirrored = ww.warp_frame(m, (0, 0, s, s), flip=True, frame_norm=False)
    assert mirrored.view(np.uint32).tolist() == np.ascontiguousarray(m[:, ::-1]).view(np.uint32).tolist()
    # with the frame normalisation: one f32 reciprocal and one f32 product per value, the maximum becomes 1 where it is exact
    normed = ww.warp_frame(m, (0, 0, s, s))
    assert np.array_equal(normed, m * (np.float32(1) / m.max())) and normed.dtype == np.float32


def _grid_map(hp, seed):
    """Map values k / 1024, k = 1 .. 1023: see test_patch_aligned_boxes_are_torchs_bilinear_interpolation for why."""
    return (np.random.default_rng(seed).integers(1, 1024, (hp, hp)) / 1024).astype(np.float32)


@pytest.mark.parametrize("hp", HPS)
def test_patch_aligned_boxes_are_torchs_bilinear_interpolation(hp):
    """v against F.interpolate(m[lo:hi+1, lo':hi'+1], size=(hp, hp), mode="bilinear", align_corners=False) in float64: half an f32 ulp
    of v for the one rounding to f32, plus 8 * 2^-53 * max|m| for the f64 roundings of the seven operations of the definition and of
    the weight.

    The data.  The bound budgets the twin's float64 roundings and nothing for the reference's own: torch forms the source coordinate
    as scale * (j + 0.5) - 0.5 with a rounded scale (25 / 28 and the like), so its float64 result is up to about hp * 2^-53 * max|m|
    from the exact value.  That matters only where the exact value lies within that distance of a TIE between two float32 values:
    there the twin, correctly, rounds to one neighbour (half an ulp away), and torch's value may lie on the other side.  So the maps
    are taken from a grid on which no exact value can lie that close to a tie without being representable: values k / 1024,
    1 <= k < 1024.  The weights are multiples of 1 / (16 hp), so an exact value is P / (q * 2^s) with q the odd part of hp^2
    (at most 289), s <= 10 + 2 * 7 = 24 (hp = 8: 16 hp = 2^7) and, the taps being at least 2^-10, lies in some [2^-e-1, 2^-e) with
    e <= 10.  If q divides P the value is below 1 with at most 24 fractional bits and IS a float32 (no rounding at all); if not, its
    distance from every midpoint odd / 2^(25+e) is at least 1 / (q * 2^(25+e)) >= 2^-35 / 289 = 1.0e-13, twenty times torch's error
    and the twin's together (under 40 * 2^-53 = 4.4e-15).
    On such maps "the twin is the exact value rounded once" (the next test, on full-mantissa maps) and "within the bound of
    torch" say the same thing, and a wrong tap or weight is off by a multiple of 2^-28 at least.
    Measured on full-mantissa maps in [0, 1) instead (multiples of 2^-24, where exact ties are common; 30 boxes per hp, six seeds):
    hp <= 17 stay inside the bound; at hp = 28, 21 of 180 boxes hold an element at half an ulp plus 8 to 15 * 2^-53, in every case an
    exact tie, the twin exactly half an ulp from the exact value and torch's float64 value 8 to 15 * 2^-53 from it."""
    rng = np.random.default_rng(100 + hp)
    m = _grid_map(hp, 50 + hp)
    worst = 0.0
    for box in _aligned_boxes(hp, 30, rng) + [(0, 0, 8 * hp, 8 * hp), (8 * (hp - 1), 8 * (hp - 1), 8, 8)]:
        top, left, h, w = box
        crop = torch.from_numpy(m.astype(np.float64))[top // 8:(top + h) // 8, left // 8:(left + w) // 8]
        want = torch.nn.functional.interpolate(crop[None, None], size=(hp, hp), mode="bilinear", align_corners=False)[0, 0].numpy()
        got = ww.warp_frame(m, box, frame_norm=False)
        ulp = np.spacing(np.abs(got)).astype(np.float64)
        bound = 0.5 * ulp + 8 * 2.0 ** -53 * float(np.abs(m).max())
        err = np.abs(got.astype(np.float64) - want)
        worst = max(worst, float(err.max()))
        assert (err <= bound).all(), (box, float(err.max()), float(bound.min()))
    print(f"hp = {hp}: worst |twin - interpolate| = {worst:.3e}")


def _exact_value(m, hp, box, i, j):
    """The definition in rational arithmetic: no rounding anywhere."""
    top, left, height, width = box
    d = 16 * hp

    def weight(k, off, length):
        n = 2 * off * hp + (2 * k + 1) * length - 8 * hp
        return Fraction(n - (n // d) * d, d)
    (a, b, _), (c, e, _) = ww.axis(i, hp, top, height), ww.axis(j, hp, left, width)
    wy, wx = weight(i, top, height), weight(j, left, width)
    r0 = (1 - wx) * Fraction(float(m[a, c])) + wx * Fraction(float(m[a, e]))
    r1 = (1 - wx) * Fraction(float(m[b, c])) + wx * Fraction(float(m[b, e]))
    return (1 - wy) * r0 + wy * r1


@pytest.mark.parametrize("hp", HPS)
def test_the_twin_is_the_exact_value_rounded_once(hp):
    """Against rational arithmetic, where the reference has no error of its own: |v - exact| <= half an f32 ulp of v (the one rounding
    to float32) + 8 * 2^-53 * max|m| (the weight's division and the seven float64 operations, each within 2^-53 of a value no larger
    than max|m|).  Full-mantissa maps, where exact ties between two float32 values are common (two of the boxes are ones where torch's
    float64 result lies on the other side of such a tie), patch-aligned and arbitrary boxes."""
    rng = np.random.default_rng(100 + hp)
    m = _map(hp, 50 + hp)
    slack = Fraction(8, 2 ** 53) * Fraction(float(m.max()))
    aligned = _aligned_boxes(hp, 30, rng)
    for box in aligned[:6] + [b for b in aligned if b in ((160, 8, 16, 200), (32, 0, 144, 224))] + _any_boxes(hp, 6, rng):
        got = ww.warp_frame(m, box, frame_norm=False)
        for i in range(hp):
            for j in range(hp):
                err = abs(Fraction(float(got[i, j])) - _exact_value(m, hp, box, i, j))
                assert err <= Fraction(float(np.spacing(got[i, j]))) / 2 + slack, (box, i, j, float(err))


@pytest.mark.parametrize("hp", HPS)
def test_output_lies_between_its_taps(hp):
    rng = np.random.default_rng(200 + hp)
    m = _map(hp, 70 + hp)
    for box in _aligned_boxes(hp, 10, rng) + _any_boxes(hp, 30, rng):
        got = ww.warp_frame(m, box, frame_norm=False)
        t = ww.taps(hp, box)
        vals = m[t[..., 0], t[..., 1]]                              # [hp, hp, 4]
        top, left, h, w = box
        assert t[..., 0].min() >= top // 8 and t[..., 0].max() <= (top + h - 1) // 8, box
        assert t[..., 1].min() >= left // 8 and t[..., 1].max() <= (left + w - 1) // 8, box
        assert (got >= vals.min(-1)).all() and (got <= vals.max(-1)).all(), box


def test_axis_by_hand():
    # hp = 2 (16 pixels), rows 4 .. 11: output centres at pixel 6 and 10 = source patch units 0.25 and 0.75 -> taps (0, 1), weights
    assert ww.axis(0, 2, 4, 8) == (0, 1, 0.25) and ww.axis(1, 2, 4, 8) == (0, 1, 0.75)
    # a 1-pixel box in the last row of hp = 3: every tap is patch 2
    assert [ww.axis(i, 3, 23, 1)[:2] for i in range(3)] == [(2, 2)] * 3
    # the whole frame: output patch i lies on source patch i (weight 0; the second tap of the last one is clamped)
    assert ww.axis(0, 3, 0, 24) == (0, 1, 0.0) and ww.axis(2, 3, 0, 24) == (2, 2, 0.0)
    # upsampling the top-left patch: centres above the patch centre clamp to it (y0 = -1)
    assert ww.axis(0, 3, 0, 8)[:2] == (0, 0) and ww.axis(2, 3, 0, 8)[:2] == (0, 0)


# ---- the Python layer on CPU tensors ---------------------------------------------------------------------------------------------
T, FRAME_HOP, HPF, HOP, S = 3, 1, 1, 40, 16


def _bank(size=S, **kw):
    bank = ClipBank(size, T, FRAME_HOP, HPF, HOP, capacity_frames=16, capacity_samples=8000, device="cpu", **kw)
    g = torch.Generator().manual_seed(1)
    bank.add_recording(torch.rand(4000, generator=g), maps=torch.rand(6, (size // 8) ** 2, generator=g))
    return bank


def _boxes(*rows):
    return torch.tensor(rows, dtype=torch.int32)


def test_every_refusal_comes_before_any_device_work():
    bank = _bank()
    assert len(bank) == 4
    whole = _boxes((0, 0, S, S), (0, 0, S, S))
    for call in (lambda **kw: bank.batch([0, 1], **kw), lambda **kw: bank.cut(*bank.check_indices([0, 1]), **kw),
                 lambda boxes=None, **kw: bank.warp_maps([0, 1], boxes, **kw)):
        with pytest.raises(ValueError, match=r"boxes must be a CPU int32 tensor \[2, 4\]"):
            call(boxes=whole.to(torch.int64))
        with pytest.raises(ValueError, match=r"boxes must be a CPU int32 tensor \[2, 4\]"):
            call(boxes=whole[:1])
        with pytest.raises(ValueError, match="boxes must be a CPU int32"):
            call(boxes=whole.tolist())
        with pytest.raises(ValueError, match="boxes must be a CPU int32"):
            call(boxes=whole.float())
        for bad in ((0, 0, 0, S), (0, 0, S, 0), (-1, 0, 4, 4), (0, -1, 4, 4), (1, 0, S, 4), (0, 9, 4, 8), (S, 0, 1, 1)):
            with pytest.raises(ValueError, match=r"box 1 = .* is empty or not inside the 16x16 frame"):
                call(boxes=_boxes((0, 0, S, S), bad))
        with pytest.raises(ValueError, match=r"flip must be a CPU bool or uint8 tensor \[2\]"):
            call(boxes=whole, flip=torch.tensor([0, 1]))
        with pytest.raises(ValueError, match="flip must be a CPU bool or uint8"):
            call(boxes=whole, flip=torch.tensor([True]))
        with pytest.raises(ValueError, match="flip must be a CPU bool or uint8"):
            call(boxes=whole, flip=[True, False])
        # valid arguments reach the device work, which a CPU bank refuses like every other op without the MI355X
        with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
            call(boxes=whole, flip=torch.tensor([True, False]), frame_norm=False)
        with pytest.raises(IndexError):
            bank.batch([9, 0], boxes=whole)
    with pytest.raises(ValueError, match="warp_maps needs boxes="):
        bank.warp_maps([0, 1], None, flip=torch.tensor([True, False]))
    with pytest.raises(ValueError, match="frame_norm= belongs to the warped path"):
        bank.batch([0, 1], frame_norm=False)
    with pytest.raises(ValueError, match="frame_norm= belongs to the warped path"):
        bank.cut(*bank.check_indices([0]), frame_norm=False)
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        bank.batch([0, 1], flip=torch.tensor([1, 0], dtype=torch.uint8))     # flip alone is a warp of the whole frame
    odd = _bank(size=12)                                                     # a multiple of 4, as the bank asks, but not of 8
    with pytest.raises(ValueError, match="frame_size % 8 == 0, got 12"):
        odd.batch([0], boxes=_boxes((0, 0, 8, 8)))
    with pytest.raises(ValueError, match="frame_size % 8 == 0, got 12"):
        odd.batch([0], flip=torch.tensor([True]))
    with pytest.raises(ValueError, match="frame_size % 8 == 0, got 12"):
        odd.warp_maps([0], _boxes((0, 0, 8, 8)))
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        odd.batch([0])                                                       # the plain cut does not ask for it


def test_check_warp_fills_in_what_is_missing():
    bank = _bank()
    assert bank.check_warp(3, None, None) is None
    boxes, flip = bank.check_warp(3, None, torch.tensor([True, False, True]))
    assert boxes.dtype == torch.int32 and boxes.tolist() == [[0, 0, S, S]] * 3 and flip.dtype == torch.uint8 and flip.tolist() == [1, 0, 1]
    given = _boxes((1, 2, 3, 4), (15, 15, 1, 1), (0, 0, 16, 16))
    boxes, flip = bank.check_warp(3, given, None)
    assert torch.equal(boxes, given) and flip.tolist() == [0, 0, 0]
    assert bank.check_warp(3, given, torch.tensor([0, 7, 1], dtype=torch.uint8))[1].tolist() == [0, 1, 1]


def test_bank_crop_draws_sample_boxes_first_and_the_flips_after_them():
    crop = BankCrop(flip=0.5)
    g, h = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    boxes, flip = crop.sample(6, 224, g)
    want = VideoTransform(224, (0.6, 1.0), (3 / 4, 4 / 3)).sample_boxes(6, 224, 224, h)
    assert boxes.dtype == torch.int32 and torch.equal(boxes, want)
    assert flip.dtype == torch.bool and torch.equal(flip, torch.rand(6, dtype=torch.float64, generator=h) < 0.5)
    assert torch.equal(g.get_state(), h.get_state())
    assert flip.any() and not flip.all()
    # no flip: the same boxes, no flag set and the generator left where the boxes left it
    g, h = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    boxes0, flip0 = BankCrop().sample(6, 224, g)
    VideoTransform(224).sample_boxes(6, 224, 224, h)
    assert torch.equal(boxes0, want) and not flip0.any() and flip0.dtype == torch.bool and torch.equal(g.get_state(), h.get_state())
    # other scale / ratio reach sample_boxes
    g, h = torch.Generator().manual_seed(12), torch.Generator().manual_seed(12)
    small = BankCrop(scale=(0.1, 0.2), ratio=(1.0, 2.0)).sample(4, 64, g)[0]
    assert torch.equal(small, VideoTransform(64, (0.1, 0.2), (1.0, 2.0)).sample_boxes(4, 64, 64, h))
    assert bool((small[:, 2] * small[:, 3] <= 0.2 * 64 * 64 + 64).all())
    assert BankCrop(flip=1.0).sample(5, 16, torch.Generator().manual_seed(0))[1].all()
    # every drawn box is one the bank takes
    _bank().check_warp(6, BankCrop().sample(6, S, torch.Generator().manual_seed(3))[0], None)
    for bad in (-0.1, 1.5, True, "0.5"):
        with pytest.raises(ValueError, match="flip must be a probability"):
            BankCrop(flip=bad)
    with pytest.raises(ValueError, match="bad scale"):
        BankCrop(scale=(0.0, 1.0))
    with pytest.raises(ValueError, match="batch"):
        crop.sample(0, 16)


def test_pipeline_seed_gives_the_crops_and_its_refusals():
    bank = _bank()
    stft = maavss_amd.STFT(512, HOP, device="cpu")
    with pytest.raises(ValueError, match="it needs bank="):
        maavss_amd.ClipPipeline(None, stft, T, bank_crop=BankCrop())
    with pytest.raises(ValueError, match="frame_size % 8 == 0, got 12"):
        maavss_amd.ClipPipeline(None, stft, T, bank=_bank(size=12), bank_crop=BankCrop())
    # the host side of submit_clips on a pipeline without its side stream (the constructor opens one on the device)
    pipe = object.__new__(maavss_amd.ClipPipeline)
    pipe.bank, pipe.bank_crop = bank, None
    assert pipe.check_crop(2, 5, None, None) == (None, None)
    with pytest.raises(ValueError, match="built with bank_crop="):
        pipe.check_crop(2, 5, _boxes((0, 0, S, S), (0, 0, S, S)), None)
    with pytest.raises(ValueError, match="built with bank_crop="):
        pipe.check_crop(2, 5, None, torch.tensor([True, False]))
    pipe.bank_crop = BankCrop(flip=0.5)
    want = pipe.bank_crop.sample(4, S, torch.Generator().manual_seed(77))
    boxes, flip = pipe.check_crop(4, 77, None, None)
    assert torch.equal(boxes, want[0]) and torch.equal(flip, want[1].to(torch.uint8))
    assert not torch.equal(pipe.check_crop(4, 78, None, None)[0], boxes)
    # one of the two given: the other is the seed's
    mine = _boxes(*[(1, 2, 3, 4)] * 4)
    got = pipe.check_crop(4, 77, mine, None)
    assert torch.equal(got[0], mine) and torch.equal(got[1], want[1].to(torch.uint8))
    got = pipe.check_crop(4, 77, None, torch.tensor([True] * 4))
    assert torch.equal(got[0], want[0]) and got[1].tolist() == [1] * 4
    with pytest.raises(ValueError, match="box 0 = .* not inside"):
        pipe.check_crop(4, 77, _boxes(*[(9, 9, 9, 9)] * 4), None)
    # submit_clips refuses them before any device work
    pipe.mixer, pipe.reverb, pipe.head, pipe.tail, pipe.depth, pipe.slots = None, None, 0, 0, 2, [None, None]
    with pytest.raises(ValueError, match="box 0 = .* not inside"):
        pipe.submit_clips([0, 1, 2, 3], 77, _boxes(*[(9, 9, 9, 9)] * 4))
    with pytest.raises(ValueError, match="flip must be a CPU bool or uint8"):
        pipe.submit_clips([0, 1, 2, 3], 77, flip=torch.zeros(4))
