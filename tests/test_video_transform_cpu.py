"""VideoTransform (maavss_amd/video_transform.py) without a device: torchvision-style box sampling (RandomResizedCrop.get_params)
and the host-side argument checks that run before any device work; the C-ABI declarations of maavss_video_transform."""
import pytest
import torch

import maavss_amd
from maavss_amd import _lib


def test_sample_boxes_is_deterministic_per_generator():
    t = maavss_amd.VideoTransform(256)
    a = t.sample_boxes(64, 360, 640, torch.Generator().manual_seed(7))
    b = t.sample_boxes(64, 360, 640, torch.Generator().manual_seed(7))
    c = t.sample_boxes(64, 360, 640, torch.Generator().manual_seed(8))
    assert a.dtype == torch.int32 and a.device.type == "cpu" and tuple(a.shape) == (64, 4)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    # the global RNG when no generator is given: reproducible under torch.manual_seed
    torch.manual_seed(3)
    d = t.sample_boxes(8, 360, 640)
    torch.manual_seed(3)
    assert torch.equal(d, t.sample_boxes(8, 360, 640))


@pytest.mark.parametrize("hw", [(360, 640), (240, 320), (257, 333), (1080, 1920), (640, 360), (64, 64)])
def test_sampled_boxes_lie_inside_and_follow_scale_and_ratio(hw):
    h0, w0 = hw
    t = maavss_amd.VideoTransform(224)
    boxes = t.sample_boxes(400, h0, w0, torch.Generator().manual_seed(h0 * 7 + w0))
    top, left, h, w = boxes.long().unbind(1)
    assert bool(((top >= 0) & (left >= 0) & (h >= 1) & (w >= 1) & (top + h <= h0) & (left + w <= w0)).all())
    # a sampled (non-fallback) box: area / (H0 W0) in [0.6, 1] and w / h in [3/4, 4/3], up to the rounding of w and h to integers
    area = (h * w).double() / (h0 * w0)
    ratio = w.double() / h.double()
    tol_a = (h + w + 1).double() / (h0 * w0)
    tol_r = 1.0 / h.double() + ratio / h.double()
    assert bool(((area >= 0.6 - tol_a) & (area <= 1.0 + tol_a)).all()), area.min()
    assert bool(((ratio >= 0.75 - tol_r) & (ratio <= 4 / 3 + tol_r)).all()), (ratio.min(), ratio.max())
    # top / left are drawn, not fixed: the 400 boxes are not all the central crop
    assert len({tuple(b) for b in boxes.tolist()}) > 1


def test_degenerate_frames_take_the_central_fallback():
    t = maavss_amd.VideoTransform(224)
    # 1 x 1000: no attempt can fit; in_ratio 1000 > 4/3 -> h = 1, w = round(1 * 4/3) = 1, centred
    assert t.sample_boxes(3, 1, 1000, torch.Generator().manual_seed(0)).tolist() == [[0, 499, 1, 1]] * 3
    # 1000 x 1: in_ratio 0.001 < 3/4 -> w = 1, h = round(1 / (3/4)) = 1, centred
    assert t.sample_boxes(2, 1000, 1, torch.Generator().manual_seed(0)).tolist() == [[499, 0, 1, 1]] * 2


def test_bad_arguments_raise_before_device_work():
    t = maavss_amd.VideoTransform(32)
    video = torch.zeros(4, 20, 30, 3, dtype=torch.uint8)          # CPU: any device work would fail differently
    with pytest.raises(ValueError, match="not inside"):
        t(video, boxes=torch.tensor([[0, 0, 21, 10], [0, 0, 5, 5]]), clip_frames=2)
    with pytest.raises(ValueError, match="not inside"):
        t(video, boxes=torch.tensor([[0, 25, 10, 6], [0, 0, 5, 5]]), clip_frames=2)
    with pytest.raises(ValueError, match="not inside"):
        t(video, boxes=torch.tensor([[0, 0, 0, 5], [0, 0, 5, 5]]), clip_frames=2)
    with pytest.raises(ValueError, match="not inside"):
        t(video, boxes=torch.tensor([[-1, 0, 5, 5], [0, 0, 5, 5]]), clip_frames=2)
    with pytest.raises(ValueError, match="one per clip"):
        t(video, boxes=torch.tensor([[0, 0, 5, 5]]), clip_frames=2)
    with pytest.raises(ValueError, match="whole number of clips"):
        t(video, clip_frames=3)
    with pytest.raises(ValueError, match="uint8"):
        t(video.float(), clip_frames=2)
    with pytest.raises(ValueError, match="HWC"):
        t(torch.zeros(4, 3, 20, 30, dtype=torch.uint8))         # CHW, not the decoder's HWC
    with pytest.raises(ValueError, match="conflicts"):
        t(video.view(2, 2, 20, 30, 3), clip_frames=3)
    with pytest.raises(ValueError, match="CPU integer"):
        t(video, boxes=torch.tensor([[0.0, 0, 5, 5], [0, 0, 5, 5]]), clip_frames=2)
    for s in (4, 6, 30):
        with pytest.raises(ValueError, match="framesize"):
            maavss_amd.VideoTransform(s)
    # valid arguments get as far as the device check: there is no CPU fallback
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        t(video, boxes=torch.tensor([[0, 0, 20, 30], [1, 2, 5, 5]]), clip_frames=2)


def test_header_declares_the_transform_entry_points():
    protos = _lib.parse_header()
    ret, args = protos["maavss_video_transform"]
    names = [n for _, n in args]
    assert names[:6] == ["src", "boxes", "host_boxes", "out", "ws", "ws_bytes"] and names[-1] == "stream"
    assert {"antialias", "autocontrast", "clip_frames", "S"} <= set(names)
    ret, args = protos["maavss_video_transform_ws_bytes"]
    assert [n for _, n in args] == ["F", "clip_frames", "H0", "W0", "S", "antialias", "autocontrast"]
    assert _lib.header_abi_version() == 402          # additive in 400; 401 removed the convt2d, 402 the conv2d entry points
