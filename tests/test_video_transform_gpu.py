"""maavss_video_transform (VideoTransform) on the GPU against torch on the CPU: the reference's clip transform (av_dataset.py:315-319)
restated as crop of permute(0,3,1,2).float() / 255 -> F.interpolate(bilinear, align_corners=False, antialias) -> Normalize ->
torchvision's float autocontrast (restated below from its formula), per clip box.

Sources 360x640, 240x320 (crop smaller than S: upsampling), 257x333 (odd sizes) and one 1080x1920 frame (antialias support of
~8.6 source pixels per side); full-frame boxes, boxes on every edge, boxes that shrink one axis and stretch the other; clips of 2
frames sharing a box; S = 224 and 256; antialias and autocontrast on and off, with an exactly constant plane that must take
autocontrast's scale = 1, min = 0 branch.  Gate: max |err| <= 1e-5; measured on MI355X (max over the four antialias x autocontrast
combinations): 360x640 -> 256 1.07e-6, 240x320 -> 256 8.3e-7, 257x333 -> 224 9.5e-7, 1080x1920 -> 224 9.5e-7."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MEAN = torch.tensor([0.485, 0.456, 0.406])
STD = torch.tensor([0.229, 0.224, 0.225])


def oracle(video_u8, boxes, clip_frames, S, antialias, autocontrast):
    x = video_u8.permute(0, 3, 1, 2).float() / 255
    out = []
    for c, (t, l, h, w) in enumerate(boxes.tolist()):
        crop = x[c * clip_frames:(c + 1) * clip_frames, :, t:t + h, l:l + w]
        y = F.interpolate(crop, size=(S, S), mode="bilinear", align_corners=False, antialias=antialias)
        y = (y - MEAN[:, None, None]) / STD[:, None, None]
        if autocontrast:             # torchvision.transforms.functional.autocontrast on a float tensor (bound 1.0)
            lo, hi = y.amin((-2, -1), keepdim=True), y.amax((-2, -1), keepdim=True)
            scale = 1.0 / (hi - lo)
            bad = ~torch.isfinite(scale)
            lo[bad] = 0
            scale[bad] = 1
            y = ((y - lo) * scale).clamp(0, 1)
        out.append(y)
    return torch.cat(out)


def _video(f, h0, w0, seed):
    return torch.randint(0, 256, (f, h0, w0, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


CASES = [
    # (H0, W0, frames, clip_frames, S, boxes (top, left, h, w))
    (360, 640, 4, 2, 256, [[0, 0, 360, 640], [100, 200, 260, 440]]),               # full frame; bottom + right edges
    (240, 320, 3, 1, 256, [[0, 0, 240, 320], [0, 100, 120, 220], [50, 0, 190, 150]]),  # 240 -> 256 up, 320 -> 256 down; top; left + bottom
    (257, 333, 2, 1, 224, [[1, 0, 256, 333], [0, 17, 201, 97]]),                   # odd sizes; left + right; top, upsampled both ways
    (1080, 1920, 1, 1, 224, [[0, 0, 1080, 1920]]),                                 # wide antialias support
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_transform_matches_torch(case):
    import maavss_amd
    h0, w0, f, cf, s, boxes = CASES[case]
    video = _video(f, h0, w0, 11 + case)
    if case == 1:
        video[1, :, :, 0] = 0          # a constant plane: autocontrast's max == min branch
    boxes = torch.tensor(boxes, dtype=torch.int32)
    dev = video.cuda()
    worst = 0.0
    for aa in (False, True):
        for ac in (False, True):
            t = maavss_amd.VideoTransform(s, antialias=aa, autocontrast=ac)
            got = t(dev, boxes=boxes, clip_frames=cf).cpu()
            want = oracle(video, boxes, cf, s, aa, ac)
            err = (got - want).abs().max().item()
            worst = max(worst, err)
            assert got.shape == (f, 3, s, s)
            assert err <= 1e-5, f"{h0}x{w0} -> {s}, antialias={aa}, autocontrast={ac}: max|err| {err:.3e}"
            if case == 1:
                plane = want[1, 0]
                assert ac or plane.max() == plane.min()
                if ac:
                    assert torch.equal(got[1, 0], torch.zeros(s, s))     # clamp((0 - 0.485) / 0.229, 0, 1), not NaN
    print(f"[video_transform] {h0}x{w0} -> {s}: max|err| over antialias x autocontrast = {worst:.2e}")


def test_sampled_boxes_and_repeat_bit_identical():
    import maavss_amd
    video = _video(8, 360, 640, 5)
    t = maavss_amd.VideoTransform(256, antialias=True, autocontrast=True)
    boxes = t.sample_boxes(2, 360, 640, torch.Generator().manual_seed(1))
    dev = video.cuda()
    a = t(dev.view(2, 4, 360, 640, 3), boxes=boxes)
    b = t(dev, boxes=boxes, clip_frames=4)
    assert torch.equal(a, b)
    err = (a.cpu() - oracle(video, boxes, 4, 256, True, True)).abs().max().item()
    assert err <= 1e-5, err
    # boxes drawn from a generator inside the call: the same draw as sample_boxes with that seed
    c = t(dev, clip_frames=4, generator=torch.Generator().manual_seed(1))
    assert torch.equal(a, c)


def test_pipeline_with_transform_equals_transform_then_pipeline():
    import maavss_amd
    from oracle import avse_ref_cpu as orc, stft_ref_cpu as sref, vit_ref_cpu as vref
    B, T, W, FFT, HPF = 2, 8, 128, 256, 8
    hop, length, t_a = maavss_amd.calc_hop_size(T, HPF, 30, 16000)
    va = maavss_amd.VideoAttention(path_to_weights="/nonexistent.pth")
    va.load_state_dict(vref.seeded_vit_state(3))
    stft = maavss_amd.STFT(FFT, hop, noise_std=0.1, device="cuda")
    tr = maavss_amd.VideoTransform(W, autocontrast=True)
    raws = [_video(B * T, 96, 160, 30 + i).cuda() for i in range(3)]
    audio = [sref.synthetic_audio(B, length, 40 + i).cuda() for i in range(3)]
    # by hand: transform with the boxes submit() draws by default, then the float-frame extractor
    want = []
    for i in range(3):
        boxes = tr.sample_boxes(B, 96, 160, torch.Generator().manual_seed(i))
        want.append(va.attention_frames(tr(raws[i], boxes=boxes, clip_frames=T), clip_frames=T).view(B, 1, T, W, W).clone())
    n_bins = FFT // 2 + 1
    shapes = ([B, 2, t_a, n_bins], [B, 1, T, W, W], HPF)
    model = maavss_amd.AV_Fusion_Model_Frames(*shapes)
    model.load_state_dict(orc.seeded_state_dict(orc.AVFusionFramesRef(*shapes), 5), strict=True)
    step = maavss_amd.TrainStep(model.cuda().train(), lr=1e-4)
    pipe = maavss_amd.ClipPipeline(va, stft, T, transform=tr)
    pipe.submit(raws[0], audio[0], seed=0)
    losses = []
    for i in range(3):
        if i + 1 < 3:
            pipe.submit(raws[i + 1].view(B, T, 96, 160, 3), audio[i + 1], seed=i + 1)
        x_v, x_stft, y_stft = pipe.get()
        assert torch.equal(x_v, want[i]), f"batch {i}: attention frames differ from transform-then-extract"
        if i < 2:
            mid = T // 2
            losses.append(step(x_stft, x_v, y_stft[:, :, mid * HPF:(mid + 1) * HPF, :], x_v[:, :, mid])[2].item())
        pipe.release()
    pipe.drain()
    assert all(torch.isfinite(torch.tensor(losses))), losses
    print(f"[video_transform] pipeline: 3 uint8 batches bit-identical to transform + extractor; 2 training steps, losses {losses}")
