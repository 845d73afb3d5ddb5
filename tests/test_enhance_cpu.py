"""Enhancer (maavss_amd/enhance.py) without a device: the audio-clocked tiling of a recording into training clips (clip count C, the
video frame v_c each clip starts at, the output length and its first sample) and every refusal, raised before any device work; the
C-ABI declarations of the window kernels."""
from fractions import Fraction

import pytest
import torch

import maavss_amd
from maavss_amd import _lib
from maavss_amd.enhance import clip_tiling

T, W, FFT, HPF = 8, 128, 256, 8


def _model(batch=4, t=T, w=W, hpf=HPF):
    hop, _, t_a = maavss_amd.calc_hop_size(t, hpf, 30, 16000)
    return maavss_amd.AV_Fusion_Model_Frames([batch, 2, t_a, FFT // 2 + 1], [batch, 1, t, w, w], hpf), hop


def _brute(L, N, n, s, a, h, fps, sr):
    """The definition read literally: every clip count for which all clips fit, the largest one."""
    tc, step = n + s, s * a * h
    v = lambda c: round(c * step * Fraction(fps) / sr)
    best = 0
    for cnt in range(0, L // step + 2):
        if all(c * step + a * h * tc <= L and v(c) + tc <= N for c in range(cnt)):
            best = cnt
    return best, [v(c) for c in range(best)]


@pytest.mark.parametrize("fps,sr,a,n,s,N,L", [
    (30, 16000, 8, 16, 4, 1800, 960000),        # the reference's run_config: a*h = 528 samples, not 533.3
    (30, 16000, 8, 8, 3, 40, 16000 * 2),
    (25, 16000, 4, 5, 2, 33, 20000),
    (24, 48000, 5, 6, 1, 20, 48000),
    (30, 16000, 8, 16, 4, 30, 960000),          # video-limited
    (30, 16000, 8, 16, 4, 1800, 12000),         # audio-limited
    (29.97, 44100, 7, 4, 5, 300, 400000),       # a non-integer frame rate
])
def test_tiling_matches_the_definition(fps, sr, a, n, s, N, L):
    h = int((sr / fps) / a)                     # calc_hop_size
    got_c, got_v = clip_tiling(L, N, n, s, a, h, fps, sr)
    want_c, want_v = _brute(L, N, n, s, a, h, fps, sr)
    assert (got_c, got_v) == (want_c, want_v)
    assert got_v == sorted(got_v) and all(v >= 0 for v in got_v)
    if got_c:
        # the last clip fits and one more would not
        step, tc = s * a * h, n + s
        assert (got_c - 1) * step + a * h * tc <= L and got_v[-1] + tc <= N
        nxt = round(got_c * step * Fraction(fps) / sr)
        assert got_c * step + a * h * tc > L or nxt + tc > N


def test_reference_config_counts():
    # 60 s at 30 fps / 16 kHz, a = 8, n = 16, s = 4: h = 66, step 2112 samples, clip 10560 samples / 20 frames
    c, v = clip_tiling(960000, 1800, 16, 4, 8, 66, 30, 16000)
    assert c == (960000 - 10560) // 2112 + 1 == 450
    assert v[:6] == [0, 4, 8, 12, 16, 20] and v[25] == 99 and v[-1] == round(449 * 2112 * 30 / 16000) == 1778


@pytest.mark.parametrize("fps,sr,a", [(30, 15840, 8), (25, 16000, 8), (50, 16000, 4), (30, 48000, 10)])
def test_audio_clock_equal_to_the_video_clock_gives_steps_of_num_seq(fps, sr, a):
    h = int((sr / fps) / a)
    assert Fraction(sr, 1) / Fraction(fps) == a * h                     # sr / fps == a*h exactly
    n, s = 6, 3
    c, v = clip_tiling(10 ** 6, 10 ** 4, n, s, a, h, fps, sr)
    assert c > 10 and v == [i * s for i in range(c)]


def test_enhancer_tiling_start_and_output_length():
    model, hop = _model()
    model.eval()
    stft = maavss_amd.STFT(FFT, hop, device="cpu")
    for s, off, want_off in ((3, None, 1), (4, None, 1), (1, None, 0), (4, 4, 4), (2, T, T)):
        enh = maavss_amd.Enhancer(model, stft, T, s, HPF, target_offset=off)
        assert enh.target_offset == want_off
        assert enh.clip_frames == T + s and enh.clip_samples == HPF * hop * (T + s)
        c, v = enh.tiling(16000 * 3, 90)
        assert (c, v) == clip_tiling(16000 * 3, 90, T, s, HPF, hop, 30, 16000)
        # [h (C s a - 1)] samples, wave[0] at sample target_offset * a * h of the input
        assert enh.output_length(c) == hop * (c * s * HPF - 1)
        assert enh.output_length(c) + want_off * HPF * hop <= 16000 * 3
    assert maavss_amd.Enhancer(model, stft, T, 3, HPF).windows_per_launch == 4          # the model's constructed batch
    assert maavss_amd.Enhancer(model, stft, T, 3, HPF, windows_per_launch=7).windows_per_launch == 7


class _NoDevice:
    """_lib.call / query replaced: a refusal must come before any entry point runs."""

    def __init__(self, monkeypatch):
        def boom(*a, **k):
            raise AssertionError("device work before the argument checks")
        monkeypatch.setattr(_lib, "call", boom)
        monkeypatch.setattr(_lib, "query", boom)
        monkeypatch.setattr(maavss_amd.enhance, "call", boom)


def test_refusals_come_before_any_device_work(monkeypatch):
    _NoDevice(monkeypatch)
    model, hop = _model()
    stft = maavss_amd.STFT(FFT, hop, device="cpu")
    s = 3
    clip = HPF * hop * (T + s)
    audio = torch.zeros(3 * clip)
    frames = torch.zeros(40, 3, W, W)
    attn = torch.zeros(40, 1, W, W)
    va = object()                                      # never reached: a stand-in for VideoAttention
    enh = maavss_amd.Enhancer(model, stft, T, s, HPF, video_attention=va)
    # training mode: model.eval() is the caller's job
    assert model.training
    with pytest.raises(ValueError, match="training mode"):
        enh(audio, attn=attn)
    model.eval()
    with pytest.raises(ValueError, match="exactly one"):
        enh(audio, frames=frames, attn=attn)
    with pytest.raises(ValueError, match="exactly one"):
        enh(audio)
    with pytest.raises(ValueError, match="video_attention"):
        maavss_amd.Enhancer(model, stft, T, s, HPF)(audio, frames=frames)
    # shapes that do not fit the model
    with pytest.raises(ValueError, match="attn must be"):
        enh(audio, attn=torch.zeros(40, 1, 64, 64))
    with pytest.raises(ValueError, match="attn must be"):
        enh(audio, attn=torch.zeros(40, 3, W, W))
    with pytest.raises(ValueError, match="frames must be"):
        enh(audio, frames=torch.zeros(40, 1, W, W))
    with pytest.raises(ValueError, match="frames must be"):
        enh(audio, frames=frames.double())
    with pytest.raises(ValueError, match="audio"):
        enh(audio.view(3, clip), attn=attn)
    with pytest.raises(ValueError, match="num_frames"):
        maavss_amd.Enhancer(model, stft, T + 1, s, HPF)
    with pytest.raises(ValueError, match="hops_per_frame"):
        maavss_amd.Enhancer(model, stft, T, s, HPF // 2)
    with pytest.raises(ValueError, match="frequency bins"):
        maavss_amd.Enhancer(model, maavss_amd.STFT(FFT, hop, trim_stft_end=True, device="cpu"), T, s, HPF)
    with pytest.raises(ValueError, match="target_offset"):
        maavss_amd.Enhancer(model, stft, T, s, HPF, target_offset=T + 1)
    with pytest.raises(ValueError, match="windows_per_launch"):
        maavss_amd.Enhancer(model, stft, T, s, HPF, windows_per_launch=0)
    with pytest.raises(ValueError, match="AV_Fusion_Model_Frames"):
        maavss_amd.Enhancer(torch.nn.Linear(2, 2), stft, T, s, HPF)
    # a recording shorter than one clip: in audio, in frames
    with pytest.raises(ValueError, match="shorter than one clip"):
        enh(audio[:clip - 1], attn=attn)
    with pytest.raises(ValueError, match="shorter than one clip"):
        enh(audio, attn=attn[:T + s - 1])


def test_valid_arguments_reach_the_device_check():
    model, hop = _model()
    model.eval()
    stft = maavss_amd.STFT(FFT, hop, device="cpu")
    enh = maavss_amd.Enhancer(model, stft, T, 3, HPF)
    clip = HPF * hop * (T + 3)
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        enh(torch.zeros(clip), attn=torch.zeros(T + 3, 1, W, W))


def test_header_declares_the_window_entry_points():
    protos = _lib.parse_header()
    for name in ("maavss_vit_attn_maps_pass1", "maavss_av_clip_scale", "maavss_av_attn_windows", "maavss_av_stft_windows",
                 "maavss_av_stitch"):
        ret, args = protos[name]
        assert args[-1][1] == "stream", name
    assert [n for _, n in protos["maavss_av_stitch"][1]][:2] == ["pred", "clip_absmax"]
    assert _lib.header_abi_version() == 402          # additive in 400; 401 removed the convt2d, 402 the conv2d entry points
