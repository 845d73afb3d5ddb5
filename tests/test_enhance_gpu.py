"""Enhancer (maavss_amd/enhance.py) on the MI355X: whole-recording inference against the straightforward loop built from the existing
public pieces (per-clip VideoAttention.attention_frames(..., clip_frames=T_c), per-clip STFT, torch slicing, model(...) per clip with
batch num_seq, STFT.inverse) and against the fp32 CPU oracle chain (train_avse_frames.py:139-176,196-200 over every clip of a
recording).  Small shapes of tests/test_pipeline_gpu.py: 8-frame windows, 128^2, 256-point STFT, a = 8; 4 clips of num_seq = 3."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T, W, FFT, HPF, S = 8, 128, 256, 8, 3          # num_frames, frame size, fft_len, hops_per_frame, num_seq
TC = T + S
N_FRAMES = 21


def _setup(precise=False, seed=5):
    import maavss_amd
    from oracle import avse_ref_cpu as orc, stft_ref_cpu as sref, vit_ref_cpu as vref
    hop, _, t_a = maavss_amd.calc_hop_size(T, HPF, 30, 16000)
    shapes = ([S, 2, t_a, FFT // 2 + 1], [S, 1, T, W, W], HPF)
    model = maavss_amd.AV_Fusion_Model_Frames(*shapes, precise=precise)
    model.load_state_dict(orc.seeded_state_dict(orc.AVFusionFramesRef(*shapes), 11), strict=True)
    model = model.cuda().eval()
    va = maavss_amd.VideoAttention(path_to_weights="/nonexistent.pth")
    va.load_state_dict(vref.seeded_vit_state(3))
    stft = maavss_amd.STFT(FFT, hop, normalize_output_fft=True, device="cuda")
    clip, step = HPF * hop * TC, S * HPF * hop
    length = 3 * step + clip + 100                  # 4 clips, and a tail that holds no fifth one
    frames = vref.synthetic_frames(N_FRAMES, W, 100 + seed)
    audio = sref.synthetic_audio(1, length, 200 + seed)[0]
    return maavss_amd, model, va, stft, frames, audio, hop


def _loop(maavss_amd, model, va, stft, frames, audio, hop, attn_diff=False):
    """The loop a user writes today from the public pieces: -> (x_a [C*S,...], x_v [C*S,...], amax [C], stitched [1,2,..], wave)."""
    enh = maavss_amd.Enhancer(model, stft, T, S, HPF, video_attention=va)
    n_clips, starts = enh.tiling(audio.shape[0], frames.shape[0])
    clip, step = HPF * hop * TC, S * HPF * hop
    xs_a, xs_v, amaxs, preds = [], [], [], []
    stitched = torch.zeros(1, 2, HPF * S * n_clips, stft.n_bins(), device="cuda")
    with torch.no_grad():
        for c, v in enumerate(starts):
            att = va.attention_frames(frames[v:v + TC].cuda(), clip_frames=TC, attn_diff=attn_diff)        # [TC,1,W,W]
            _, y, amax = stft(audio[c * step:c * step + clip][None].cuda(), want_x=False, return_scale=True)
            x_v = torch.stack([att[j:j + T].permute(1, 0, 2, 3) for j in range(S)])                         # [S,1,T,W,W]
            x_a = torch.stack([y[0, :, HPF * j:HPF * (j + T)] for j in range(S)])                           # [S,2,HPF*T,F]
            pred = model(x_a, x_v)[0]
            for j in range(S):
                w = c * S + j
                stitched[0, :, HPF * w:HPF * (w + 1)] = pred[j] * (amax[0] + 1e-7)
            xs_a.append(x_a)
            xs_v.append(x_v)
            amaxs.append(amax)
        wave = stft.inverse(stitched)[0]
    return torch.cat(xs_a), torch.cat(xs_v), torch.cat(amaxs), stitched, wave, starts


@pytest.mark.parametrize("attn_diff", [False, True])
def test_window_inputs_are_bit_identical_to_the_per_clip_loop(attn_diff):
    maavss_amd, model, va, stft, frames, audio, hop = _setup()
    x_a_ref, x_v_ref, amax_ref, _, _, starts = _loop(maavss_amd, model, va, stft, frames, audio, hop, attn_diff)
    assert len(starts) == 4 and starts == [0, 3, 6, 9]          # v_c = round(c * 1584 * 30 / 16000)
    enh = maavss_amd.Enhancer(model, stft, T, S, HPF, video_attention=va, attn_diff=attn_diff)
    x_a, x_v, amax = enh.window_inputs(audio.cuda(), frames=frames.cuda())
    assert x_v.shape == x_v_ref.shape and x_a.shape == x_a_ref.shape
    assert torch.equal(amax, amax_ref)
    assert torch.equal(x_a, x_a_ref), "STFT windows differ from the per-clip STFT"
    bad = (x_v != x_v_ref).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, f"attention windows {bad} differ from attention_frames(clip, clip_frames={TC}, attn_diff={attn_diff})"
    # the same gather from given full-resolution per-frame maps (attn=): the slices of the clip-normalised maps
    maps = va.attention_frames(frames.cuda(), clip_frames=0)
    _, x_v2, _ = enh.window_inputs(audio.cuda(), attn=maps)
    for c, v in enumerate(starts):
        clip = maps[v:v + TC]
        if attn_diff:
            clip = torch.cat([torch.zeros_like(clip[:1]), clip[1:] - clip[:-1]])
        clip = clip * (1.0 / clip.max())
        for j in range(S):
            assert torch.equal(x_v2[c * S + j, 0], clip[j:j + T, 0]), (c, j)


def test_stitch_is_torch_indexing_times_the_clip_gain():
    from maavss_amd.enhance import stitch_windows
    g = torch.Generator(device="cpu").manual_seed(4)
    n_clips, nb = 4, FFT // 2 + 1
    amax = (torch.rand(n_clips, generator=g) * 3 + 0.1).cuda()
    for w0, k, gain in ((0, n_clips * S, amax), (2, 5, amax), (7, 1, None)):
        pred = torch.randn(k, 2, HPF, nb, generator=g).cuda()
        out = torch.full((1, 2, HPF * S * n_clips, nb), 7.0, device="cuda")
        stitch_windows(pred, gain, n_clips, S, w0, out)
        want = torch.full_like(out, 7.0)
        for i in range(k):
            w = w0 + i
            want[0, :, HPF * w:HPF * (w + 1)] = pred[i] * (gain[w // S] + 1e-7) if gain is not None else pred[i]
        assert torch.equal(out, want), (w0, k)
    # a run length that is not a multiple of 4 floats takes the scalar path: same result
    pred = torch.randn(4, 2, 3, 5, generator=g).cuda()
    out = stitch_windows(pred, amax, 2, 2)
    want = torch.stack([pred[i] * (amax[i // 2] + 1e-7) for i in range(4)], 1).reshape(2, 12, 5)[None]
    assert torch.equal(out, want)


@pytest.mark.parametrize("deterministic", [False, True])
def test_whole_chain_matches_the_per_clip_loop(deterministic):
    maavss_amd, model, va, stft, frames, audio, hop = _setup()
    prev = maavss_amd.set_deterministic(deterministic)
    try:
        _, _, _, st_ref, wave_ref, starts = _loop(maavss_amd, model, va, stft, frames, audio, hop)
        enh = maavss_amd.Enhancer(model, stft, T, S, HPF, video_attention=va, windows_per_launch=S)
        stitched, start = enh.enhance_stft(audio.cuda(), frames=frames.cuda())
        wave, start2 = enh(audio.cuda(), frames=frames.cuda())
    finally:
        maavss_amd.set_deterministic(prev)
    n_clips = len(starts)
    assert start == start2 == ((S - 1) // 2) * HPF * hop
    assert tuple(stitched.shape) == (1, 2, HPF * S * n_clips, FFT // 2 + 1)
    assert wave.shape[0] == hop * (n_clips * S * HPF - 1) == enh.output_length(n_clips)
    e_st = (stitched - st_ref).abs().max().item() / st_ref.abs().max().item()
    e_w = (wave - wave_ref).abs().max().item() / wave_ref.abs().max().item()
    print(f"[enhance] chain vs per-clip loop (deterministic={deterministic}): stitched {e_st:.3e}, wave {e_w:.3e} (relative max)")
    if deterministic:
        assert torch.equal(stitched, st_ref) and torch.equal(wave, wave_ref)
    assert e_st <= 1e-5 and e_w <= 1e-5


def test_windows_per_launch_does_not_change_the_result():
    maavss_amd, model, va, stft, frames, audio, hop = _setup()
    audio, frames = audio.cuda(), frames.cuda()
    outs = {}
    for wpl in (1, S, 4 * S, 5):
        enh = maavss_amd.Enhancer(model, stft, T, S, HPF, video_attention=va, windows_per_launch=wpl)
        outs[wpl] = enh(audio, frames=frames)[0]
    ref = outs[S]
    for wpl, w in outs.items():
        err = (w - ref).abs().max().item() / ref.abs().max().item()
        assert err <= 1e-5, (wpl, err)


def _oracle_chain(frames, audio, hop, attn_maps, starts):
    """fp32 CPU chain: clip_normalise_ref of the per-frame maps, stft_ref, AVFusionFramesRef (eval), times g_c, istft_ref."""
    from oracle import avse_ref_cpu as orc, stft_ref_cpu as sref, vit_ref_cpu as vref
    shapes = ([S, 2, HPF * T, FFT // 2 + 1], [S, 1, T, W, W], HPF)
    twin = orc.AVFusionFramesRef(*shapes)
    twin.load_state_dict(orc.seeded_state_dict(twin, 11), strict=True)
    twin.eval()
    clip, step = HPF * hop * TC, S * HPF * hop
    n_clips = len(starts)
    masks = torch.zeros(1, 2, HPF * S * n_clips, FFT // 2 + 1)
    gains = []
    with torch.no_grad():
        for c, v in enumerate(starts):
            x_v_clip = vref.clip_normalise_ref(attn_maps[v:v + TC])                                     # [1,TC,W,W]
            y = sref.stft_ref(audio[c * step:c * step + clip], FFT, hop)                              # [2,HPF*TC,F]
            gain = y.abs().max() + 1e-7
            y = y * (1 / gain)
            x_v = torch.stack([x_v_clip[:, j:j + T] for j in range(S)])
            x_a = torch.stack([y[:, HPF * j:HPF * (j + T)] for j in range(S)])
            a = twin(x_a, x_v)[0]
            for j in range(S):
                w = c * S + j
                masks[0, :, HPF * w:HPF * (w + 1)] = a[j]
            gains.append(gain)
    gains = torch.stack(gains)
    stitched = masks.clone()
    for c in range(n_clips):
        stitched[0, :, HPF * S * c:HPF * S * (c + 1)] *= gains[c]
    return masks, gains, stitched, sref.istft_ref(stitched, FFT, hop)[0]


def _masks(stitched, gains):
    out = stitched.clone()
    for c in range(gains.shape[0]):
        out[0, :, HPF * S * c:HPF * S * (c + 1)] /= gains[c]
    return out


@pytest.mark.parametrize("mode", ["frames", "attn"])
def test_against_the_fp32_cpu_oracle(mode):
    from oracle import vit_ref_cpu as vref
    maavss_amd, model, va, stft, frames, audio, hop = _setup(precise=(mode == "attn"))
    sd = vref.seeded_vit_state(3)
    with torch.no_grad():
        attn_ref = vref.inference_ref(sd, frames)                        # [N,1,W,W], each frame / its max
    enh = maavss_amd.Enhancer(model, stft, T, S, HPF, video_attention=va)
    n_clips, starts = enh.tiling(audio.shape[0], frames.shape[0])
    masks_ref, gains_ref, st_ref, wave_ref = _oracle_chain(frames, audio, hop, attn_ref, starts)
    if mode == "frames":
        stitched, _ = enh.enhance_stft(audio.cuda(), frames=frames.cuda())
        wave, _ = enh(audio.cuda(), frames=frames.cuda())
    else:
        stitched, _ = enh.enhance_stft(audio.cuda(), attn=attn_ref.cuda())
        wave, _ = enh(audio.cuda(), attn=attn_ref.cuda())
    _, _, amax = enh.window_inputs(audio.cuda(), attn=attn_ref.cuda())
    gains = amax.cpu() + 1e-7
    assert torch.allclose(gains, gains_ref, rtol=1e-5, atol=0)
    mse = float(((_masks(stitched.cpu(), gains) - masks_ref) ** 2).mean())
    e_w = (wave.cpu() - wave_ref).abs().max().item() / wave_ref.abs().max().item()
    print(f"[enhance] {mode}: normalised stitched STFT MSE vs the fp32 oracle {mse:.3e}; wave max rel err {e_w:.3e}")
    assert wave.shape == wave_ref.shape
    if mode == "frames":
        assert mse <= 1e-5, mse                     # the end-to-end gate of tests/test_parity_r2_gpu.py, ViT in the loop
    else:
        assert mse <= 1e-9, mse                     # exact-f32 model from the oracle's own maps


def test_non_finite_attention_raises():
    import maavss_amd
    from maavss_amd._lib import MaavssError
    from oracle import vit_ref_cpu as vref
    _, model, _, stft, frames, audio, _ = _setup()
    sd = vref.seeded_vit_state(3)
    sd["blocks.0.mlp.fc1.weight"] = sd["blocks.0.mlp.fc1.weight"] * 3e5      # the GELU hidden leaves IEEE half's range
    va = maavss_amd.VideoAttention(path_to_weights="/nonexistent.pth", act_dtype="f16")
    va.load_state_dict(sd)
    enh = maavss_amd.Enhancer(model, stft, T, S, HPF, video_attention=va)
    with pytest.raises(MaavssError, match="non-finite"):
        enh(audio.cuda(), frames=frames.cuda())
