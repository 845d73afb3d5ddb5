"""The images of the reference's training callback (train_avse_frames.py:191-215) as RGBA bytes made on the device (csrc/figures.hip):
the target and predicted STFT (utilities.stft_ae_image_callback), magnitude and unwrapped-phase spectrograms of the two waveforms
(utilities.plot_waveform_specgram -> Axes.specgram) and the filmstrip of video, target attention and predicted attention
(utilities.video_frames_image).  Every pixel is what matplotlib's colour mapping gives for the same array: include/maavss.h states the
definitions, tests/figures_twin.py restates them in float64.  Nothing here waits for the device: every function only enqueues launches
on the current stream and returns device uint8 tensors; save_png (host side) is the one place that copies."""
import os

import torch

from ._lib import call, ptr, query, require_cuda, stream_ptr, wave_rows

IMAGE_KEYS = ("stft", "input_mag", "input_phase", "output_mag", "output_phase", "attention_frames")
_DTYPES = {torch.float32: 0, torch.float64: 1}


def _scale(scale):
    if (not isinstance(scale, (tuple, list)) or len(scale) != 2
            or any(isinstance(s, bool) or not isinstance(s, int) or not 1 <= s <= 64 for s in scale)):
        raise ValueError(f"scale must be two integers (rows, columns) in 1 .. 64, got {scale!r}")
    return int(scale[0]), int(scale[1])


def _limit(v, what):
    if v is None:
        return 0.0
    if isinstance(v, torch.Tensor) or isinstance(v, bool):
        raise ValueError(f"{what} must be a Python number or None (a device range is what the autoscale computes), got {type(v).__name__}")
    v = float(v)
    if v != v or v in (float("inf"), float("-inf")):
        raise ValueError(f"{what} must be finite, got {v}")
    return v


def viridis_image(x, vmin=None, vmax=None, *, transpose=False, flip_rows=False, scale=(1, 1), out=None):
    """x: f32 or f64 cuda [H, W] or [N, H, W] with any element strides >= 0 (a view such as y_stft[0, 0] or a transpose is taken as it is)
    -> uint8 [..., H sy, W sx, 4]: cm.viridis(Normalize(vmin, vmax)(masked_invalid(x)), bytes=True) per image.  vmin / vmax None: the
    image's minimum / maximum over its finite elements, which stay on the device.  A non-finite element gives (0, 0, 0, 0).  `transpose`
    and `flip_rows` act on the image before the nearest replication by `scale`.  `out`: a contiguous uint8 tensor of the result's shape
    to write into."""
    if not isinstance(x, torch.Tensor) or x.dtype not in _DTYPES or x.dim() not in (2, 3):
        raise ValueError(f"x must be a float32 or float64 tensor [H, W] or [N, H, W], got {tuple(getattr(x, 'shape', ()))} {getattr(x, 'dtype', type(x))}")
    sy, sx = _scale(scale)
    lo, hi = _limit(vmin, "vmin"), _limit(vmax, "vmax")
    if vmin is not None and vmax is not None and lo > hi:
        raise ValueError(f"vmin = {lo} is above vmax = {hi}")
    single = x.dim() == 2
    xs = x[None] if single else x
    n, h, w = xs.shape
    if n < 1 or h < 1 or w < 1:
        raise ValueError(f"x is empty: {tuple(x.shape)}")
    if any(s < 0 for s in xs.stride()):
        raise ValueError(f"x has a negative stride: {xs.stride()}")
    require_cuda(xs)
    hi_, wi_ = (w, h) if transpose else (h, w)
    shape = (n, hi_ * sy, wi_ * sx, 4)
    if out is None:
        res = torch.empty(shape, dtype=torch.uint8, device=xs.device)
    else:
        want = shape[1:] if single else shape
        if out.dtype != torch.uint8 or tuple(out.shape) != want or not out.is_contiguous() or out.device != xs.device:
            raise ValueError(f"out must be a contiguous uint8 tensor {want} on {xs.device}, got {tuple(out.shape)} {out.dtype}")
        res = out
    dt, st = _DTYPES[xs.dtype], stream_ptr()
    sn = xs.stride(0) if n > 1 else 0
    fixed = (1 if vmin is not None else 0) | (2 if vmax is not None else 0)
    rng = None
    if fixed != 3:
        rng = torch.empty(n, 2, dtype=torch.float64, device=xs.device)
        call("maavss_viridis_range", ptr(xs), dt, n, h, w, sn, xs.stride(1), xs.stride(2), ptr(rng), st)
    call("maavss_viridis_image", ptr(xs), dt, n, h, w, sn, xs.stride(1), xs.stride(2), ptr(rng), fixed, lo, hi, int(bool(transpose)),
         int(bool(flip_rows)), sy, sx, ptr(res), st)
    if out is not None:
        return out
    return res[0] if single else res


def specgram_planes(wave, nfft=256, noverlap=128):
    """wave: f32 cuda [L] or [B, L], samples contiguous, any row stride >= 0 (rows may overlap) and any 4-byte-aligned offset
    -> (mag_db, phase), both f64 [B, nfft / 2 + 1, n]: the arrays Axes.specgram(x, mode='magnitude') and (mode='phase') hand to imshow
    with matplotlib's other defaults (Hann window, no detrending, one-sided, dB, np.unwrap along frequency, row 0 the Nyquist bin).
    nfft: a power of two in 32 .. 1024; 0 <= noverlap < nfft."""
    wave = wave_rows(wave, "wave")
    for v, what in ((nfft, "nfft"), (noverlap, "noverlap")):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{what} must be an integer, got {v!r}")
    if nfft < 32 or nfft > 1024 or nfft & (nfft - 1):
        raise ValueError(f"nfft = {nfft} must be a power of two in 32 .. 1024")
    if not 0 <= noverlap < nfft:
        raise ValueError(f"noverlap = {noverlap} must be in [0, nfft = {nfft})")
    require_cuda(wave)
    b, length = wave.shape
    n = int(query("maavss_specgram_segments", b, length, nfft, noverlap))
    if n < 1:
        raise ValueError(f"specgram_planes: {b} rows of {length} samples are beyond the kernel's index range")
    planes = torch.empty(2, b, nfft // 2 + 1, n, dtype=torch.float64, device=wave.device)
    call("maavss_specgram", ptr(wave), wave.stride(0), b, length, nfft, noverlap, ptr(planes[0]), ptr(planes[1]), stream_ptr())
    return planes[0], planes[1]


def specgram_images(wave, nfft=256, noverlap=128, scale=(1, 1)):
    """-> (mag_image, phase_image), uint8 [B, (nfft / 2 + 1) sy, n sx, 4] ([..] without B for a [L] wave): the two planes of
    specgram_planes through viridis_image, every image autoscaled on its own as imshow does.  -inf dB of a silent segment and the NaNs
    of a non-finite sample are transparent pixels."""
    single = isinstance(wave, torch.Tensor) and wave.dim() == 1
    mag, phase = specgram_planes(wave, nfft, noverlap)
    imgs = tuple(viridis_image(p, scale=scale) for p in (mag, phase))
    return tuple(i[0] for i in imgs) if single else imgs


def stft_panels(y_stft, yh_stft):
    """utilities.stft_ae_image_callback (utilities.py:328-356): y_stft, yh_stft f32 cuda [2, T_a, F] (any strides >= 0) -> uint8
    [4, F, T_a, 4]: y real, y imag, y-hat real, y-hat imag, each transposed and autoscaled on its own like plt.imshow(y_stft_ex[0].T)."""
    for t, what in ((y_stft, "y_stft"), (yh_stft, "yh_stft")):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[0] != 2:
            raise ValueError(f"{what} must be [2, T_a, F], got {tuple(getattr(t, 'shape', ()))}")
    if y_stft.shape != yh_stft.shape:
        raise ValueError(f"y_stft {tuple(y_stft.shape)} and yh_stft {tuple(yh_stft.shape)} differ in shape")
    _, t_a, f = y_stft.shape
    out = torch.empty(4, f, t_a, 4, dtype=torch.uint8, device=y_stft.device)
    viridis_image(y_stft.detach(), transpose=True, out=out[:2])
    viridis_image(yh_stft.detach(), transpose=True, out=out[2:])
    return out


def filmstrip_image(y_attn, yh_attn, video=None):
    """utilities.video_frames_image with generate_filmstrip(..., resize=False) (utilities.py:286-326): y_attn, yh_attn f32 cuda
    [1, T, H, W], video [3, T, H, W] or None -> uint8 [R H, T W, 4], strips from the top: video (when given), y, y-hat.  Each tensor
    times 1 / (its max + 1e-7), clipped to [0, 1], in f32 as the reference forms it; attention through viridis with vmin = -1,
    vmax = 1, video as trunc(255 v) RGB.  Unlike the reference, which scales its arguments in place, the inputs are left unchanged;
    frames may be rectangular."""
    for t, what in ((y_attn, "y_attn"), (yh_attn, "yh_attn")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.shape[0] != 1:
            raise ValueError(f"{what} must be a float32 tensor [1, T, H, W], got {tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))}")
    if y_attn.shape != yh_attn.shape:
        raise ValueError(f"y_attn {tuple(y_attn.shape)} and yh_attn {tuple(yh_attn.shape)} differ in shape")
    _, t, h, w = y_attn.shape
    if min(t, h, w) < 1:
        raise ValueError(f"y_attn is empty: {tuple(y_attn.shape)}")
    if video is not None and (not isinstance(video, torch.Tensor) or video.dtype != torch.float32 or tuple(video.shape) != (3, t, h, w)):
        raise ValueError(f"video must be a float32 tensor {(3, t, h, w)}, got {tuple(getattr(video, 'shape', ()))} {getattr(video, 'dtype', type(video))}")
    require_cuda(y_attn, yh_attn, video)
    y_attn, yh_attn = y_attn.detach().contiguous(), yh_attn.detach().contiguous()
    video = None if video is None else video.detach().contiguous()
    rows = 3 if video is not None else 2
    out = torch.empty(rows * h, t * w, 4, dtype=torch.uint8, device=y_attn.device)
    maxes = torch.empty(192, dtype=torch.float32, device=y_attn.device)                  # 64 partial maxima per tensor
    call("maavss_filmstrip", ptr(y_attn), ptr(yh_attn), ptr(video), t, h, w, ptr(maxes), ptr(out), stream_ptr())
    return out


class CallbackFigures:
    """The dict the reference logs every cb_freq steps (train_avse_frames.py:191-215) for one clip of the batch, made on the device.

        figures = CallbackFigures(stft)
        losses, output_stft, output_attn = step.sliding_window_step(x_stft, y_stft, attn, attn, nf, hpf, collect=True)
        logs = figures(y_stft, output_stft, attn, output_attn, video=None)      # launches only; copy when you like
        save_png(logs, "figures", i)

    y_stft [B, 2, T_a, F] and attn [B, 1, T, H, W] are the clip's targets; output_stft [B, 2, hpf num_seq, F] and output_attn
    [B, 1, num_seq, H, W] the stitched outputs of sliding_window_step(collect=True).  As the reference does (:195-197), the targets
    are cut to the num_seq middle frames the outputs cover, from idx_mid = (num_seq - 1) // 2 (a target that already has the outputs'
    length is taken whole).  video: [B, 3, T, H, W] or None."""

    def __init__(self, stft, nfft=256, noverlap=128, scale=(1, 1)):
        self.stft, self.nfft, self.noverlap, self.scale = stft, nfft, noverlap, _scale(scale)

    def __call__(self, y_stft, output_stft, attn, output_attn, video=None, clip=0):
        num_seq = output_attn.shape[2]
        idx_mid = (num_seq - 1) // 2
        rows = output_stft.shape[2]
        if rows % num_seq:
            raise ValueError(f"output_stft has {rows} STFT frames, no multiple of output_attn's {num_seq} video frames")
        hpf = rows // num_seq

        def middle(t, dim, start, count, what):
            if t.shape[dim] == count:
                return t
            if t.shape[dim] < start + count:
                raise ValueError(f"{what} has {t.shape[dim]} frames, fewer than the {start} + {count} the outputs cover")
            return t.narrow(dim, start, count)

        y = middle(y_stft[clip], 1, idx_mid * hpf, rows, "y_stft").detach()
        yh = output_stft[clip].detach()
        a = middle(attn[clip], 1, idx_mid, num_seq, "attn").detach()
        ah = output_attn[clip].detach()
        v = None if video is None else middle(video[clip], 1, idx_mid, num_seq, "video").detach()
        waves = self.stft.inverse(torch.stack((y, yh)))                          # [2, hop (rows - 1)]: one launch for both waveforms
        mag, phase = specgram_images(waves, self.nfft, self.noverlap, self.scale)
        return {"stft": stft_panels(y, yh), "input_mag": mag[0], "input_phase": phase[0], "output_mag": mag[1], "output_phase": phase[1],
                "attention_frames": filmstrip_image(a, ah, v), "audio_input": waves[0], "audio_output": waves[1]}


def save_png(figures, directory, step):
    """Host side: one device-to-host copy per image of `figures` (a CallbackFigures dict, or any dict of uint8 [H, W, 4] or [K, H, W, 4]
    tensors; other entries are skipped), written as <directory>/<key>_<step>.png with PIL; the K panels of a [K, H, W, 4] entry ("stft")
    side by side, as the reference's subplots stand.  -> the list of paths."""
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    paths = []
    for key, img in figures.items():
        if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 4:
            continue
        arr = img.cpu().numpy()
        if arr.ndim == 4:
            arr = arr.transpose(1, 0, 2, 3).reshape(arr.shape[1], arr.shape[0] * arr.shape[2], 4)
        path = os.path.join(directory, f"{key}_{int(step):06d}.png")
        Image.fromarray(arr, "RGBA").save(path)
        paths.append(path)
    return paths
