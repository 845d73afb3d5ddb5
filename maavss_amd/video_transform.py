"""AV_Dataset's frame transform on the GPU (av_dataset.py:108-112, applied at :315-319 and :346-350): the decoder's uint8 HWC
clips -> /255 -> RandomResizedCrop(framesize, scale=(0.6, 1.0)) -> Normalize(ImageNet mean / std) [-> autocontrast], in the
f32 [F,3,S,S] layout VideoAttention.attention_frames reads.  The kernels are maavss_video_transform (include/maavss.h); the random
boxes are drawn on the host, as torchvision draws them."""
import math

import torch

from . import _lib

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class VideoTransform:
    """RandomResizedCrop(framesize, scale, ratio) + Normalize(mean, std) [+ autocontrast] for whole clips: one random box per clip,
    shared by its frames, as torchvision's transform applied to a [T,3,H,W] clip tensor does.

    antialias=False is what tensor resize did in the torchvision of the reference's time (its default became True in 0.17);
    True is the antialiased (triangle-filter) bilinear resize of a current torchvision.  autocontrast=True is the reference's
    `--autocontrast` flag (run_config.py): torchvision's autocontrast applied AFTER Normalize, as av_dataset.py:318-319 does it,
    so with it the frames are no longer ImageNet-normalised but stretched to [0, 1] per (frame, channel) plane."""

    def __init__(self, framesize, scale=(0.6, 1.0), ratio=(3 / 4, 4 / 3), mean=IMAGENET_MEAN, std=IMAGENET_STD, antialias=False,
                 autocontrast=False, device="cuda"):
        framesize = int(framesize)
        if framesize < 8 or framesize % 4:
            raise ValueError(f"framesize must be >= 8 and a multiple of 4, got {framesize}")
        if len(mean) != 3 or len(std) != 3 or any(float(s) == 0.0 for s in std):
            raise ValueError("mean and std need 3 channels, std non-zero")
        if not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]):
            raise ValueError(f"bad scale {scale} or ratio {ratio}")
        self.size = framesize
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        self.antialias, self.autocontrast = bool(antialias), bool(autocontrast)
        self.device = torch.device(device)

    def sample_boxes(self, n_clips, H0, W0, generator=None):
        """-> CPU int32 [n_clips, 4] of (top, left, height, width): torchvision's RandomResizedCrop.get_params once per clip -- up to
        10 attempts of area * U(scale) and exp(U(log ratio)), w / h = round(sqrt(...)), randint top / left, else the central-crop
        fallback -- drawing in the same order from `generator` (the global RNG when None).  With the global RNG this is meant to
        reproduce torchvision's boxes call for call; that has not been checked against torchvision itself, which is not a dependency."""
        H0, W0 = int(H0), int(W0)
        if n_clips < 0 or H0 < 1 or W0 < 1:
            raise ValueError(f"bad sample_boxes arguments ({n_clips}, {H0}, {W0})")
        area = H0 * W0
        log_ratio = torch.log(torch.tensor(self.ratio))
        out = torch.empty(n_clips, 4, dtype=torch.int32)
        for c in range(n_clips):
            out[c] = torch.tensor(self._get_params(H0, W0, area, log_ratio, generator), dtype=torch.int32)
        return out

    def _get_params(self, height, width, area, log_ratio, g):
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(self.scale[0], self.scale[1], generator=g).item()
            aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0].item(), log_ratio[1].item(), generator=g)).item()
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if 0 < w <= width and 0 < h <= height:
                i = torch.randint(0, height - h + 1, size=(1,), generator=g).item()
                j = torch.randint(0, width - w + 1, size=(1,), generator=g).item()
                return i, j, h, w
        in_ratio = float(width) / float(height)
        if in_ratio < min(self.ratio):
            w = width
            h = int(round(w / min(self.ratio)))
        elif in_ratio > max(self.ratio):
            h = height
            w = int(round(h * max(self.ratio)))
        else:
            w, h = width, height
        return (height - h) // 2, (width - w) // 2, h, w

    def check(self, video_u8, boxes, clip_frames=1):
        """Host-side validation (no device work): -> (frames [F,H0,W0,3] view, clip_frames, CPU int32 contiguous boxes)."""
        if not isinstance(video_u8, torch.Tensor) or video_u8.dtype != torch.uint8:
            raise ValueError(f"video must be a uint8 tensor, got {getattr(video_u8, 'dtype', type(video_u8))}")
        if video_u8.dim() not in (4, 5) or video_u8.shape[-1] != 3:
            raise ValueError(f"video must be HWC uint8 [F,H,W,3] or [B,T,H,W,3], got {tuple(video_u8.shape)}")
        if not video_u8.is_contiguous():
            raise ValueError("video must be contiguous")
        if video_u8.dim() == 5:
            t = video_u8.shape[1]
            if clip_frames not in (1, t):
                raise ValueError(f"clip_frames = {clip_frames} conflicts with the [B,T={t},H,W,3] input")
            clip_frames = t
            video_u8 = video_u8.view(-1, *video_u8.shape[2:])
        f, h0, w0, _ = video_u8.shape
        clip_frames = int(clip_frames)
        if f < 1 or clip_frames < 1 or f % clip_frames:
            raise ValueError(f"{f} frames are not a whole number of clips of {clip_frames} frames")
        if boxes is None:
            return video_u8, clip_frames, None
        if not isinstance(boxes, torch.Tensor) or boxes.device.type != "cpu" or boxes.dtype.is_floating_point or boxes.dtype == torch.bool:
            raise ValueError("boxes must be a CPU integer tensor [n_clips, 4]")
        n = f // clip_frames
        if tuple(boxes.shape) != (n, 4):
            raise ValueError(f"boxes must be [{n}, 4] (one per clip), got {tuple(boxes.shape)}")
        b = boxes.to(torch.int64)
        top, left, h, w = b.unbind(1)
        bad = (h < 1) | (w < 1) | (top < 0) | (left < 0) | (top + h > h0) | (left + w > w0)
        if bool(bad.any()):
            k = int(bad.nonzero()[0, 0])
            raise ValueError(f"box {k} = {tuple(boxes[k].tolist())} (top, left, h, w) is not inside the {h0}x{w0} frame")
        return video_u8, clip_frames, boxes.to(torch.int32).contiguous()

    def __call__(self, video_u8, boxes=None, clip_frames=1, out=None, generator=None):
        """video_u8: uint8 device tensor [F,H0,W0,3] (clips of `clip_frames` consecutive frames) or [B,T,H0,W0,3] (clip_frames = T).
        boxes: CPU int tensor [F / clip_frames, 4] of (top, left, height, width), sampled with `generator` when None.  Returns f32
        [F,3,S,S] (into `out` when given).  Everything is checked before any device work; the boxes reach the device through
        pinned memory without a synchronisation, and all work goes to the current stream."""
        frames, clip_frames, boxes = self.check(video_u8, boxes, clip_frames)
        f, h0, w0, _ = frames.shape
        if boxes is None:
            boxes = self.sample_boxes(f // clip_frames, h0, w0, generator)
        s = self.size
        if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != (f, 3, s, s) or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous f32 [{f},3,{s},{s}] tensor")
        _lib.require_cuda(frames, out)
        dev = frames.device
        if self.device.index is not None and dev != self.device:
            raise ValueError(f"video is on {dev}, the transform was built for {self.device}")
        if out is None:
            out = torch.empty(f, 3, s, s, device=dev, dtype=torch.float32)
        nbytes = _lib.query("maavss_video_transform_ws_bytes", f, clip_frames, h0, w0, s, int(self.antialias), int(self.autocontrast))
        if nbytes < 0:
            raise ValueError(f"unsupported transform shape: {f} frames of {h0}x{w0}, clips of {clip_frames}, S = {s}")
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        dev_boxes = torch.empty_like(boxes, device=dev)
        dev_boxes.copy_(boxes.pin_memory(), non_blocking=True)
        _lib.call("maavss_video_transform", _lib.ptr(frames), _lib.ptr(dev_boxes), boxes.data_ptr(), _lib.ptr(out), _lib.ptr(ws), nbytes, f,
                  clip_frames, h0, w0, s, *self.mean, *self.std, int(self.antialias), int(self.autocontrast), _lib.stream_ptr())
        return out
