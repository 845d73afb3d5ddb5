"""Drop-in `VideoAttention` (reference video_attention.py:24) on the MI355X HIP kernels.

Same constructor arguments and `_inference(frames [T,3,H,W]) -> [T,1,H,W]` contract (CPU float32 result, like
the reference which fills a CPU tensor frame by frame, video_attention.py:39,96); adds the batched entry
point `attention_frames(frames [F,3,H,W], clip_frames)` that keeps everything on the GPU and also applies the
per-clip normalisation of av_dataset.py:328.  The ViT-S/8 (dino.vision_transformer.vit_small(patch_size=8,
num_classes=0), an un-vendored submodule of the reference) is restated from its published architecture:
`self.model` is a plain state-dict holder with DINO's key names, so a DINO checkpoint
(`dino_deitsmall8_pretrain.pth`, key "teacher", prefixes "module."/"backbone." stripped -- video_attention.py:
116-129) loads unchanged.  architecture="vit_base" builds DINO's other patch-8 backbone, ViT-B/8
(`dino_vitbase8_pretrain.pth`: width 768, 12 heads, MLP 3072), on the width-generic kernels (`_cls_attention_generic`).
There is no network in this environment: if the weights file is absent the extractor keeps its seeded random
initialisation and says so (the reference would try to download).

The sort/cumsum/threshold block of the reference (video_attention.py:59-78) -- DINO's per-head segmentation masks, which the
reference computes and then discards -- never influences the returned frames, so `_inference` / `attention_frames` do not
compute it; `attention_masks` returns it on request (one HIP kernel, maavss_vit_attn_masks), with the constructor's `threshold`.
"""
import math
import os
import sys
from typing import NamedTuple

import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

DIM, DEPTH, HEADS, MLP, PATCH = 384, 12, 6, 1536, 8
LN_EPS = 1e-6
EPI_BF16_BIAS, EPI_BF16_BIAS_GELU, EPI_F32_BIAS_RESID, EPI_F32_ROWTABLE = 0, 1, 2, 3
# 16-bit storage / MFMA operand format of the extractor (include/maavss.h `dtype`)
DT_BF16, DT_F16 = 0, 2
_TORCH_DT = {DT_BF16: torch.bfloat16, DT_F16: torch.float16}


class ViTSpec(NamedTuple):
    dim: int
    heads: int
    mlp: int
    depth: int
    checkpoint: str       # DINO's published file of this backbone at patch 8


# The DINO patch-8 backbones the extractor builds.  vit_tiny (192 wide, 3 heads) is refused: DINO publishes no checkpoint for it,
# and its widths 192 / 576 fall outside the N % 128 tiling of the generic GEMM.
VIT_SPECS = {"vit_small": ViTSpec(DIM, HEADS, MLP, DEPTH, "dino_deitsmall8_pretrain.pth"),
             "vit_base": ViTSpec(768, 12, 3072, 12, "dino_vitbase8_pretrain.pth")}


def vit_shapes(architecture="vit_small", img_size=224):
    """DINO state-dict keys and shapes of one backbone (pos_embed for img_size^2 frames)."""
    d, _, mlp, depth, _ = VIT_SPECS[architecture]
    n = (img_size // PATCH) ** 2
    sh = {"cls_token": (1, 1, d), "pos_embed": (1, n + 1, d),
          "patch_embed.proj.weight": (d, 3, PATCH, PATCH), "patch_embed.proj.bias": (d,),
          "norm.weight": (d,), "norm.bias": (d,)}
    for i in range(depth):
        p = f"blocks.{i}."
        sh.update({p + "norm1.weight": (d,), p + "norm1.bias": (d,),
                   p + "attn.qkv.weight": (3 * d, d), p + "attn.qkv.bias": (3 * d,),
                   p + "attn.proj.weight": (d, d), p + "attn.proj.bias": (d,),
                   p + "norm2.weight": (d,), p + "norm2.bias": (d,),
                   p + "mlp.fc1.weight": (mlp, d), p + "mlp.fc1.bias": (mlp,),
                   p + "mlp.fc2.weight": (d, mlp), p + "mlp.fc2.bias": (d,)})
    return sh


def vit_small_shapes(img_size=224):
    return vit_shapes("vit_small", img_size)


class DinoViTWeights:
    """State-dict holder for the frozen ViT (the object the reference exposes as `VideoAttention.model`), DINO key names."""

    def __init__(self, architecture="vit_small", seed=0):
        self.architecture, self.spec = architecture, VIT_SPECS[architecture]
        g = torch.Generator().manual_seed(seed)
        self.sd = {}
        for k, shape in vit_shapes(architecture).items():
            if k.endswith("norm1.weight") or k.endswith("norm2.weight") or k == "norm.weight":
                t = torch.ones(shape)
            elif k.endswith(".bias"):
                t = torch.zeros(shape)
            else:
                t = torch.randn(shape, generator=g) * 0.02       # DINO's trunc_normal_(std=.02) scale
            self.sd[k] = t
        self.loaded_from = None

    def state_dict(self):
        return dict(self.sd)

    def load_state_dict(self, state_dict, strict=True):
        missing = [k for k in self.sd if k not in state_dict]
        unexpected = [k for k in state_dict if k not in self.sd]
        width = next((int(state_dict[k].shape[-1]) for k in ("cls_token", "patch_embed.proj.bias") if k in state_dict), self.spec.dim)
        if width != self.spec.dim:
            # the common case: the reference's default path (dino_deitsmall8_pretrain.pth, width 384) under architecture="vit_base"
            other = next((f" (a {a} checkpoint such as {s.checkpoint})" for a, s in VIT_SPECS.items() if s.dim == width), "")
            raise RuntimeError(f"ViT checkpoint of width {width}{other} does not fit architecture={self.architecture!r}, which is "
                               f"{self.spec.dim} wide: load {self.spec.checkpoint}")
        if strict and (missing or unexpected):
            raise RuntimeError(f"ViT state_dict mismatch: missing {missing[:4]}..., unexpected {unexpected[:4]}...")
        for k in self.sd:
            if k in state_dict:
                t = torch.as_tensor(state_dict[k]).detach().float().cpu()
                if k == "pos_embed":
                    # any token count (interpolated per resolution), but a [1, n + 1, dim] table of this backbone's width
                    if t.dim() != 3 or t.shape[0] != 1 or t.shape[2] != self.spec.dim:
                        raise RuntimeError(f"pos_embed of shape {tuple(t.shape)} does not fit architecture={self.architecture!r}: "
                                           f"expected [1, tokens, {self.spec.dim}]")
                elif tuple(t.shape) != tuple(self.sd[k].shape):
                    raise RuntimeError(f"shape mismatch for {k}: {tuple(t.shape)} vs {tuple(self.sd[k].shape)}")
                self.sd[k] = t.clone()
        return missing, unexpected

    def eval(self):
        return self

    def to(self, *a, **k):
        return self


class ViTSmall8Weights(DinoViTWeights):
    def __init__(self, seed=0):
        super().__init__("vit_small", seed)


def interpolate_pos_embed(pos_embed, h_tok, w_tok):
    """Host-side, once per resolution: DINO's bicubic resize of the patch position embedding (incl. its +0.1)."""
    n, d = pos_embed.shape[1] - 1, pos_embed.shape[2]
    if n == h_tok * w_tok and h_tok == w_tok:
        return pos_embed
    side = int(math.sqrt(n))
    patch = pos_embed[:, 1:].reshape(1, side, side, d).permute(0, 3, 1, 2)
    patch = torch.nn.functional.interpolate(patch, scale_factor=((h_tok + 0.1) / side, (w_tok + 0.1) / side),
                                            mode="bicubic")
    patch = patch.permute(0, 2, 3, 1).reshape(1, -1, d)
    return torch.cat([pos_embed[:, :1], patch], 1)


class VideoAttention:
    def __init__(self, patch_size=8, threshold=0.6, path_to_weights="dino_deitsmall8_pretrain.pth",
                 architecture="vit_small", resize=None, device="cuda", frames_per_launch=512, act_dtype="f16",
                 attn_dtype=None, fp8_blocks=None, gelu="f32", qkv_ln=None):
        if patch_size != PATCH:
            raise ValueError(f"patch_size={patch_size!r}: only DINO's patch-8 backbones are built (the reference uses patch 8, "
                             "av_dataset.py:50; the patchify and attention-map kernels are specialised to 8x8 patches)")
        if architecture == "vit_tiny":
            raise ValueError("architecture='vit_tiny' is not built: DINO publishes no vit_tiny checkpoint, and its widths 192 / 576 fall "
                             "outside the N % 128 tiling of the ViT GEMM")
        if architecture not in VIT_SPECS:
            raise ValueError(f"architecture={architecture!r}: choose one of {sorted(VIT_SPECS)}")
        self.architecture, self.spec = architecture, VIT_SPECS[architecture]
        if architecture != "vit_small":
            # the fp8 attention images, the packed-half GELU and the gamma-folded qkv live in the weight-stationary K = 384 kernels
            # (widths 384 / 1152 hard-wired): the other backbones run the width-generic kernels only
            why = f"is built for vit_small only (its kernels are hard-wired to width 384 / 1152), not for architecture={architecture!r}"
            if attn_dtype in ("fp8", "fp8-late"):
                raise ValueError(f"attn_dtype={attn_dtype!r} {why}")
            if fp8_blocks is not None:
                raise ValueError(f"fp8_blocks {why}")
            if gelu == "half":
                raise ValueError(f"gelu='half' {why}")
            if qkv_ln == "post":
                raise ValueError(f"qkv_ln='post' {why}")
            qkv_ln = "pre"           # the MAAVSS_QKV_LN environment default concerns the vit_small kernels only
        self.resize, self.threshold, self.patch_size = resize, threshold, patch_size
        # Keyword-only in spirit (not in the reference signature): storage format of weights and activations between the
        # kernels.  "f16" (default) = IEEE half: same MFMA rate as bf16, 8x smaller rounding error -- the difference
        # between an end-to-end mask-MSE of 1.7e-4 (bf16) and 7e-6 (f16) against the fp32 reference chain;
        # "bf16" keeps bf16's exponent range for checkpoints with out-of-range activations.
        if act_dtype not in ("f16", "bf16"):
            raise ValueError("act_dtype must be 'f16' or 'bf16'")
        self.act_dtype = act_dtype
        self.dt = DT_F16 if act_dtype == "f16" else DT_BF16
        # attn_dtype="fp8": Q K^T and P V of the 11 full blocks on the block-scaled fp8 MFMA (OCP MX: e4m3 with one e8m0 scale
        # per 32 elements, v_mfma_scale_f32_32x32x64_f8f6f4; BASELINE config "fp8 MFMA attention"); the attn.qkv GEMM writes the
        # quantised operand images directly.  None = the activation format.  The last block's CLS row stays 16-bit.
        # attn_dtype="fp8-late" (round 4): the same kernels in blocks 8-10 only.  The per-operand / per-block ablation on the CPU oracle
        # (profiles/r4_fp8_operand_ablation.txt) shows the end-to-end error of the fp8 mode is made in the EARLY blocks (all four
        # operands in blocks 0-5: mask-MSE 3.6e-3, block 0 alone 1.7e-3; blocks 6-10: 1.4e-4; blocks 8-10: 4e-5): the late-block hybrid
        # is the fp8 mode with a stated tolerance (end-to-end mask-MSE <= 1e-4, tests/test_parity_r4_gpu.py).  `fp8_blocks` = an explicit
        # set of block indices (0..10) overrides either default.
        if attn_dtype not in (None, "fp8", "fp8-late", act_dtype):
            raise ValueError("attn_dtype must be None, 'fp8', 'fp8-late' or equal to act_dtype")
        self.attn_fp8 = attn_dtype in ("fp8", "fp8-late")
        if fp8_blocks is None:
            fp8_blocks = range(DEPTH - 1) if attn_dtype == "fp8" else ((8, 9, 10) if attn_dtype == "fp8-late" else ())
        self.fp8_blocks = frozenset(int(i) for i in fp8_blocks)
        if self.fp8_blocks and not self.attn_fp8:
            raise ValueError("fp8_blocks needs attn_dtype='fp8' or 'fp8-late'")
        if any(i < 0 or i >= DEPTH - 1 for i in self.fp8_blocks):
            raise ValueError(f"fp8_blocks must be block indices 0..{DEPTH - 2} (the last block only computes the CLS attention row, in 16 bits)")
        # gelu="half" (round 4, IEEE-half storage only): mlp.fc1's GELU polynomial evaluated in packed half instead of f32 -- fc1 543 -> 504 us
        # per launch (packed-half vector instructions overlap with the matrix pipe), at twice the rounding error of the stored
        # hidden activation: end-to-end mask-MSE 3.8e-6 ... 8.4e-6 over three seed sets against 3.0e-6 ... 6.5e-6 -- inside 1e-5 with less
        # margin, so it is a selectable mode (bench.py --vit-gelu half), not the default.
        if gelu not in ("f32", "half") or (gelu == "half" and act_dtype != "f16"):
            raise ValueError("gelu must be 'f32' or 'half' (the latter with act_dtype='f16' only)")
        self.gelu_epilogue = 4 if gelu == "half" else EPI_BF16_BIAS_GELU
        # qkv_ln (round 4): where norm1 is applied.  "pre" = on the way into the attn.qkv GEMM (the normalised rows are rounded to the storage
        # format); "post" = AFTER the product: the raw rows are rounded, the weights are the gamma-folded W diag(gamma), and the epilogue applies
        # rstd_r (x W'^T - mean_r s_n) + (b + W beta) -- the loader then has no per-element LayerNorm arithmetic (a third of the launch).  Same
        # result in exact arithmetic, another rounding realisation in 16 bits (CPU oracle, end-to-end mask-MSE: 3.0e-6 / 4.7e-6 against 6.5e-6 / 3.1e-6
        # of "pre" on the two seed sets tried).  Default: MAAVSS_QKV_LN (else "pre").
        if qkv_ln is None:
            qkv_ln = os.environ.get("MAAVSS_QKV_LN", "pre")
        if qkv_ln not in ("pre", "post"):
            raise ValueError("qkv_ln must be 'pre' or 'post'")
        self.qkv_ln = qkv_ln
        self.checkpoint_key = "teacher"
        self.device = torch.device(device)
        self.frames_per_launch = frames_per_launch
        self.model = self.__load_model(path_to_weights)
        self._dev = None          # device-side weight images, built lazily
        self._tables = {}
        # range guard of the 16-bit storage (see attention_frames): sticky device flag + the pinned host copy of the last call
        self._flag, self._flag_pending, self._flag_hosts = None, [], []
        self._mx_ws = {}          # (rows, stream) -> zero-initialised workspace of the fp8 operand images (tails must stay zero); at most 4, LRU

    def __load_model(self, pretrained_weights):
        model = ViTSmall8Weights() if self.architecture == "vit_small" else DinoViTWeights(self.architecture)
        if os.path.isfile(pretrained_weights):
            sd = torch.load(pretrained_weights, map_location="cpu", weights_only=True)
            if self.checkpoint_key is not None and self.checkpoint_key in sd:
                sd = sd[self.checkpoint_key]
            sd = {k.replace("module.", "").replace("backbone.", ""): v for k, v in sd.items()}
            model.load_state_dict(sd, strict=False)
            model.loaded_from = pretrained_weights
        else:
            print(f"[maavss_amd] DINO weights '{pretrained_weights}' not found and there is no network: "
                  f"VideoAttention keeps its random initialisation (load one with .model.load_state_dict).", file=sys.stderr)
        return model

    def load_state_dict(self, sd, strict=True):
        out = self.model.load_state_dict(sd, strict)
        self._dev, self._tables = None, {}
        return out

    # ---- device images of the frozen weights -------------------------------------------------------
    def _device_weights(self):
        if self._dev is None:
            sd, dev = self.model.sd, self.device
            bf = lambda t: t.to(dev).to(_TORCH_DT[self.dt]).contiguous()  # one-off dtype conversion of frozen weights
            f32 = lambda t: t.to(dev).float().contiguous()
            d = {"patch_w": bf(sd["patch_embed.proj.weight"].reshape(self.spec.dim, 192))}
            for i in range(self.spec.depth):
                p = f"blocks.{i}."
                d[i] = dict(n1w=f32(sd[p + "norm1.weight"]), n1b=f32(sd[p + "norm1.bias"]),
                            qkv_w=bf(sd[p + "attn.qkv.weight"]), qkv_b=f32(sd[p + "attn.qkv.bias"]),
                            proj_w=bf(sd[p + "attn.proj.weight"]), proj_b=f32(sd[p + "attn.proj.bias"]),
                            n2w=f32(sd[p + "norm2.weight"]), n2b=f32(sd[p + "norm2.bias"]),
                            fc1_w=bf(sd[p + "mlp.fc1.weight"]), fc1_b=f32(sd[p + "mlp.fc1.bias"]),
                            fc2_w=bf(sd[p + "mlp.fc2.weight"]), fc2_b=f32(sd[p + "mlp.fc2.bias"]))
                if self.qkv_ln == "post":
                    # W' = W diag(gamma) in the storage format, s_n = row sums of the ROUNDED W' (f32), b' = b + W beta (exact weights, f64 sums)
                    w64 = sd[p + "attn.qkv.weight"].double()
                    wf = bf((w64 * sd[p + "norm1.weight"].double()[None, :]).float())
                    d[i]["qkv_wf"] = wf
                    d[i]["qkv_cs"] = wf.float().sum(-1).contiguous()
                    d[i]["qkv_bf"] = f32((sd[p + "attn.qkv.bias"].double() + w64 @ sd[p + "norm1.bias"].double()).float())
            self._dev = d
        return self._dev

    def _row_table(self, h_tok, w_tok):
        """[ntok][dim] f32: row 0 = cls_token + pos[0]; row j = conv bias + pos[j] (prepare_tokens of DINO)."""
        key = (h_tok, w_tok)
        if key not in self._tables:
            sd = self.model.sd
            pos = interpolate_pos_embed(sd["pos_embed"], h_tok, w_tok)[0]
            table = pos + sd["patch_embed.proj.bias"][None, :]
            table[0] = pos[0] + sd["cls_token"][0, 0]
            self._tables[key] = table.float().contiguous().to(self.device)
        return self._tables[key]

    # ---- the ViT forward up to the last block's CLS attention ---------------------------------------
    def cls_attention(self, frames):
        """frames [F,3,H,W] f32 cuda (H, W multiples of 8 are used) -> [F, heads, (H//8)*(W//8)] f32 cuda (6 heads for vit_small,
        12 for vit_base)."""
        _lib.require_cuda(frames)
        assert frames.dim() == 4 and frames.shape[1] == 3 and frames.dtype == torch.float32
        frames = frames.contiguous()
        if self.architecture != "vit_small":
            return self._cls_attention_generic(frames)
        f, _, h, w = frames.shape
        hp, wp = h // PATCH, w // PATCH
        ntok = hp * wp + 1
        rows = f * ntok
        dev, st, dt, tdt = frames.device, stream_ptr(), self.dt, _TORCH_DT[self.dt]
        wts, table = self._device_weights(), self._row_table(hp, wp)
        # maavss_vit_ws_gemm reads and stores whole 64-row panels: its operands need ceil(rows / 64) * 64 allocated rows (include/maavss.h)
        rpad = (rows + 127) // 128 * 128
        a = torch.empty(rows, 192, device=dev, dtype=tdt)
        x = torch.empty(rpad, DIM, device=dev, dtype=torch.float32)
        xn = torch.empty(rpad, DIM, device=dev, dtype=tdt)
        # per-row LayerNorm partials of x over its three 128-column thirds, written by the kernels that store x (patch
        # embedding, fc2) and merged by the qkv kernel, which normalises x on the way in: norm1 never runs as a pass
        stats = torch.empty(rows, 3, 2, device=dev, dtype=torch.float32)
        qkv = torch.empty(rpad, 3 * DIM, device=dev, dtype=tdt)
        att_o = torch.empty(rpad, DIM, device=dev, dtype=tdt)
        hid = torch.empty(rpad, MLP, device=dev, dtype=tdt)
        ws8 = None
        if self.attn_fp8:
            key = (rows, torch.cuda.current_stream().cuda_stream)
            # one workspace per (rows, stream): the tail group of a batch (F % frames_per_launch) and the pipeline's side stream each
            # keep theirs -- replacing a single entry on every miss re-allocated and zero-filled 0.46 GB (1.4 GB at 384^2) per call
            ws8 = self._mx_ws.pop(key, None)
            if ws8 is None:
                while len(self._mx_ws) >= 4:
                    self._mx_ws.pop(next(iter(self._mx_ws)))          # oldest use first (dicts keep insertion order)
                ws8 = torch.zeros(_lib.query("maavss_vit_attn_mx_ws_bytes", rows), device=dev, dtype=torch.uint8)
            self._mx_ws[key] = ws8                                    # (re-)inserted last = most recently used
            # rows of the last 64-row panel past the real ones take part in V's 32-token scale blocks: keep them finite
            x[rows:].zero_()
            att_o[rows:].zero_()
        call("maavss_vit_patchify", ptr(frames), ptr(a), f, h, w, dt, st)
        call("maavss_vit_gemm_stats", ptr(a), 192, ptr(wts["patch_w"]), None, ptr(table), ntok, ptr(x), DIM, rows, DIM, 192,
             EPI_F32_ROWTABLE, 0, 1.0, ptr(stats), dt, st)
        qs = 0.125 * 1.4426950408889634          # q *= log2(e)/sqrt(64): the attention kernels run softmax on exp2
        for i in range(DEPTH):
            b = wts[i]
            # the last block only feeds the CLS-row attention (get_last_selfattention): q and k, not v -- the weight rows
            # are [q; k; v], so N = 2 DIM computes exactly those two thirds into the same [rows, 3 DIM] buffer
            nqkv = 2 * DIM if i == DEPTH - 1 else 3 * DIM
            fp8_here = i in self.fp8_blocks          # (never the last block)
            # norm1 + qkv: weights stationary in registers, x normalised on its way into LDS (row statistics from the kernel that wrote x)
            if fp8_here:
                # -> block-scaled fp8 operand images, no 16-bit qkv tensor and no quantisation pass
                call("maavss_vit_ws_gemm_ln_mx", ptr(x), rpad, ptr(stats), ptr(b["n1w"]), ptr(b["n1b"]), LN_EPS, ptr(b["qkv_w"]),
                     ptr(b["qkv_b"]), ptr(ws8), rows, DIM, qs, dt, st)
            elif self.qkv_ln == "post":
                call("maavss_vit_ws_gemm_ln_post", ptr(x), rpad, ptr(stats), ptr(b["qkv_cs"]), LN_EPS, ptr(b["qkv_wf"]), ptr(b["qkv_bf"]),
                     ptr(qkv), 3 * DIM, rpad, rows, nqkv, DIM, qs, dt, st)
            else:
                call("maavss_vit_ws_gemm_ln", ptr(x), rpad, ptr(stats), ptr(b["n1w"]), ptr(b["n1b"]), LN_EPS, ptr(b["qkv_w"]),
                     ptr(b["qkv_b"]), ptr(qkv), 3 * DIM, rpad, rows, nqkv, DIM, qs, dt, st)
            if i == DEPTH - 1:
                break
            if fp8_here:
                call("maavss_vit_attn_mx", ptr(ws8), ptr(att_o), f, ntok, HEADS, DIM, dt, st)
            else:
                call("maavss_vit_attn", ptr(qkv), ptr(att_o), f, ntok, HEADS, 3 * DIM, DIM, dt, st)
            # proj adds into the residual stream and writes norm2 of the updated rows; fc1 reads that
            call("maavss_vit_ws_gemm", ptr(att_o), DIM, rpad, ptr(b["proj_w"]), ptr(b["proj_b"]), ptr(x), DIM, rpad, rows, DIM,
                 EPI_F32_BIAS_RESID, 0, 1.0, ptr(xn), ptr(b["n2w"]), ptr(b["n2b"]), LN_EPS, dt, st)
            call("maavss_vit_ws_gemm", ptr(xn), DIM, rpad, ptr(b["fc1_w"]), ptr(b["fc1_b"]), ptr(hid), MLP, rpad, rows, MLP,
                 self.gelu_epilogue, 0, 1.0, None, None, None, LN_EPS, dt, st)
            call("maavss_vit_gemm_stats", ptr(hid), MLP, ptr(b["fc2_w"]), ptr(b["fc2_b"]), None, 0, ptr(x), DIM, rows, DIM, MLP,
                 EPI_F32_BIAS_RESID, 0, 1.0, ptr(stats), dt, st)
        att = torch.empty(f, HEADS, ntok - 1, device=dev, dtype=torch.float32)
        call("maavss_vit_cls_attn", ptr(qkv), ptr(att), f, ntok, HEADS, 3 * DIM, dt, st)
        return att

    def _cls_attention_generic(self, frames):
        """The block loop on the width-generic kernels (vit_base): LayerNorm passes of width dim, every dense layer on maavss_vit_gemm
        (N % 128, K % 64), the flash attention and the CLS row with `heads` heads.  None of these kernels reads or writes a row past
        M = frames * ntok (the GEMM clamps its A rows and guards its stores, the attention kernels clamp to the frame's last token),
        so the buffers hold exactly the real rows."""
        f, _, h, w = frames.shape
        d, heads, mlp, depth, _ = self.spec
        ntok = (h // PATCH) * (w // PATCH) + 1
        rows = f * ntok
        dev, st, dt, tdt = frames.device, stream_ptr(), self.dt, _TORCH_DT[self.dt]
        wts, table = self._device_weights(), self._row_table(h // PATCH, w // PATCH)
        a = torch.empty(rows, 192, device=dev, dtype=tdt)
        x = torch.empty(rows, d, device=dev, dtype=torch.float32)            # residual stream
        xn = torch.empty(rows, d, device=dev, dtype=tdt)
        qkv = torch.empty(rows, 3 * d, device=dev, dtype=tdt)
        att_o = torch.empty(rows, d, device=dev, dtype=tdt)
        hid = torch.empty(rows, mlp, device=dev, dtype=tdt)
        call("maavss_vit_patchify", ptr(frames), ptr(a), f, h, w, dt, st)
        call("maavss_vit_gemm", ptr(a), 192, ptr(wts["patch_w"]), None, ptr(table), ntok, ptr(x), d, rows, d, 192,
             EPI_F32_ROWTABLE, 0, 1.0, dt, st)
        qs = 0.125 * 1.4426950408889634          # q *= log2(e)/sqrt(64): the attention kernels run softmax on exp2
        for i in range(depth):
            b = wts[i]
            call("maavss_vit_layernorm", ptr(x), ptr(b["n1w"]), ptr(b["n1b"]), ptr(xn), rows, d, LN_EPS, dt, st)
            # last block: q and k only (the CLS-row attention needs no v), into the same [rows, 3 d] buffer
            nqkv = 2 * d if i == depth - 1 else 3 * d
            call("maavss_vit_gemm", ptr(xn), d, ptr(b["qkv_w"]), ptr(b["qkv_b"]), None, 0, ptr(qkv), 3 * d, rows, nqkv, d,
                 EPI_BF16_BIAS, d, qs, dt, st)
            if i == depth - 1:
                break
            call("maavss_vit_attn", ptr(qkv), ptr(att_o), f, ntok, heads, 3 * d, d, dt, st)
            call("maavss_vit_gemm", ptr(att_o), d, ptr(b["proj_w"]), ptr(b["proj_b"]), None, 0, ptr(x), d, rows, d, d,
                 EPI_F32_BIAS_RESID, 0, 1.0, dt, st)
            call("maavss_vit_layernorm", ptr(x), ptr(b["n2w"]), ptr(b["n2b"]), ptr(xn), rows, d, LN_EPS, dt, st)
            call("maavss_vit_gemm", ptr(xn), d, ptr(b["fc1_w"]), ptr(b["fc1_b"]), None, 0, ptr(hid), mlp, rows, mlp, d,
                 EPI_BF16_BIAS_GELU, 0, 1.0, dt, st)
            call("maavss_vit_gemm", ptr(hid), mlp, ptr(b["fc2_w"]), ptr(b["fc2_b"]), None, 0, ptr(x), d, rows, d, mlp,
                 EPI_F32_BIAS_RESID, 0, 1.0, dt, st)
        att = torch.empty(f, heads, ntok - 1, device=dev, dtype=torch.float32)
        call("maavss_vit_cls_attn", ptr(qkv), ptr(att), f, ntok, heads, 3 * d, dt, st)
        return att

    def check_finite(self, wait=True):
        """Raise if an attention_frames(..., finite_check="deferred") call produced a non-finite CLS attention.  wait=True waits for
        the flag copies of all such calls (not for the device); wait=False looks only at copies that have already arrived."""
        raised = False
        while self._flag_pending:
            event, host = self._flag_pending[0]
            if not wait and not event.query():
                break
            event.synchronize()
            self._flag_pending.pop(0)
            raised |= int(host.item()) != 0
        if raised:
            self._flag_pending.clear()
            self._flag.zero_()
            raise _lib.MaavssError(
                "VideoAttention: non-finite attention maps -- an activation of the ViT left the range of its 16-bit storage "
                f"format (act_dtype={self.act_dtype!r}" + (": IEEE half saturates at 65504; build the extractor with "
                "act_dtype='bf16', which has fp32's exponent range" if self.act_dtype == "f16" else "") +
                ") or the input frames / weights hold inf or NaN")

    def attention_frames(self, frames, clip_frames=0, out=None, attn_diff=False, finite_check="sync"):
        """Batched GPU path: frames [F,3,H,W] -> attention frames [F,1,H,W] (each /frame max; with
        clip_frames = T additionally /clip max over consecutive groups of T frames, av_dataset.py:328;
        attn_diff=True first replaces each clip's frames by their temporal difference, av_dataset.py:323-326).
        Frames are processed `frames_per_launch` at a time (bounds the activation scratch: ~9.6 MB per frame at
        224^2 for vit_small, ~13.6 MB for vit_base); measured on MI355X, fewer and larger launches win (512 frames/group: 75 ms/step vs 88 ms at 64).

        finite_check: the reference runs the ViT in fp32; here activations are stored in 16 bits and IEEE half (the default)
        overflows above 65504 -> inf -> NaN maps.  The maps kernel raises a sticky device flag when a CLS-attention value is
        not finite (every upstream overflow ends there).  "sync" (default): wait for this call and raise MaavssError now;
        "deferred": copy the flag to pinned host memory asynchronously and raise at a later call (once the copy has arrived)
        or at check_finite() -- no host-device synchronisation inside a training step (bench.py); None: no check."""
        _lib.require_cuda(frames)
        flag = self._finite_flag(finite_check)
        f, _, h, w = frames.shape
        if out is None:
            out = torch.empty(f, 1, h, w, device=frames.device, dtype=torch.float32)
        step = self.frames_per_launch
        if clip_frames:
            step = max(clip_frames, (step // clip_frames) * clip_frames)
        hp, wp = h // PATCH, w // PATCH
        for s in range(0, f, step):
            e = min(f, s + step)
            att = self.cls_attention(frames[s:e])
            ws = torch.empty((e - s) * (hp * wp + 1), device=frames.device, dtype=torch.float32)
            call("maavss_vit_attn_maps_checked", ptr(att), ptr(out[s:e]), ptr(ws), e - s, self.spec.heads, h, w, int(clip_frames),
                 int(bool(attn_diff)), ptr(flag), stream_ptr())
        self._finite_flag_read(flag, finite_check)
        return out

    # ---- the finite guard shared by attention_frames and attention_masks ---------------------------
    def _finite_flag(self, finite_check):
        """Before the launches of a guarded call: raise what earlier deferred calls found, -> the sticky device flag (None = no check)."""
        if finite_check not in ("sync", "deferred", None):
            raise ValueError("finite_check must be 'sync', 'deferred' or None")
        self.check_finite(wait=False)             # deferred flags of earlier calls that have arrived (never blocks)
        if finite_check is not None and self._flag is None:
            self._flag = torch.zeros(1, device=self.device, dtype=torch.int32)
            self._flag_hosts = [torch.zeros(1, dtype=torch.int32).pin_memory() for _ in range(8)]
        return self._flag if finite_check is not None else None

    def _finite_flag_read(self, flag, finite_check):
        """After the launches: copy the flag to pinned host memory behind them; "sync" waits for it and raises."""
        if flag is None:
            return
        if len(self._flag_pending) >= len(self._flag_hosts):
            self.check_finite()                   # the ring of pinned flag copies is full: wait for the oldest calls
        used = {id(h) for _, h in self._flag_pending}
        host = next(h for h in self._flag_hosts if id(h) not in used)
        host.copy_(flag, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        self._flag_pending.append((event, host))
        if finite_check == "sync":
            self.check_finite()

    def attention_masks(self, frames=None, *, att=None, threshold=None, upsample=True, dtype=torch.uint8, out=None,
                        finite_check="sync", frame_size=None):
        """DINO's per-head segmentation masks (video_attention.py:59-78): for every frame and head, the patches that hold the top
        `threshold` share of the CLS attention mass -- sorted ascending (ties by patch index), normalised, cumulated, kept where the
        cumulative share exceeds 1 - threshold, written back in patch order -- as 0 / 1 values of `dtype` (torch.uint8, or torch.float32
        = the reference's .float() at :68).  -> [F, heads, H, W] (each patch repeated 8 x 8, nearest as at :70-75; zero outside the patch
        grid, as in attention_frames), or [F, heads, H//8, W//8] with upsample=False.

        Exactly one of `frames` ([F,3,H,W] f32 cuda; processed `frames_per_launch` at a time like attention_frames) and `att` (a tensor
        cls_attention returned, [F, heads, n] f32 cuda: a caller who also wants attention_frames runs the ViT once).  With `att` pass
        frame_size=(H, W); without it only upsample=False is possible and the masks come back flat, [F, heads, n], like `att`.
        threshold=None: the constructor's.  finite_check: as in attention_frames (a non-finite CLS attention value raises MaavssError;
        the masks of such a row are unspecified)."""
        threshold = self.threshold if threshold is None else threshold
        if not 0.0 <= float(threshold) <= 1.0:                                                # NaN fails both comparisons
            raise ValueError(f"threshold={threshold!r}: the kept share of the attention mass must lie in [0, 1]")
        if (frames is None) == (att is None):
            raise ValueError("attention_masks takes exactly one of `frames` and `att`")
        if dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"dtype={dtype!r}: masks are written as torch.uint8 or torch.float32")
        if finite_check not in ("sync", "deferred", None):
            raise ValueError("finite_check must be 'sync', 'deferred' or None")
        _lib.require_cuda(frames, att, out)
        if frames is not None:
            if frames.dim() != 4 or frames.shape[1] != 3 or frames.dtype != torch.float32:
                raise ValueError(f"frames must be [F, 3, H, W] float32, got {tuple(frames.shape)} {frames.dtype}")
            if frame_size is not None and tuple(frame_size) != tuple(frames.shape[2:]):
                raise ValueError(f"frame_size={tuple(frame_size)} contradicts frames of {tuple(frames.shape[2:])}")
            f, heads, (h, w) = frames.shape[0], self.spec.heads, frames.shape[2:]
        else:
            if att.dim() != 3 or att.dtype != torch.float32:
                raise ValueError(f"att must be the [F, heads, n] float32 tensor of cls_attention, got {tuple(att.shape)} {att.dtype}")
            att = att.contiguous()
            f, heads, n = att.shape
            if frame_size is None:
                if upsample:
                    raise ValueError("attention_masks(att=...) needs frame_size=(H, W) to upsample (or upsample=False)")
                h, w = PATCH, PATCH * n               # one row of n patches: the flat layout of `att`
            else:
                h, w = (int(v) for v in frame_size)
                if (h // PATCH) * (w // PATCH) != n:
                    raise ValueError(f"frame_size={(h, w)} has {(h // PATCH) * (w // PATCH)} patches, att has {n}")
        if upsample:
            shape = (f, heads, h, w)
        else:
            shape = (f, heads, n) if frames is None and frame_size is None else (f, heads, h // PATCH, w // PATCH)
        if out is None:
            out = torch.empty(shape, device=self.device if frames is None else frames.device, dtype=dtype)
        elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {dtype} tensor of shape {shape}, got {tuple(out.shape)} {out.dtype}")
        if f == 0:
            return out
        flag = self._finite_flag(finite_check)
        code, up = (1 if dtype == torch.float32 else 0), int(bool(upsample))
        if frames is None:
            call("maavss_vit_attn_masks", ptr(att), ptr(out), code, f, heads, h, w, PATCH, up, float(threshold), ptr(flag), stream_ptr())
        else:
            for s in range(0, f, self.frames_per_launch):
                e = min(f, s + self.frames_per_launch)
                a = self.cls_attention(frames[s:e])
                call("maavss_vit_attn_masks", ptr(a), ptr(out[s:e]), code, e - s, heads, h, w, PATCH, up, float(threshold), ptr(flag),
                     stream_ptr())
        self._finite_flag_read(flag, finite_check)
        return out

    def _inference(self, frames):
        """Reference contract (video_attention.py:38-103): [T,3,H,W] float -> [T,1,H,W] float32 on the CPU."""
        # `resize` is stored and never read by the reference's _inference (video_attention.py:29-30,38-103): same here.
        # Frame sizes that are not multiples of 8: the reference crops to the patch grid and then fails on the shape
        # mismatch of its assignment at :96; here the area outside the patch grid stays zero (documented extension).
        dev_frames = frames.to(self.device, dtype=torch.float32)
        return self.attention_frames(dev_frames, clip_frames=0).cpu()
