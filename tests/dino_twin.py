"""TEST INFRASTRUCTURE ONLY -- a CPU fp32 twin of DINO's VisionTransformer, generic over its configuration.

oracle/vit_ref_cpu.py restates the ViT-S/8 alone (module constants dim 384, 6 heads).  This twin takes the configuration as data
so that the ViT-B/8 backbone (VideoAttention(architecture="vit_base"): dim 768, 12 heads, MLP 3072) has an fp32 reference to be
graded against.  Same published architecture: pre-LN blocks, LayerNorm eps 1e-6, qkv bias, exact-erf GELU, Conv2d patch embedding,
CLS token, learned position embedding bicubic-resized (DINO's +0.1 rule) for frames other than the table's; DINO state-dict keys.
It is checked against the oracle in the S configuration and against transformers.ViTModel in the B configuration
(tests/test_vit_base_cpu.py).

seeded_state: the oracle's recipe (oracle/vit_ref_cpu.seeded_vit_state) with every scale taken from the configuration, so that the
S configuration reproduces the oracle's state bit for bit.  attn.qkv is drawn at 1.6 / sqrt(dim): logits sharper than DINO's init,
so the CLS attention maps are not flat.  Largest |activation| of the B configuration with seed 3 on oracle synthetic_frames (seed 5):
22.4 at 224^2, 20.0 at 64^2 and 384^2, reached by the residual stream (the LayerNorm outputs, qkv and the MLP hidden stay below it)
-- inside IEEE half's range (65504) by more than three orders of magnitude; tests/test_vit_base_cpu.py pins it below 100.
"""
import math
import zlib
from typing import NamedTuple

import torch
import torch.nn.functional as F

LN_EPS = 1e-6


class Config(NamedTuple):
    dim: int
    heads: int
    mlp: int
    depth: int = 12
    patch: int = 8


S8 = Config(384, 6, 1536)
B8 = Config(768, 12, 3072)


def param_shapes(cfg, img_size=224):
    d, p = cfg.dim, cfg.patch
    n = (img_size // p) ** 2
    sh = {"cls_token": (1, 1, d), "pos_embed": (1, n + 1, d),
          "patch_embed.proj.weight": (d, 3, p, p), "patch_embed.proj.bias": (d,),
          "norm.weight": (d,), "norm.bias": (d,)}
    for i in range(cfg.depth):
        b = f"blocks.{i}."
        sh.update({b + "norm1.weight": (d,), b + "norm1.bias": (d,),
                   b + "attn.qkv.weight": (3 * d, d), b + "attn.qkv.bias": (3 * d,),
                   b + "attn.proj.weight": (d, d), b + "attn.proj.bias": (d,),
                   b + "norm2.weight": (d,), b + "norm2.bias": (d,),
                   b + "mlp.fc1.weight": (cfg.mlp, d), b + "mlp.fc1.bias": (cfg.mlp,),
                   b + "mlp.fc2.weight": (d, cfg.mlp), b + "mlp.fc2.bias": (d,)})
    return sh


def seeded_state(cfg, seed, img_size=224):
    out = {}
    for k, shape in param_shapes(cfg, img_size).items():
        g = torch.Generator(device="cpu")
        g.manual_seed((zlib.crc32(k.encode()) ^ (seed * 2654435761)) & 0x7FFFFFFF)
        r = torch.randn(shape, generator=g)
        if k.endswith("norm1.weight") or k.endswith("norm2.weight") or k == "norm.weight":
            t = 1.0 + 0.1 * r
        elif k.endswith(".bias"):
            t = 0.05 * r
        elif k in ("cls_token", "pos_embed"):
            t = 0.2 * r
        elif k == "patch_embed.proj.weight":
            t = r * (1.0 / math.sqrt(3 * cfg.patch * cfg.patch))
        elif "attn.qkv.weight" in k:
            t = r * (1.6 / math.sqrt(cfg.dim))          # sharper-than-init logits so softmax is not flat
        else:
            t = r * (1.0 / math.sqrt(shape[1]))
        out[k] = t.float()
    return out


def interpolate_pos_embed(pos_embed, h_tok, w_tok):
    n, d = pos_embed.shape[1] - 1, pos_embed.shape[2]
    if n == h_tok * w_tok and h_tok == w_tok:
        return pos_embed
    side = int(math.sqrt(n))
    patch = pos_embed[:, 1:].reshape(1, side, side, d).permute(0, 3, 1, 2)
    patch = F.interpolate(patch, scale_factor=((h_tok + 0.1) / side, (w_tok + 0.1) / side), mode="bicubic")
    patch = patch.permute(0, 2, 3, 1).reshape(1, -1, d)
    return torch.cat([pos_embed[:, :1], patch], 1)


def forward(cfg, sd, frames, return_hidden=False):
    """frames [B,3,H,W] -> the last block's self-attention [B, heads, n+1, n+1] (get_last_selfattention); with return_hidden also
    the inputs of the blocks and the largest |value| of the LayerNorm outputs, qkv, residual stream and mlp.fc1 pre-activation
    (this bounds the attention output, a convex combination of v, and the GELU output too)."""
    b, _, h, w = frames.shape
    d, hd = cfg.dim, cfg.dim // cfg.heads
    x = F.conv2d(frames, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=cfg.patch).flatten(2).transpose(1, 2)
    x = torch.cat([sd["cls_token"].expand(b, -1, -1), x], 1)
    x = x + interpolate_pos_embed(sd["pos_embed"], h // cfg.patch, w // cfg.patch)
    n = x.shape[1]
    hidden, amax = [x], x.abs().max().item()
    for i in range(cfg.depth):
        p = f"blocks.{i}."
        y = F.layer_norm(x, (d,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], LN_EPS)
        qkv = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
        amax = max(amax, y.abs().max().item(), qkv.abs().max().item())
        q, k, v = qkv.reshape(b, n, 3, cfg.heads, hd).permute(2, 0, 3, 1, 4)
        att = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(-1)
        if i == cfg.depth - 1:
            return (att, hidden, amax) if return_hidden else att
        y = (att @ v).transpose(1, 2).reshape(b, n, d)
        x = x + F.linear(y, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
        y = F.layer_norm(x, (d,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], LN_EPS)
        hpre = F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])
        hact = F.gelu(hpre)
        x = x + F.linear(hact, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
        amax = max(amax, y.abs().max().item(), hpre.abs().max().item(), x.abs().max().item())
        hidden.append(x)


def cls_attention(cfg, sd, frames):
    """[B,3,H,W] -> CLS-row attention without the CLS column, [B, heads, n]."""
    return forward(cfg, sd, frames)[:, :, 0, 1:]


def attention_frames(cfg, sd, frames, clip_frames=0):
    """video_attention.py:80-96 (+ av_dataset.py:328 with clip_frames): [F,3,H,W] -> [F,1,H,W], H and W multiples of the patch."""
    f, _, h, w = frames.shape
    hp, wp = h // cfg.patch, w // cfg.patch
    a = cls_attention(cfg, sd, frames).reshape(f, cfg.heads, hp, wp)
    a = F.interpolate(a, scale_factor=cfg.patch, mode="nearest").sum(1)
    a = a * (1.0 / a.flatten(1).max(1).values)[:, None, None]
    a = a[:, None]
    if clip_frames:
        a = a.view(f // clip_frames, clip_frames, 1, h, w)
        a = a * (1.0 / a.flatten(1).max(1).values)[:, None, None, None, None]
        a = a.view(f, 1, h, w)
    return a
