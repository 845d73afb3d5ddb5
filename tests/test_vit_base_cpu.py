"""VideoAttention(architecture="vit_base") on the host: the CPU fp32 twin it is graded against (tests/dino_twin.py) and the
constructor / checkpoint rules.  No kernel runs here."""
import numpy as np
import pytest
import torch

import dino_twin as tw
from maavss_amd.video_attention import (DIM, HEADS, MLP, VIT_SPECS, DinoViTWeights, VideoAttention, ViTSmall8Weights,
                                        interpolate_pos_embed, vit_shapes, vit_small_shapes)
from oracle import vit_ref_cpu as vref

KW = dict(path_to_weights="/nonexistent/weights.pth", device="cpu")


def test_twin_in_the_small_configuration_is_the_oracle():
    sd = tw.seeded_state(tw.S8, 3)
    osd = vref.seeded_vit_state(3)
    assert set(sd) == set(osd) and all(torch.equal(sd[k], osd[k]) for k in osd)
    for width, n in ((64, 3), (96, 1)):                      # 96^2: the 224^2 position table interpolated
        fr = vref.synthetic_frames(n, width, 5)
        with torch.no_grad():
            got, want = tw.cls_attention(tw.S8, sd, fr), vref.cls_attention(osd, fr)
        assert (got - want).abs().max().item() < 1e-6


def test_twin_in_the_base_configuration_matches_transformers_vit():
    """Independent cross-check of the B configuration against transformers.ViTModel built from a local config at 224^2
    (tests/test_oracle_cpu.py test_vit_oracle_vs_hf_vit is the same check of the S oracle)."""
    tr = pytest.importorskip("transformers")
    cfg = tw.B8
    hf_cfg = tr.ViTConfig(hidden_size=cfg.dim, num_hidden_layers=cfg.depth, num_attention_heads=cfg.heads, intermediate_size=cfg.mlp,
                          image_size=224, patch_size=8, layer_norm_eps=1e-6, hidden_act="gelu", qkv_bias=True,
                          attn_implementation="eager")
    hf = tr.ViTModel(hf_cfg, add_pooling_layer=False).eval()
    sd = tw.seeded_state(cfg, 3)
    d = cfg.dim
    m = {"embeddings.cls_token": sd["cls_token"], "embeddings.position_embeddings": sd["pos_embed"],
         "embeddings.patch_embeddings.projection.weight": sd["patch_embed.proj.weight"],
         "embeddings.patch_embeddings.projection.bias": sd["patch_embed.proj.bias"],
         "layernorm.weight": sd["norm.weight"], "layernorm.bias": sd["norm.bias"]}
    new_names = any(k.startswith("layers.0.attention.q_proj") for k in hf.state_dict())   # transformers >= 5
    for i in range(cfg.depth):
        p = f"blocks.{i}."
        qw, qb = sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]
        if new_names:
            h = f"layers.{i}."
            qkv_names = [h + "attention.q_proj", h + "attention.k_proj", h + "attention.v_proj"]
            o, f1, f2 = h + "attention.o_proj", h + "mlp.fc1", h + "mlp.fc2"
        else:
            h = f"encoder.layer.{i}."
            qkv_names = [h + f"attention.attention.{nm}" for nm in ("query", "key", "value")]
            o, f1, f2 = h + "attention.output.dense", h + "intermediate.dense", h + "output.dense"
        for j, nm in enumerate(qkv_names):
            m[nm + ".weight"] = qw[d * j:d * (j + 1)]
            m[nm + ".bias"] = qb[d * j:d * (j + 1)]
        m[o + ".weight"], m[o + ".bias"] = sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"]
        m[h + "layernorm_before.weight"], m[h + "layernorm_before.bias"] = sd[p + "norm1.weight"], sd[p + "norm1.bias"]
        m[h + "layernorm_after.weight"], m[h + "layernorm_after.bias"] = sd[p + "norm2.weight"], sd[p + "norm2.bias"]
        m[f1 + ".weight"], m[f1 + ".bias"] = sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]
        m[f2 + ".weight"], m[f2 + ".bias"] = sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"]
    missing = hf.load_state_dict(m, strict=False)
    assert not missing.unexpected_keys and not missing.missing_keys, missing
    frames = vref.synthetic_frames(1, 224, 11)
    with torch.no_grad():
        ours, _, amax = tw.forward(cfg, sd, frames, return_hidden=True)
        theirs = hf(pixel_values=frames, output_attentions=True).attentions[-1]
    assert theirs.shape == (1, 12, 785, 785)
    np.testing.assert_allclose(ours[:, :, 0, 1:].numpy(), theirs[:, :, 0, 1:].numpy(), rtol=2e-3, atol=2e-6)
    # the seeded recipe keeps every activation far inside IEEE half's range (the GPU tests run the f16 extractor on it)
    assert amax < 100, amax
    # and its maps are not flat: the CLS row is peaked
    assert ours[:, :, 0, 1:].max().item() > 20 / 784


def test_vit_base_builds_without_touching_the_device(capsys):
    va = VideoAttention(architecture="vit_base", device="cuda", **{k: v for k, v in KW.items() if k != "device"})
    assert va.spec == VIT_SPECS["vit_base"] and (va.spec.dim, va.spec.heads, va.spec.mlp, va.spec.depth) == (768, 12, 3072, 12)
    assert va._dev is None and va._flag is None                        # device images and the range flag are built lazily
    assert isinstance(va.model, DinoViTWeights) and va.model.architecture == "vit_base"
    assert {k: tuple(v.shape) for k, v in va.model.state_dict().items()} == vit_shapes("vit_base")
    assert va.model.loaded_from is None and "not found" in capsys.readouterr().err
    assert VideoAttention(architecture="vit_base", act_dtype="bf16", **KW).act_dtype == "bf16"


def test_small_backbone_names_are_unchanged():
    assert (DIM, HEADS, MLP) == (384, 6, 1536) and vit_small_shapes() == vit_shapes("vit_small")
    a, b = ViTSmall8Weights(seed=4), DinoViTWeights("vit_small", seed=4)
    assert all(torch.equal(a.sd[k], b.sd[k]) for k in a.sd)
    va = VideoAttention(**KW)
    assert va.architecture == "vit_small" and isinstance(va.model, ViTSmall8Weights)


@pytest.mark.parametrize("bad,why", [(dict(attn_dtype="fp8"), "vit_small only"), (dict(attn_dtype="fp8-late"), "vit_small only"),
                                     (dict(attn_dtype="fp8", fp8_blocks=(9, 10)), "vit_small only"), (dict(fp8_blocks=()), "fp8_blocks"),
                                     (dict(gelu="half"), "gelu"), (dict(qkv_ln="post"), "qkv_ln"), (dict(patch_size=16), "patch")])
def test_vit_base_rejects_the_small_only_modes(bad, why):
    with pytest.raises(ValueError, match=why):
        VideoAttention(architecture="vit_base", **KW, **bad)


def test_vit_base_ignores_the_qkv_ln_environment_default(monkeypatch):
    monkeypatch.setenv("MAAVSS_QKV_LN", "post")
    assert VideoAttention(**KW).qkv_ln == "post"                         # vit_small: unchanged
    assert VideoAttention(architecture="vit_base", **KW).qkv_ln == "pre"


def test_unbuilt_architectures_say_why():
    with pytest.raises(ValueError, match="no vit_tiny checkpoint"):
        VideoAttention(architecture="vit_tiny", **KW)
    with pytest.raises(ValueError, match="vit_base"):
        VideoAttention(architecture="vit_large", **KW)
    with pytest.raises(ValueError, match="patch"):
        VideoAttention(patch_size=16, **KW)


def _dino_checkpoint(path, cfg, img_size=224, seed=3):
    sd = tw.seeded_state(cfg, seed, img_size)
    teacher = {"module.backbone." + k: v for k, v in sd.items()}
    teacher["module.head.mlp.0.weight"] = torch.zeros(4, 4)
    torch.save({"student": {}, "teacher": teacher, "epoch": 1}, path)
    return sd


def test_vit_base_loads_a_dino_checkpoint(tmp_path):
    path = str(tmp_path / "dino_vitbase8_pretrain.pth")
    sd = _dino_checkpoint(path, tw.B8)
    va = VideoAttention(architecture="vit_base", path_to_weights=path, device="cpu")
    assert va.model.loaded_from == path
    got = va.model.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], v) for k, v in sd.items())
    # a bare state dict with the "backbone." prefix loads too
    bare = str(tmp_path / "bare.pth")
    torch.save({"backbone." + k: v for k, v in sd.items()}, bare)
    assert torch.equal(VideoAttention(architecture="vit_base", path_to_weights=bare, device="cpu").model.sd["pos_embed"], sd["pos_embed"])


def test_wrong_width_checkpoint_names_the_architecture_and_its_file(tmp_path):
    path = str(tmp_path / "dino_deitsmall8_pretrain.pth")                # the reference's default path, a ViT-S/8 checkpoint
    _dino_checkpoint(path, tw.S8)
    with pytest.raises(RuntimeError, match=r"'vit_base'.*dino_vitbase8_pretrain\.pth"):
        VideoAttention(architecture="vit_base", path_to_weights=path, device="cpu")
    with pytest.raises(RuntimeError, match=r"'vit_small'.*dino_deitsmall8_pretrain\.pth"):
        VideoAttention(**KW).load_state_dict(tw.seeded_state(tw.B8, 1))
    # a position table of the wrong width alone is refused as well (its token count may differ: it is interpolated)
    va = VideoAttention(architecture="vit_base", **KW)
    sd = tw.seeded_state(tw.B8, 2)
    sd["pos_embed"] = torch.zeros(1, 785, 384)
    with pytest.raises(RuntimeError, match="pos_embed"):
        va.load_state_dict(sd)
    sd["pos_embed"] = torch.zeros(1, 2305, 768)                          # a 384^2 table of the right width is fine
    va.load_state_dict(sd)


@pytest.mark.parametrize("side", [32, 48])                              # 256^2 and 384^2 frames through the 224^2 table
def test_position_table_interpolation_takes_its_width_from_the_tensor(side):
    pe = tw.seeded_state(tw.B8, 3)["pos_embed"]
    got = interpolate_pos_embed(pe, side, side)
    assert tuple(got.shape) == (1, side * side + 1, 768)
    assert torch.equal(got, tw.interpolate_pos_embed(pe, side, side)) and torch.equal(got[:, 0], pe[:, 0])
