"""Attention masks (VideoAttention.attention_masks / maavss_vit_attn_masks), the part that needs no GPU: the float64 twin
(tests/mask_twin.py) against a literal restatement of the reference's video_attention.py:59-66, its handling of ties, zero rows and
the ends of the threshold range, the cap on undecided elements for every synthetic input the GPU tests use, and the host-side
argument checks of the method and of the entry point (which come before any device work)."""
import pytest
import torch

import mask_twin as mt


def reference_lines_59_66(att, threshold):
    """video_attention.py:59-66 as written (non-stable sort, argsort, per-head un-permute loop), evaluated in float64."""
    attentions = att.double().clone()
    nh = attentions.shape[0]
    val, idx = torch.sort(attentions)
    val /= torch.sum(val, dim=1, keepdim=True)
    cumval = torch.cumsum(val, dim=1)
    th_attn = cumval > (1 - threshold)
    idx2 = torch.argsort(idx)
    for head in range(nh):
        th_attn[head] = th_attn[head][idx2[head]]
    return th_attn


@pytest.mark.parametrize("n", [1, 2, 63, 784, 2304])
@pytest.mark.parametrize("threshold", [0.1, 0.6, 0.9])
def test_twin_equals_the_reference_lines_on_tie_free_rows(n, threshold):
    g = torch.Generator().manual_seed(n)
    att = torch.softmax(2.0 * torch.randn(6, n, generator=g, dtype=torch.float64), -1).float()
    assert all(att[h].unique().numel() == n for h in range(6)), "the rows must be tie-free for the non-stable sort"
    mask, _ = mt.masks_twin(att, threshold)
    assert torch.equal(mask, reference_lines_59_66(att, threshold))


def test_twin_ties_go_by_patch_index():
    # eight equal values, total 8: c = 1/8 .. 8/8 in sorted order = patch order.  threshold 0.5: kept <=> c > 0.5 <=> the last four
    # patches BY INDEX; the margin 8 * 2^-23 leaves c = 0.5 itself (patch 3) undecided and nothing else
    att = torch.ones(1, 8)
    mask, und = mt.masks_twin(att, 0.5)
    assert mask.tolist() == [[False] * 4 + [True] * 4]
    assert und.tolist() == [[False, False, False, True, False, False, False, False]]
    # values 1 1 2 2 2 (total 8): sorted order = patches 0 1 | 2 3 4, c = 1/8 2/8 4/8 6/8 8/8; threshold 0.7 -> cut 0.3: the three 2s;
    # threshold 0.3 -> cut 0.7: patches 3 and 4, the LATER two of the tied 2s
    att = torch.tensor([[1.0, 1.0, 2.0, 2.0, 2.0]])
    assert mt.masks_twin(att, 0.7)[0].tolist() == [[False, False, True, True, True]]
    assert mt.masks_twin(att, 0.3)[0].tolist() == [[False, False, False, True, True]]
    # the same values in another patch order: the flags follow the patches
    att = torch.tensor([[2.0, 1.0, 2.0, 1.0, 2.0]])
    assert mt.masks_twin(att, 0.3)[0].tolist() == [[False, False, True, False, True]]


def test_twin_zero_rows_and_the_ends_of_the_threshold_range():
    att = torch.tensor([[0.0, 0.0, 0.0, 0.0], [0.1, 0.2, 0.3, 0.4], [0.0, 0.5, 0.0, 0.5]])
    for thr in (0.0, 0.6, 1.0):
        mask, und = mt.masks_twin(att, thr)
        assert not mask[0].any() and not und[0].any(), "a zero row keeps nothing and is decided (NaN > x is False)"
    mask, und = mt.masks_twin(att, 0.0)                   # c > 1 never holds; c = 1 (the last sorted element) is undecided
    assert not mask.any() and und[1].tolist() == [False, False, False, True]
    mask, und = mt.masks_twin(att, 1.0)                   # c > 0: every patch behind the zeros; c = 0 is undecided
    assert mask[1].all() and not und[1].any()
    assert mask[2].tolist() == [False, True, False, True] and und[2].tolist() == [True, False, True, False]


@pytest.mark.parametrize("grid", mt.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("heads", mt.HEADS)
def test_synthetic_inputs_respect_the_cap_on_undecided_elements(grid, heads):
    """The precondition of the kernel-against-twin test on the GPU, proved on the same rows (same generator, same seeds)."""
    n = grid[0] * grid[1]
    for thr in mt.THRESHOLDS:
        att = mt.synthetic_att(*grid, heads, thr)
        assert att.shape == (mt.FRAMES_PER_SCALE * len(mt.scales_for(thr)), heads, n) and (att > 0).all()
        _, und = mt.masks_twin(att, thr)
        worst = int(und.sum(-1).max())
        print(f"[masks] grid {grid} heads {heads} threshold {thr}: at most {worst} undecided per row (cap {mt.cap(n)})")
        assert worst <= mt.cap(n), (grid, heads, thr, worst)


def test_exact_tie_rows_are_exact_in_f32():
    """The rows of the GPU test `exact ties`: power-of-two totals, and an f32 evaluation of the contract (any summation order is exact
    on them) gives the twin's mask on EVERY element, the ones the margin calls undecided included."""
    for n in (784, 1024, 2304, 4096, 880):
        att = mt.exact_tie_rows(n)
        tot = att.double().sum(-1)
        assert (torch.log2(tot) % 1 == 0).all() and (att == att.round()).all() and (att >= 0).all()
        assert min(att[r, h].unique().numel() for r in range(att.shape[0]) for h in range(att.shape[1])) <= 9, "few distinct values: ties"
        for thr in mt.EXACT_THRESHOLDS:
            val, idx = torch.sort(att, dim=-1, stable=True)
            c32 = torch.cumsum(val / val.sum(-1, keepdim=True), -1)
            assert c32.dtype == torch.float32
            m32 = torch.zeros_like(c32, dtype=torch.bool).scatter(-1, idx, c32 > torch.tensor(1.0 - thr, dtype=torch.float32))
            assert torch.equal(m32, mt.masks_twin(att, thr)[0])


# ---- host-side argument checks ------------------------------------------------------------------------------------------------------

def _extractor():
    import maavss_amd
    return maavss_amd.VideoAttention(path_to_weights="/nonexistent.pth", threshold=0.6)


def test_attention_masks_validates_its_arguments_on_the_host():
    from maavss_amd._lib import MaavssError
    va = _extractor()
    frames, att = torch.zeros(2, 3, 16, 16), torch.full((2, 6, 4), 0.25)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            va.attention_masks(frames, threshold=bad)
    with pytest.raises(ValueError, match="threshold"):
        type(va)(path_to_weights="/nonexistent.pth", threshold=2.0).attention_masks(frames)       # the constructor's, at last read
    with pytest.raises(ValueError, match="exactly one"):
        va.attention_masks()
    with pytest.raises(ValueError, match="exactly one"):
        va.attention_masks(frames, att=att)
    for bad in (torch.float16, torch.bool, torch.int32):
        with pytest.raises(ValueError, match="dtype"):
            va.attention_masks(frames, dtype=bad)
    with pytest.raises(ValueError, match="finite_check"):
        va.attention_masks(frames, finite_check="later")
    with pytest.raises(MaavssError, match="CPU tensor"):
        va.attention_masks(frames)
    with pytest.raises(MaavssError, match="CPU tensor"):
        va.attention_masks(att=att, frame_size=(16, 16))
    with pytest.raises(MaavssError, match="CPU tensor"):
        va.attention_masks(att=att, upsample=False)


def test_entry_point_is_exported_and_validates_before_touching_the_device():
    from maavss_amd import _lib
    L = _lib.lib()
    assert "maavss_vit_attn_masks" in L.protos and len(L.protos["maavss_vit_attn_masks"][1]) == 12
    assert _lib.header_abi_version() == 402 and L.cdll.maavss_version() == 402, "the entry point was additive in 400; 401 removed the convt2d, 402 the conv2d entry points"
    good = dict(att=256, out=512, out_dtype=0, n_frames=2, heads=6, H=224, W=224, patch=8, upsample=1, threshold=0.6, flag=None, stream=None)

    def call(**kw):
        _lib.call("maavss_vit_attn_masks", *{**good, **kw}.values())

    for kw, msg in [(dict(att=None), "null pointer"), (dict(out=None), "null pointer"), (dict(heads=0), "heads"), (dict(patch=0), "patch"),
                    (dict(H=7), "n < 1"), (dict(W=4), "n < 1"), (dict(H=520, W=512), "at most 4096"), (dict(threshold=-0.01), "threshold"),
                    (dict(threshold=1.01), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(out_dtype=2), "out_dtype"),
                    (dict(out_dtype=-1), "out_dtype"), (dict(n_frames=0), "n_frames")]:
        with pytest.raises(_lib.MaavssError, match=msg):
            call(**kw)
