"""Attention masks on the MI355X: maavss_vit_attn_masks against the float64 twin of its contract (tests/mask_twin.py: every decided
element bit for bit, the inputs proved to respect the cap on undecided ones by tests/test_attn_masks_cpu.py), the rounding-free order
property, exact ties, the output layouts, the finite guard, VideoAttention.attention_masks end to end on both backbones, and how far
the 16-bit extractor moves the masks of the fp32 twin ViT (tests/dino_twin.py)."""
import pytest
import torch

import dino_twin as tw
import mask_twin as mt

pytestmark = pytest.mark.gpu

DTYPES = [torch.uint8, torch.float32]


def _masks(att, h, w, threshold, dtype, upsample, flag=None, patch=mt.PATCH):
    """The raw entry point on att [F, heads, n] (cuda) into a buffer with a sentinel tail, which must come back untouched."""
    from maavss_amd import _lib
    f, heads, _ = att.shape
    shape = (f, heads, h, w) if upsample else (f, heads, h // patch, w // patch)
    numel = f * heads * shape[2] * shape[3]
    buf = torch.full((numel + 64,), 7, dtype=dtype, device="cuda")
    _lib.call("maavss_vit_attn_masks", att.data_ptr(), buf.data_ptr(), int(dtype == torch.float32), f, heads, h, w, patch, int(upsample),
              threshold, None if flag is None else flag.data_ptr(), _lib.stream_ptr())
    assert (buf[numel:] == 7).all(), "the kernel wrote past the end of its output"
    return buf[:numel].view(shape)


@pytest.mark.parametrize("heads", mt.HEADS)
@pytest.mark.parametrize("grid", mt.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_kernel_matches_the_float64_twin(grid, heads):
    """Every threshold, both dtypes, both layouts on the shared synthetic rows softmax(s * randn): decided elements equal the twin bit for
    bit, a row leaves out at most max(2, n / 256) undecided ones (a condition on the inputs, proved on the CPU)."""
    hp, wp = grid
    h, w = hp * mt.PATCH, wp * mt.PATCH
    for thr in mt.THRESHOLDS:
        att = mt.synthetic_att(hp, wp, heads, thr)
        ac = att.cuda()
        for dtype in DTYPES:
            small = _masks(ac, h, w, thr, dtype, False)
            assert small.dtype == dtype and small.shape == (att.shape[0], heads, hp, wp)
            moved = mt.assert_masks_match(small.cpu().flatten(2), att, thr, f"grid {grid} heads {heads} threshold {thr} {dtype}")
            print(f"[masks] grid {grid} heads {heads} threshold {thr} {dtype}: {moved} undecided elements differ from the twin")
            big = _masks(ac, h, w, thr, dtype, True)
            assert torch.equal(big.cpu(), mt.upsample_ref(small.cpu(), hp, wp, h, w)), "upsampled != patch-resolution repeated 8 x 8"
    # the ends of the range by reasoning instead of by margin, on peaked rows too (softmax scale 3, strictly positive values): with
    # threshold = 1 every c is positive in any arithmetic -> everything is kept; with threshold = 0 only a c rounded above 1 can be kept,
    # which the sorted order allows for the largest values alone
    peaked = mt.synthetic_att(hp, wp, heads, 0.5)
    assert _masks(peaked.cuda(), h, w, 1.0, torch.uint8, False).all()
    assert _masks(peaked.cuda(), h, w, 0.0, torch.uint8, False).flatten(2).sum(-1).max().item() <= mt.cap(hp * wp)


@pytest.mark.parametrize("grid", [(28, 28), (48, 48), (22, 40), (64, 64)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_order_property_is_exact(grid):
    """Independent of rounding: in every row min(kept values) >= max(dropped values) -- the kept set is a suffix of the sorted order --,
    the kept patches hold at least `threshold` of the mass and no longer do without the smallest of them (both within n * 2^-23)."""
    hp, wp = grid
    n = hp * wp
    for thr in (0.1, 0.6, 0.9):
        att = mt.synthetic_att(hp, wp, 12, thr, seed=1)
        m = _masks(att.cuda(), hp * 8, wp * 8, thr, torch.uint8, False).cpu().flatten(2).bool()
        a = att.double()
        inf = torch.tensor(float("inf"), dtype=torch.float64)
        kept_min, drop_max = torch.where(m, a, inf).min(-1).values, torch.where(~m, a, -inf).max(-1).values
        assert (kept_min >= drop_max).all(), f"threshold {thr}: a dropped patch outweighs a kept one"
        assert m.any(-1).all()
        share = (a * m).sum(-1) / a.sum(-1)
        assert (share >= thr - mt.margin(n)).all(), f"threshold {thr}: kept mass {share.min().item()}"
        assert (share - kept_min / a.sum(-1) <= thr + mt.margin(n)).all(), f"threshold {thr}: a kept patch is superfluous"


@pytest.mark.parametrize("n_grid", [(28, 28), (32, 32), (48, 48), (64, 64), (22, 40)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_exact_ties_follow_the_patch_index(n_grid):
    """Rows of small integers with a power-of-two total: value / total and every partial sum are exact in f32, so the mask equals the
    twin on EVERY element; the many exact ties (eight distinct values over up to 4096 patches) pin torch.sort(stable=True)'s rule."""
    hp, wp = n_grid
    att = mt.exact_tie_rows(hp * wp)
    for thr in mt.EXACT_THRESHOLDS:
        want = mt.masks_twin(att, thr)[0]
        for dtype in DTYPES:
            got = _masks(att.cuda(), hp * 8, wp * 8, thr, dtype, False).cpu().flatten(2)
            assert torch.equal(got != 0, want), f"threshold {thr} {dtype}: {(want != (got != 0)).sum().item()} elements differ"
    zero = torch.zeros(1, 6, hp * wp)
    zero[0, 1] = att[0, 1]
    got = _masks(zero.cuda(), hp * 8, wp * 8, 0.5, torch.uint8, False).cpu().flatten(2)
    assert not got[0, [0, 2, 3, 4, 5]].any() and torch.equal(got[0, 1] != 0, mt.masks_twin(att[0, 1], 0.5)[0]), "zero rows keep nothing"


@pytest.mark.parametrize("h,w", [(230, 236), (229, 240), (64, 72), (12, 20)])
def test_layout_outside_the_patch_grid_is_zero(h, w):
    """H, W not multiples of 8 (the 16-byte and the element store paths of both dtypes): zeros outside the patch grid."""
    hp, wp = h // 8, w // 8
    att = torch.softmax(torch.randn(3, 6, hp * wp, generator=torch.Generator().manual_seed(h)), -1)
    for dtype in DTYPES:
        small = _masks(att.cuda(), h, w, 0.6, dtype, False).cpu()
        mt.assert_masks_match(small.flatten(2), att, 0.6, f"{h}x{w} {dtype}")
        big = _masks(att.cuda(), h, w, 0.6, dtype, True).cpu()
        assert torch.equal(big, mt.upsample_ref(small, hp, wp, h, w))
        assert not big[..., hp * 8:, :].any() and not big[..., wp * 8:].any() and big.any()


def _extractor(arch="vit_small", act="f16", seed=3, **kw):
    import maavss_amd
    va = maavss_amd.VideoAttention(architecture=arch, path_to_weights="/nonexistent.pth", act_dtype=act, **kw)
    va.load_state_dict(tw.seeded_state(tw.S8 if arch == "vit_small" else tw.B8, seed))
    return va


def test_method_out_streams_and_repeatability():
    va = _extractor()
    att = mt.synthetic_att(28, 28, 6, 0.6).cuda()
    first = va.attention_masks(att=att, frame_size=(224, 224))
    assert first.shape == (att.shape[0], 6, 224, 224) and first.dtype == torch.uint8
    assert torch.equal(first, va.attention_masks(att=att, frame_size=(224, 224))), "two calls differ"
    out = torch.full_like(first, 9)
    assert va.attention_masks(att=att, frame_size=(224, 224), out=out) is out and torch.equal(out, first), "out= is filled in place"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = va.attention_masks(att=att, frame_size=(224, 224))
    side.synchronize()
    assert torch.equal(on_side, first), "a side stream gives other bytes"
    # the flat form (no frame size), the float form (= the reference's .float()), a threshold of the call's own
    flat = va.attention_masks(att=att, upsample=False)
    assert flat.shape == att.shape and torch.equal(flat.view(-1, 6, 28, 28), va.attention_masks(att=att, frame_size=(224, 224), upsample=False))
    assert torch.equal(mt.upsample_ref(flat.view(-1, 6, 28, 28).cpu(), 28, 28, 224, 224), first.cpu())
    asf = va.attention_masks(att=att, frame_size=(224, 224), dtype=torch.float32)
    assert asf.dtype == torch.float32 and torch.equal(asf, first.float())
    assert va.threshold == 0.6 and torch.equal(first, va.attention_masks(att=att, frame_size=(224, 224), threshold=0.6))
    fewer = va.attention_masks(att=att, frame_size=(224, 224), threshold=0.2)
    assert fewer.sum().item() < first.sum().item() and (first[fewer.bool()] == 1).all(), "a smaller share keeps a subset"
    with pytest.raises(ValueError, match="frame_size"):
        va.attention_masks(att=att)
    with pytest.raises(ValueError, match="patches"):
        va.attention_masks(att=att, frame_size=(224, 232))
    with pytest.raises(ValueError, match="out must be"):
        va.attention_masks(att=att, frame_size=(224, 224), out=out.float())


def test_finite_guard_is_a_data_check():
    """One NaN in `att`: finite_check="sync" raises MaavssError, finite_check=None returns, and the next clean call is clean."""
    from maavss_amd._lib import MaavssError
    va = _extractor()
    att = mt.synthetic_att(28, 28, 6, 0.6)
    clean = va.attention_masks(att=att.cuda(), upsample=False).cpu()
    bad = att.clone()
    bad[1, 2, 77] = float("nan")
    with pytest.raises(MaavssError, match="non-finite"):
        va.attention_masks(att=bad.cuda(), upsample=False)
    got = va.attention_masks(att=bad.cuda(), upsample=False, finite_check=None).cpu()
    rows = torch.ones(att.shape[:2], dtype=torch.bool)
    rows[1, 2] = False
    assert torch.equal(got[rows], clean[rows]), "a non-finite row disturbed other rows"
    assert torch.equal(va.attention_masks(att=att.cuda(), upsample=False).cpu(), clean)
    va.attention_masks(att=bad.cuda(), upsample=False, finite_check="deferred")
    with pytest.raises(MaavssError, match="non-finite"):
        va.check_finite()


@pytest.mark.parametrize("arch,act", [("vit_small", "f16"), ("vit_small", "bf16"), ("vit_base", "f16"), ("vit_base", "bf16")])
def test_attention_masks_end_to_end(arch, act):
    """Seeded weights, 5 frames of 64^2 in groups of 2 (frames_per_launch): the masks of att = cls_attention(frames) meet the
    kernel-against-twin criterion on att.cpu(); the frames= form has the right shape and dtype and agrees with it on decided elements."""
    from oracle import vit_ref_cpu as vref
    va = _extractor(arch, act, frames_per_launch=2)
    heads = va.spec.heads
    frames = vref.synthetic_frames(5, 64, 5).cuda()
    att = torch.cat([va.cls_attention(frames[s:s + 2]) for s in range(0, 5, 2)])      # the groups the frames= form runs
    assert att.shape == (5, heads, 64)
    for thr in (None, 0.1, 0.9):
        small = va.attention_masks(att=att, frame_size=(64, 64), upsample=False, threshold=thr)
        assert small.shape == (5, heads, 8, 8) and small.dtype == torch.uint8
        used = va.threshold if thr is None else thr
        mt.assert_masks_match(small.cpu().flatten(2), att.cpu(), used, f"{arch} {act} threshold {used}")
        full = va.attention_masks(frames, threshold=thr)
        assert full.shape == (5, heads, 64, 64) and full.dtype == torch.uint8 and full.is_cuda
        _, und = mt.masks_twin(att.cpu(), used)
        und_up = mt.upsample_ref(und.view(5, heads, 8, 8), 8, 8, 64, 64)
        want = mt.upsample_ref(small.cpu(), 8, 8, 64, 64)
        assert torch.equal(full.cpu()[~und_up], want[~und_up]), "frames= and att= disagree on decided elements"
    asf = va.attention_masks(frames, dtype=torch.float32, upsample=False)
    assert asf.shape == (5, heads, 8, 8) and asf.dtype == torch.float32 and ((asf == 0) | (asf == 1)).all()


# ---- against the fp32 twin ViT ---------------------------------------------------------------------------------------------------

_TWIN_ATT = {}


def mask_disagreement(arch, act, seed, frames=2, width=224, threshold=0.6):
    """Share of the patches decided for the fp32 twin's CLS attention whose mask, computed by attention_masks(frames) on the 16-bit
    extractor, differs from the twin mask of that fp32 attention."""
    from oracle import vit_ref_cpu as vref
    cfg = tw.S8 if arch == "vit_small" else tw.B8
    key = (arch, seed, frames, width)
    if key not in _TWIN_ATT:
        fr = vref.synthetic_frames(frames, width, seed + 2)
        with torch.no_grad():
            _TWIN_ATT[key] = (fr, tw.cls_attention(cfg, tw.seeded_state(cfg, seed), fr))
    fr, att32 = _TWIN_ATT[key]
    want, und = mt.masks_twin(att32, threshold)
    got = _extractor(arch, act, seed).attention_masks(fr.cuda(), upsample=False, threshold=threshold).cpu().flatten(2) != 0
    return ((got != want) & ~und).sum().item() / (~und).sum().item()


# measured on the MI355X (profiles/attn_masks_bench.json "mask_agreement": largest share over seeds 3, 4, 5) and the gate = twice that
MEASURED = {("vit_small", "f16"): 6.378e-4, ("vit_small", "bf16"): 3.827e-3, ("vit_base", "f16"): 4.253e-4, ("vit_base", "bf16"): 3.615e-3}


@pytest.mark.parametrize("seed", [3, pytest.param(4, marks=pytest.mark.slow), pytest.param(5, marks=pytest.mark.slow)])
@pytest.mark.parametrize("arch,act", list(MEASURED))
def test_masks_of_the_16_bit_extractor_against_the_fp32_twin(arch, act, seed):
    """How far the 16-bit storage of the extractor moves the mask boundary: threshold 0.6, 224^2, 2 frames, seeded weights.
    Measured share of decided patches that differ | gate (twice the largest over seeds 3, 4, 5):
        vit_small f16   0.011 % / 0.064 % / 0.043 % (1, 6, 4 of 9408 patches)      | 0.128 %
        vit_small bf16  0.298 % / 0.351 % / 0.383 %                                | 0.765 %
        vit_base  f16   0.037 % / 0.021 % / 0.043 % (7, 4, 8 of 18816 patches)     | 0.085 %
        vit_base  bf16  0.255 % / 0.361 % / 0.330 %                                | 0.723 %
    The f16 shares are a handful of patches, so they move in steps of one patch (0.011 % / 0.005 %) from seed to seed.
    """
    share = mask_disagreement(arch, act, seed)
    print(f"[masks] {arch} {act} seed {seed}: {share:.4%} of the decided patches differ from the fp32 twin's mask")
    assert share <= 2 * MEASURED[(arch, act)], (share, MEASURED[(arch, act)])
