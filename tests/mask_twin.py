"""TEST INFRASTRUCTURE ONLY -- a float64 CPU twin of the attention-mask contract (include/maavss.h, maavss_vit_attn_masks), the
inputs the mask tests share, and the comparison they apply.

The twin restates the reference's video_attention.py:59-68 with torch.sort(stable=True) in float64: sort a head's CLS attention over
the patches ascending (ties by patch index), divide by the row sum, inclusive cumulative sum c, keep a patch <=> its c > 1 - threshold,
write the flags back at the patches' own positions.  Beside the mask it says, per element, whether the element is UNDECIDED:
|c64 - (1 - threshold)| <= n * 2^-23.  That margin bounds what an f32 evaluation -- the summation of n non-negative terms that total 1,
in any association, plus one division per term -- can move c, so an f32 implementation must reproduce every DECIDED element bit for
bit, and only the undecided ones are left out of a comparison.  The margin is absolute, so it is coarse where c is small: at
threshold = 1 (cut 0) every patch whose cumulative share lies below n * 2^-23 counts as undecided although no f32 evaluation gets a
positive c wrong.  The cap on undecided elements per row, max(2, n / 256), is therefore a condition on the INPUTS of a test;
tests/test_attn_masks_cpu.py proves it for every synthetic case below, and `scales_for` is where threshold = 1 gets the flatter rows
(softmax scales 0.25 and 0.5 instead of 0.5, 1 and 3) that meet it.
"""
import torch

PATCH = 8
GRIDS = [(28, 28), (32, 32), (48, 48), (64, 64), (22, 40), (1, 1)]      # patch grids (hp, wp): 224^2, 256^2, 384^2, 512^2, 176x320, 8^2
HEADS = [6, 12]
THRESHOLDS = [0.0, 0.1, 0.6, 0.9, 1.0]
FRAMES_PER_SCALE = 2


def margin(n):
    return n * 2.0 ** -23


def cap(n):
    """Most undecided elements a row may have (a condition on test inputs, not a measurement)."""
    return max(2, n // 256)


def scales_for(threshold):
    """Softmax scales s of the synthetic rows softmax(s * randn).  At threshold = 1 the cut is 0 and the absolute margin swallows the
    small end of a peaked row (see the module docstring): flatter rows there."""
    return (0.25, 0.5) if threshold == 1.0 else (0.5, 1.0, 3.0)


def synthetic_att(hp, wp, heads, threshold, seed=0):
    """[F, heads, n] f32: FRAMES_PER_SCALE frames of softmax(s * randn) rows for every scale of `scales_for(threshold)`."""
    n, scales = hp * wp, scales_for(threshold)
    g = torch.Generator().manual_seed(1000 * seed + 17 * hp + wp + heads)
    rows = []
    for s in scales:
        rows.append(torch.softmax(s * torch.randn(FRAMES_PER_SCALE, heads, n, generator=g, dtype=torch.float64), -1).float())
    return torch.cat(rows)


EXACT_THRESHOLDS = [0.25, 0.5, 0.75, 0.9375]       # exact in f32, and so is 1 - threshold


def exact_tie_rows(n, frames=2, heads=6, seed=3):
    """[frames, heads, n] f32 rows of small integers (0 .. 7: many exact ties, zeros among them) whose total is a power of two -- patch 0
    takes the remainder.  value / total and every partial sum of those quotients, in any order, are exact in f32 and in f64 alike, so with
    a threshold of EXACT_THRESHOLDS an f32 implementation and the twin agree on every element; the ties pin the index rule."""
    g = torch.Generator().manual_seed(seed + n)
    a = torch.randint(0, 8, (frames, heads, n), generator=g).double()
    tot = a.sum(-1)
    a[..., 0] += 2.0 ** torch.ceil(torch.log2(tot)) - tot
    return a.float()


def masks_twin(att, threshold):
    """att [..., n] (any float dtype; evaluated in float64) -> (mask bool [..., n], undecided bool [..., n]) in patch order."""
    a = att.double()
    n = a.shape[-1]
    val, idx = torch.sort(a, dim=-1, stable=True)
    val = val / val.sum(-1, keepdim=True)
    c = torch.cumsum(val, -1)
    cut = 1.0 - float(threshold)
    keep = c > cut                                   # NaN > cut is False: a zero row keeps nothing
    und = (c - cut).abs() <= margin(n)               # and is decided
    mask = torch.zeros_like(keep).scatter(-1, idx, keep)
    undecided = torch.zeros_like(und).scatter(-1, idx, und)
    return mask, undecided


def upsample_ref(mask, hp, wp, h, w, patch=PATCH):
    """[..., hp, wp] -> [..., h, w]: every patch repeated patch x patch times, zero outside the patch grid."""
    m = mask
    assert m.shape[-2:] == (hp, wp)
    up = m.repeat_interleave(patch, -2).repeat_interleave(patch, -1)
    out = torch.zeros(*m.shape[:-2], h, w, dtype=mask.dtype)
    out[..., :hp * patch, :wp * patch] = up
    return out


def assert_masks_match(got, att, threshold, label=""):
    """The kernel-against-twin criterion: `got` [..., n] (0 / 1 values, any dtype) equals the twin's mask on every decided element, and no
    row of the input has more undecided elements than the cap.  -> number of undecided elements that differ (informative)."""
    want, und = masks_twin(att, threshold)
    n = att.shape[-1]
    worst = int(und.sum(-1).max())
    assert worst <= cap(n), f"{label}: a row has {worst} undecided elements, the cap for n = {n} is {cap(n)} (test input, not the kernel)"
    g = got.reshape(want.shape)
    assert ((g == 0) | (g == 1)).all(), f"{label}: mask values other than 0 / 1"
    diff = (g != 0) != want
    bad = diff & ~und
    assert not bad.any(), f"{label}: {int(bad.sum())} decided elements differ from the float64 twin (of {bad.numel()})"
    return int(diff.sum())
