"""CPU checks of what tests/test_video_edges_gpu.py relies on, at that file's own shapes and inputs: each twin of
oracle/video_edges_ref.py against an independent restatement (torch operators, the reference's slicing formulation, a float64
evaluation), the exactness conditions (IEEE rounding of the tie inputs, constant planes), the caps (every wrap case really exceeds
its kernel's grid, every dispatch lands on the instantiation the case names, no phasegram bin is undecided) and, per group, the
sensitivity of the committed cases: a twin with ONE deliberate defect must differ from the twin by a bit (exact groups) or by more
than the bound, on at least one case.  A reference that is wrong at an odd size, or a case that cannot tell a wrong clamp from a
right one, would make the GPU test meaningless without anyone noticing.  Figures are printed (`pytest -s`)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import video_edges_cases as cs
from oracle import avfm_ref_cpu as aref
from oracle import video_edges_ref as vref

U = vref.U


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def up8(x, H, W):
    """independent of vref.upsample8: F.interpolate(nearest, x 8) and zero padding; x [F, hp, wp] tensor"""
    y = F.interpolate(x[:, None], scale_factor=8, mode="nearest")[:, 0]
    return F.pad(y, (0, W - y.shape[2], 0, H - y.shape[1]))


# ------------------------------------------------------------------------------------------------ 1. attention maps
def test_attention_map_twin():
    told = {"px_le": [], "diff_crosses_clip": []}
    for case in cs.ATTN_CASES:
        h, w, heads, frames, tc, diff = case
        hp, wp = h // 8, w // 8
        n = hp * wp
        att = cs.attn_input(case)
        assert att.shape == (frames, heads, n) and att.dtype == np.float32 and (att > 0).all()
        out, small, fmax = cs.attn_want(case)
        assert out.dtype == small.dtype == fmax.dtype == np.float32 and out.shape == (frames, h, w)
        # float64 restatement in the reference's order (sum heads, / frame max, temporal difference, / clip max)
        a64 = torch.from_numpy(att).double()
        v = a64.sum(1)
        v = v / v.amax(1, keepdim=True)
        scale = 1.0
        if tc > 0:
            c = v.view(-1, tc, n)
            if diff:
                c = torch.cat([torch.zeros_like(c[:, :1]), c[:, 1:] - c[:, :-1]], 1)
                assert float(c.amax((1, 2)).min()) > 0          # no static clip (0 * inf is out of scope)
            scale = float((1 / c.amax((1, 2))).max())
            v = (c / c.amax((1, 2), keepdim=True)).reshape(frames, n)
        want = up8(v.view(frames, hp, wp), h, w).numpy()
        # heads - 1 additions, the reciprocal, two products (and with diff one subtraction of two such values, scaled by 1 / clip max)
        tol = (heads + 4) * U * (2 * scale if diff else 1.0)
        err = np.abs(out.astype(np.float64) - want).max()
        print(f"[attn twin] {case}: |twin - float64| {err:.2e}, allowed {tol:.2e}")
        assert err <= tol, (case, err, tol)
        assert (out[:, hp * 8:] == 0).all() and (out[:, :, wp * 8:] == 0).all()
        if tc > 0 and not diff:
            assert np.array_equal(fmax, small.max(1))
        for name in told:
            if name == "diff_crosses_clip" and not diff:
                continue
            mut = vref.attn_maps(att, h, w, tc, diff, **{name: True})[0]
            if not same_bits(mut, out):
                told[name].append(case)
    print(f"[attn twin] cases that tell the mutants apart: { {k: len(v) for k, v in told.items()} }")
    assert told["px_le"] and told["diff_crosses_clip"], told
    # the caps: loop trips of pass 1 and the pass-2 grid
    ns = [(c[0] // 8) * (c[1] // 8) for c in cs.ATTN_CASES]
    assert {1, 63, 64, 65, 255, 256, 257, 784} <= set(ns)
    h, w, _, frames, tc, _ = cs.ATTN_WRAP
    total4 = frames * h * (w // 4)
    assert cs.GRID_CAP < total4 < 2 * cs.GRID_CAP and frames % tc == 0
    assert any(c[4] == 0 for c in cs.ATTN_CASES) and any(c[4] == 1 for c in cs.ATTN_CASES)
    assert any(c[1] % 8 == 4 for c in cs.ATTN_CASES) and any(c[0] % 8 == 4 for c in cs.ATTN_CASES)


# ------------------------------------------------------------------------------------------------ 2. patchify
def test_patchify_reference_and_ieee_rounding():
    sp = torch.tensor(cs.PATCHIFY_SPECIALS, dtype=torch.float32)
    assert np.array_equal(bits(sp.numpy()), bits(np.array(cs.PATCHIFY_SPECIALS, np.float64).astype(np.float32)))      # all exact in float32
    want_bf = torch.tensor(cs.PATCHIFY_SPECIALS_BF16, dtype=torch.float32)
    want_h = torch.tensor(cs.PATCHIFY_SPECIALS_F16, dtype=torch.float32)
    # torch rounds as the IEEE rule says (written out by hand in the cases file), signs of zero included
    assert same_bits(sp.to(torch.bfloat16).float().numpy(), want_bf.numpy())
    assert same_bits(sp.half().float().numpy(), want_h.numpy())
    assert want_bf.to(torch.bfloat16).float().equal(want_bf) and want_h.half().float().equal(want_h)
    for case in cs.PATCHIFY_CASES:
        frames, h, w = case
        hp, wp = h // 8, w // 8
        x = cs.patchify_input(case)
        assert x[0, 0, :2, :8].reshape(-1).equal(sp) or same_bits(x[0, 0, :2, :8].reshape(-1).numpy(), sp.numpy())
        # independent gather: rows[f, 1 + py wp + px, c 64 + dy 8 + dx] = x[f, c, 8 py + dy, 8 px + dx]
        rows = np.zeros((frames, hp * wp + 1, 192), np.float32)
        xn = x.numpy()
        for py in range(hp):
            for px in range(wp):
                rows[:, 1 + py * wp + px] = xn[:, :, 8 * py:8 * py + 8, 8 * px:8 * px + 8].reshape(frames, 192)
        rows = rows.reshape(-1, 192)
        got_bf = vref.patchify_ref(x, 0)
        got_h = vref.patchify_ref(x, 2)
        assert got_bf.dtype == torch.bfloat16 and got_h.dtype == torch.float16 and got_bf.shape == rows.shape
        assert np.array_equal(got_bf.view(torch.int16).numpy().view(np.uint16), vref.round_bf16_bits(rows))      # integer RNE
        with np.errstate(over="ignore"):
            assert np.array_equal(got_h.view(torch.int16).numpy().view(np.uint16), rows.astype(np.float16).view(np.uint16))      # numpy's RNE
    assert any(c[1] % 8 for c in cs.PATCHIFY_CASES) and any(c[2] % 8 == 4 for c in cs.PATCHIFY_CASES)


# ------------------------------------------------------------------------------------------------ 3. window kernels
def _clips_ref(maps, start, tc, diff, rcp, h, w, up):
    """the reference's formulation: normalise whole clips [n_clips, tc, H, W] (attention_frames(clip, clip_frames = tc)), windows are
    slices x_attn[:, :, j:j + n] of them"""
    n_frames = maps.shape[0]
    m = torch.from_numpy(maps)
    out = []
    for c in range(len(start)):
        f0 = int(torch.clamp(torch.tensor(int(start[c])), 0, n_frames - tc))
        clip = m[f0:f0 + tc]
        if diff:
            clip = torch.cat([torch.zeros_like(clip[:1]), clip[1:] - clip[:-1]])
        clip = clip * float(rcp[c])
        out.append(up8(clip.view(tc, h // 8, w // 8), h, w) if up else clip.view(tc, h, w))
    return torch.stack(out)


def test_window_twins():
    # --- clip scale
    n_frames = cs.CLIP_SCALE_FRAMES
    told_clamp = 0
    for e, tc in cs.CLIP_SCALE_CASES:
        start = cs.clip_starts(n_frames, tc)
        assert start[0] < 0 and start[1] == 0 and start[2] == n_frames - tc and start[3] > n_frames - tc
        maps = cs.rand((n_frames, e), "clip_scale", e, tc).numpy()
        fmax = (cs.rand((n_frames,), "clip_scale_fmax", e, tc) + 0.5).numpy()
        m = torch.from_numpy(maps)
        for mode in ("fmax", "maps", "diff"):
            got = vref.clip_scale(maps, fmax if mode == "fmax" else None, start, tc, mode == "diff")
            for c, f0 in enumerate((0, 0, n_frames - tc, n_frames - tc)):
                clip = m[f0:f0 + tc]
                mx = torch.from_numpy(fmax)[f0:f0 + tc].max() if mode == "fmax" else clip.max() if mode == "maps" else \
                    torch.clamp((clip[1:] - clip[:-1]).max(), min=0)
                assert bits(got[c:c + 1])[0] == bits((1.0 / mx).numpy().reshape(1))[0], (e, tc, mode, c)
            told_clamp += not same_bits(got, vref.clip_scale(maps, fmax if mode == "fmax" else None, start, tc, mode == "diff", clamp=False))
    assert told_clamp > 0
    # --- attention windows
    told = {"clamp": 0, "zero_k0": 0, "px_le": 0}
    for name, case in cs.ATTN_WIN_CASES.items():
        h, w, up, n_frames, tc, num_seq, win, w0, n_win = case
        assert num_seq - 1 + win <= tc and w0 + n_win <= 4 * num_seq
        for diff in (0, 1):
            p = cs.attn_win_problem(name, diff)
            clips = _clips_ref(p["maps"], p["clip_start"], tc, diff, p["rcp"], h, w, up)
            ref = torch.stack([clips[(w0 + i) // num_seq, (w0 + i) % num_seq:(w0 + i) % num_seq + win] for i in range(n_win)])
            assert same_bits(p["want"], ref.numpy()), (name, diff)
            args = (p["maps"], p["rcp"], p["clip_start"], tc, num_seq, win, w0, n_win, h, w, up, diff)
            told["clamp"] += not same_bits(p["want"], vref.attn_windows(*args, clamp=False))
            told["zero_k0"] += diff and not same_bits(p["want"], vref.attn_windows(*args, zero_k0=False))
            told["px_le"] += bool(up) and not same_bits(p["want"], vref.attn_windows(*args, px_le=True))
    print(f"[window twins] attention-window cases that tell the mutants apart: {told}")
    assert all(told.values()), told
    cases = list(cs.ATTN_WIN_CASES.values())
    assert any(c[5] - 1 + c[6] == c[4] for c in cases) and any(c[5] == 1 for c in cases) and any(c[6] == 1 for c in cases)
    assert any(c[7] > 0 and (c[7] + c[8]) % c[5] for c in cases)
    h, w, _, _, _, _, win, _, n_win = cs.ATTN_WIN_WRAP
    assert cs.GRID_CAP < n_win * win * h * (w // 4) < 2 * cs.GRID_CAP
    # --- STFT windows: the reference's y[:, :, a j : a (j + n)] as an unfold
    for name, (a, f, rows, n_clips, num_seq, win, w0, n_win) in cs.STFT_WIN_CASES.items():
        assert a * (num_seq - 1 + win) <= rows and w0 + n_win <= n_clips * num_seq
        vector = (a * f) % 4 == 0 and (rows * f) % 4 == 0                 # the dispatch condition of maavss_av_stft_windows
        assert vector == cs.STFT_WIN_VECTOR[name], name
        if name.startswith("wrap"):
            assert cs.GRID_CAP < cs.stft_win_items(name) < 2 * cs.GRID_CAP
            continue
        y = cs.randn((n_clips, 2, rows, f), "stft_win", name)
        un = y.unfold(2, a * win, a)                                      # [n_clips, 2, offsets, F, a win]
        ref = torch.stack([un[(w0 + i) // num_seq, :, (w0 + i) % num_seq].transpose(1, 2) for i in range(n_win)])
        assert same_bits(vref.stft_windows(y.numpy(), a, num_seq, win, w0, n_win), ref.numpy()), name
    assert (8 * 129) % 4 == 0 and (89 * 129) % 4 != 0                     # the case the alignment fix is for
    # --- stitch: torch.cat of the scaled windows
    for name, (a, f, n_clips, num_seq, w0, n_win) in cs.STITCH_CASES.items():
        assert w0 + n_win <= n_clips * num_seq
        if name.startswith("wrap"):
            assert cs.GRID_CAP < cs.stitch_items(name) < 2 * cs.GRID_CAP
            continue
        assert w0 > 0 and w0 + n_win < n_clips * num_seq                  # rows in front and behind stay untouched
        pred = cs.randn((n_win, 2, a, f), "stitch", name)
        amax = cs.rand((n_clips,), "stitch_amax", name) + 0.5
        for use in (False, True):
            out = np.full((2, a * n_clips * num_seq, f), 777.0, np.float32)
            vref.stitch(pred.numpy(), amax.numpy() if use else None, n_clips, num_seq, w0, out)
            g = (amax + 1e-7)[(torch.arange(n_win) + w0) // num_seq] if use else torch.ones(n_win)
            ref = torch.cat(list((pred * g[:, None, None, None]).transpose(0, 1).unbind(1)), 1)      # [2, a n_win, F]
            assert same_bits(out[:, a * w0:a * (w0 + n_win)], ref.numpy()), (name, use)
            assert (out[:, :a * w0] == 777).all() and (out[:, a * (w0 + n_win):] == 777).all()


# ------------------------------------------------------------------------------------------------ 4. video transform
def _torch_weights(n_in, S, antialias):
    """[S, n_in]: torch's float32 resize of the one-hot rows along the last axis is its weight table"""
    eye = torch.eye(n_in).view(n_in, 1, 1, n_in).expand(n_in, 1, 2, n_in).contiguous()
    return F.interpolate(eye, size=(2, S), mode="bilinear", align_corners=False, antialias=antialias)[:, 0, 0].numpy().T


def test_video_transform_twin():
    video = cs.vt_video()
    # the tap tables are torch's, bit for bit, at every (crop side, S) of the cases
    for n_in in sorted({b[2] for b in cs.VT_BOXES} | {b[3] for b in cs.VT_BOXES}):
        for S in cs.VT_SIZES:
            for aa in (False, True):
                start, count, wts = vref.vt_tables(n_in, S, aa, fold=False)
                assert int(count.max()) <= vref.vt_taps(n_in, S, aa) and int(count.min()) >= 1
                full = np.zeros((S, n_in), np.float32)
                for o in range(S):
                    for j in range(count[o]):
                        full[o, min(start[o] + j, n_in - 1)] += wts[o, j]
                assert same_bits(full, _torch_weights(n_in, S, aa)), (n_in, S, aa)
    worst_ulps, told_short = 0.0, 0
    for S, cf in cs.VT_CASES:
        for aa in (False, True):
            for c, (top, left, h, w) in enumerate(cs.vt_boxes(cf)):
                crop = video[c * cf:(c + 1) * cf, top:top + h, left:left + w]
                acc, adds = vref.vt_resize_f64(crop, S, aa)
                t32 = F.interpolate(torch.from_numpy(crop).permute(0, 3, 1, 2).float(), size=(S, S), mode="bilinear", align_corners=False,
                                    antialias=aa).double().numpy()
                # torch's float32 evaluation of the same tables: within the bound the kernel is held to (here without the affine step)
                bound = U * adds[None, None] * acc + vref.ulp32(acc)
                ulps = float((np.abs(t32 - acc) / vref.ulp32(acc)).max())
                worst_ulps = max(worst_ulps, ulps)
                assert (np.abs(t32 - acc) <= bound).all(), (S, cf, aa, c, ulps, float((np.abs(t32 - acc) / bound).max()))
                if (h, w) == (1, 1):                                    # the float32 weights of a one-pixel crop sum to exactly 1
                    assert (acc == crop.reshape(cf, 3, 1, 1)).all()
            for ac in (False, True):
                want, bound = cs.vt_want(S, cf, aa, ac)
                assert want.shape == bound.shape == (cs.VT_FRAMES, 3, S, S) and np.isfinite(want).all() and (bound > 0).all()
                mut, _ = vref.video_transform(video, cs.vt_boxes(cf), cf, S, cs.VT_MEAN, cs.VT_STD, aa, ac, short=True)
                told_short += bool((np.abs(mut - want) > bound).any())
                if cf == 1 and ac:                                      # the 1 x 1 box: scale = 1, min = 0 branch
                    plain, _ = cs.vt_want(S, cf, aa, False)
                    assert np.array_equal(want[1], np.clip(plain[1], 0, 1)) and (plain[1].reshape(3, -1).std(1) == 0).all()
    print(f"[video transform twin] torch float32 resize vs float64 sum over the float32 tables: worst {worst_ulps:.2f} ulp of the result; "
          f"{told_short} of {4 * len(cs.VT_CASES)} configurations tell a tap count one short")
    assert told_short > 0
    # why the tables are taken as given: an independent float64 resize (source coordinate in double) is not the same function --
    # after Normalize it is off by several times the bound the kernel is held to
    crop = torch.from_numpy(video[:1]).permute(0, 3, 1, 2)
    std = torch.tensor(cs.VT_STD).view(1, 3, 1, 1)
    for S in (100, 68):
        d = ((F.interpolate(crop.float() / 255, size=(S, S), mode="bilinear", align_corners=False).double() -
              F.interpolate(crop.double() / 255, size=(S, S), mode="bilinear", align_corners=False)) / std.double()).abs().max().item()
        print(f"[video transform twin] torch float32 vs float64 resize of the 37 x 53 frame -> {S}, normalised: {d:.2e}")
    assert d > 3 * cs.vt_want(68, 1, False, False)[1][0].max()
    assert 68 % 64 == 4 and 68 % 16 == 4 and all(s % 4 == 0 and s >= 8 for s in cs.VT_SIZES)


# ------------------------------------------------------------------------------------------------ 5. phasegram
def _phase_ref(case, diff, cum, norm):
    return cs.phase_ref(case, diff, cum, norm)


def test_phasegram_reference_bound_and_caps():
    told = {"shift_last_two": 0, "diff_crosses_batch": 0}
    for case in cs.PHASE_SMALL + (cs.PHASE_WRAP,):
        b, t, p = case
        frames = cs.phase_frames(case)
        noise, delta = cs.phase_noise(frames), cs.phase_delta(case)
        print(f"[phasegram] {case}: seed {cs.PHASE_SEEDS[case]}, |fft2 f32 - f64| measured {noise:.3e}, recorded {cs.PHASE_NOISE[case]:.3e}, "
              f"delta {delta:.3e}")
        # the recorded figure is this measurement (another FFT back end or vector width may move it a little; delta keeps >= 3 x noise)
        assert noise <= 1.25 * cs.PHASE_NOISE[case] and cs.PHASE_NOISE[case] <= 1.5 * noise
        z, und = cs.phase_spectrum(case)
        sc = vref.self_conjugate_mask(p)
        assert float(z.imag[..., sc].abs().max()) == 0 and not bool(torch.signbit(z.imag[..., sc]).any())      # angle 0 or +pi, as the kernel's
        options = cs.PHASE_OPTIONS if case in cs.PHASE_SMALL else cs.PHASE_WRAP_OPTIONS
        for diff, cum, norm in options:
            left = vref.phasegram_left_out(und, diff, cum)
            share = float(left.any(-1).float().mean())
            assert share <= cs.UNDECIDED_MAX_SHARE, (case, diff, cum, norm, share)
            # with `normalize` the global maximum would need an analysis of its own if an element were left out: none is
            assert int(left.sum()) == 0, (case, diff, cum, norm)
            ref = _phase_ref(case, diff, cum, norm)
            if t == 1 and diff:                        # the zero row; NaN with normalize (see cases.phase_ref)
                assert ref.shape == (b, 1, p * p) and bool(torch.isnan(ref).all() if norm else (ref == 0).all())
                continue
            bound = vref.phasegram_bound(z, delta, diff, cum, norm, ref)
            assert ref.shape == bound.shape == (b, t, p * p) and bool((bound >= 0).all()) and bool(torch.isfinite(bound).all())
            # soundness: torch's own float32 evaluation (spectrum error <= noise < delta) keeps the bound
            f32 = aref.video_phasegram_ref(frames[:, None], bool(diff), bool(cum), bool(norm))[:, 0].double()
            ratio = float(((f32 - ref).abs() / bound.clamp_min(1e-300))[~left].max())
            print(f"[phasegram] {case} diff {diff} cumulative {cum} normalize {norm}: torch float32 at {ratio:.3f} of the bound")
            assert ratio <= 1.0, (case, diff, cum, norm, ratio)
            # mutants: fftshift over the last two axes only; a difference that runs over the batch boundary
            zz = torch.fft.fftshift(torch.fft.fft2(frames.double()), dim=(-2, -1))
            ph = torch.angle(zz).reshape(b, t, -1)
            val = torch.cumsum(ph, -1) / (2 * math.pi * p * p) if cum else (ph + math.pi) / (2 * math.pi)
            if diff:
                val = torch.cat([torch.zeros_like(val[:, :1]), val[:, 1:] - val[:, :-1]], 1)
            if norm:
                val = val / val.abs().max()
            told["shift_last_two"] += bool(((val - ref).abs() > bound).any())
            if diff:
                flat = _phase_ref(case, 0, cum, 0).reshape(b * t, -1)
                mut = torch.cat([torch.zeros_like(flat[:1]), flat[1:] - flat[:-1]]).reshape(b, t, -1)
                mut = mut / mut.abs().max() if norm else mut
                told["diff_crosses_batch"] += bool(((mut - ref).abs() > bound).any())
    print(f"[phasegram] option sets that tell the mutants apart: {told}")
    assert all(told.values()), told
    b, t, p = cs.PHASE_WRAP
    assert b * t * p * p > 2048 * 256 and b % 2 == 1 and t % 2 == 1
    assert any(c[0] % 2 and c[1] % 2 and c[0] > 1 for c in cs.PHASE_SMALL) and cs.PHASE_SMALL[0][:2] == (1, 1)
