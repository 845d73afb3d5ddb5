"""csrc/optim.hip on the GPU against the float32 twin (tests/optim_twin.py): maavss_adamw_ema_step and maavss_swap_f32 on flat
buffers, the non-finite skip from TensorStats' norm, and TrainStep with weight decay, weight average and a warm-up schedule on the
avse_S golden shape.

Expected agreement: p, m, v and the average BIT FOR BIT equal to the f32 twin.  Derived, not measured: every operation of the definition
is an IEEE f32 add, multiply, divide or square root; optim.hip is compiled without contraction; for gfx950 the compiler lowers `/` to
v_div_scale / v_div_fmas / v_div_fixup and sqrtf to v_sqrt_f32 with the +-1 ulp correction, both correctly rounded; the kernels run with
f32 denormals enabled.  The flat cases keep every value in the normal range all the same (|g| in [1e-4, 10], exact zeros).

Grid: min(n / 4 / 256 + 1, 4096) workgroups of 256 threads of one float4 each: the grid-stride loop takes a second trip from
n > 4 * 4096 * 256 elements (BIG below is just past it)."""
import os

import numpy as np
import pytest
import torch

import maavss_amd
import optim_twin as tw
import stats_twin
from maavss_amd import _lib, ops, trainer
from maavss_amd.tensor_stats import TensorStats

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
PAD = 64
BIG = 4 * 4096 * 256 + 4 * 300 + 3
LR, SCALE, D = 1e-3, 0.37, 0.9


def _dev(x):
    """a device copy of x with PAD sentinels behind it -> (the view the kernel gets, the whole buffer)"""
    whole = torch.full((x.size + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    whole[:x.size].copy_(torch.from_numpy(x))
    return whole[:x.size], whole


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _same_bits(dev, host, what):
    got, want = _bits(dev), np.asarray(host, dtype=np.float32).view(np.int32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} elements differ from the twin, first at {bad[0]}: "
                           f"{got.view(np.float32)[bad[0]]!r} != {want.view(np.float32)[bad[0]]!r}")


def _table(n):
    """the decay table of a flat case: five segments with different decays, one of them 64 elements long, for the 4 * 1031 + 3 case;
    three around the second trip's start for BIG; one segment otherwise.  Ends at 64-element boundaries."""
    if n == 4 * 1031 + 3:
        return [128, 192, 1024, 2048, 4160], [0.1, 0.0, 0.05, 0.3, 0.01]
    if n == BIG:
        return [64, 4 * 4096 * 256, trainer._align(n)], [0.2, 0.0, 0.1]
    return [64], [0.1]


@pytest.mark.parametrize("ema,dev_scale", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("n", [1, 3, 4, 7, 4 * 1031 + 3])
def test_flat_kernel_equals_the_twin_bit_for_bit(n, ema, dev_scale):
    _run_flat_case(n, ema, dev_scale)


def test_flat_kernel_on_the_second_trip_of_the_grid_stride_loop():
    _run_flat_case(BIG, True, True)


def _run_flat_case(n, ema, dev_scale):
    p0, gs = tw.make_case(n, seed=n % 1000 + 7)
    ends, wd = _table(n)
    twin = tw.Twin(p0, "f32", ema=ema)
    (p, pw), (m, mw), (v, vw) = _dev(p0), _dev(np.zeros(n, np.float32)), _dev(np.zeros(n, np.float32))
    e, ew = _dev(p0) if ema else (None, None)
    scale = torch.tensor([SCALE], dtype=torch.float32, device="cuda") if dev_scale else None
    for step, g0 in enumerate(gs, 1):
        g, gw = _dev(g0)
        ops.adamw_ema_step(p, g, m, v, LR, step, ends, wd, ema=e, ema_decay=D, grad_scale=7.0 if dev_scale else SCALE, scale_dev=scale)
        twin.step(g0, LR, step, seg_ends=ends, seg_wd=wd, grad_scale=SCALE, ema_decay=D if ema else None)
        _same_bits(p, twin.p, f"p, step {step}")
        _same_bits(m, twin.m, f"m, step {step}")
        _same_bits(v, twin.v, f"v, step {step}")
        if ema:
            _same_bits(e, twin.e, f"ema, step {step}")
        _same_bits(g, g0, "g (read only)")
        for w in (pw, mw, vw, gw) + ((ew,) if ema else ()):
            assert bool((w[n:] == SENTINEL).all()), "a sentinel behind a buffer was overwritten"
    assert not np.array_equal(twin.p, p0)
    if ema:
        assert not np.array_equal(twin.e, twin.p) and not np.array_equal(twin.e, p0)


def test_decay_follows_the_table_and_zero_decay_is_the_undecayed_step():
    """the same gradients with an all-zero table: the segments whose decay is 0 keep their bytes, the others do not"""
    n = 4 * 1031 + 3
    p0, gs = tw.make_case(n, seed=3)
    ends, wd = _table(n)
    out = []
    for table_wd in (wd, [0.0] * len(wd)):
        (p, _), (m, _), (v, _) = _dev(p0), _dev(np.zeros(n, np.float32)), _dev(np.zeros(n, np.float32))
        for step, g0 in enumerate(gs, 1):
            ops.adamw_ema_step(p, _dev(g0)[0], m, v, LR, step, ends, table_wd)
        out.append(p.cpu().numpy())
    same = out[0] == out[1]
    lo = 0
    for e, w in zip(ends, wd):
        seg = same[lo:min(e, n)]
        assert seg.all() if w == 0.0 else not seg.any(), (lo, e, w)
        lo = e


def test_nonfinite_norm_skips_the_step_and_counts_it():
    n = 4 * 1031 + 3
    p0, gs = tw.make_case(n, seed=11)
    ends, wd = _table(n)
    g_bad = gs[0].copy()
    g_bad[1777] = np.nan
    flat = stats_twin.fake_flat(["a", "b"], [0, 2048], [2000, n - 2048], trainer._align(n))
    flat.params = torch.zeros(flat.total, device="cuda")
    stats = TensorStats(flat, bins=1)
    gbuf = torch.zeros(flat.total, device="cuda")

    def norm_of(g0):
        gbuf[:n].copy_(torch.from_numpy(g0))
        out = stats.run(gbuf, hist=False, max_norm=float("inf"), grad_scale=SCALE)
        return gbuf[:n], out["norm"], out["scale"]

    twin = tw.Twin(p0, "f32", ema=True)
    (p, pw), (m, mw), (v, vw), (e, ew) = _dev(p0), _dev(np.zeros(n, np.float32)), _dev(np.zeros(n, np.float32)), _dev(p0)
    skipped = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = dict(ema=e, ema_decay=D, grad_scale=SCALE)

    # step 1, clean: the norm is finite, the device scale is grad_scale exactly, the step is the twin's
    g, norm, scale = norm_of(gs[0])
    ops.adamw_ema_step(p, g, m, v, LR, 1, ends, wd, scale_dev=scale, norm_dev=norm, skipped=skipped, count_skip=True, **kw)
    twin.step(gs[0], LR, 1, seg_ends=ends, seg_wd=wd, grad_scale=SCALE, ema_decay=D)
    assert scale.item() == np.float32(SCALE) and np.isfinite(norm.item()) and skipped.item() == 0
    _same_bits(p, twin.p, "p, clean step 1")
    before = [w.clone() for w in (pw, mw, vw, ew)]

    # steps 2 and 3: one NaN in g -> NaN norm -> all four buffers keep their bytes, the count goes to 1, then 2
    for count in (1, 2):
        g, norm, scale = norm_of(g_bad)
        ops.adamw_ema_step(p, g, m, v, LR, 1 + count, ends, wd, scale_dev=scale, norm_dev=norm, skipped=skipped, count_skip=True, **kw)
        assert np.isnan(norm.item()) and skipped.item() == count
        for w, b in zip((pw, mw, vw, ew), before):
            assert np.array_equal(_bits(w), _bits(b)), "a skipped step changed a buffer"
    # a launch that skips but is not the counting one leaves the count alone
    ops.adamw_ema_step(p, g, m, v, LR, 3, ends, wd, scale_dev=scale, norm_dev=norm, skipped=skipped, count_skip=False, **kw)
    assert skipped.item() == 2 and np.array_equal(_bits(pw), _bits(before[0]))

    # step 4, clean: the twin's step at the ADVANCED step count (the stated deviation from GradScaler), from the unmoved moments
    g, norm, scale = norm_of(gs[1])
    ops.adamw_ema_step(p, g, m, v, LR, 4, ends, wd, scale_dev=scale, norm_dev=norm, skipped=skipped, count_skip=True, **kw)
    twin.step(gs[1], LR, 4, seg_ends=ends, seg_wd=wd, grad_scale=SCALE, ema_decay=D)
    for d, h, what in ((p, twin.p, "p"), (m, twin.m, "m"), (v, twin.v, "v"), (e, twin.e, "ema")):
        _same_bits(d, h, f"{what}, clean step after two skipped ones")
    assert skipped.item() == 2

    # with the skip off the same input does poison the state: the test above can fail
    g, norm, scale = norm_of(g_bad)
    ops.adamw_ema_step(p, g, m, v, LR, 5, ends, wd, scale_dev=scale, **kw)
    assert np.isnan(p.cpu().numpy()).all() and np.isnan(m.cpu().numpy()).all() and np.isnan(e.cpu().numpy()).all()
    for w in (pw, mw, vw, ew):
        assert bool((w[n:] == SENTINEL).all())


@pytest.mark.parametrize("n", [1, 5, 4 * 300 + 2])
def test_swap_exchanges_two_buffers_in_place(n):
    rng = np.random.default_rng(n)
    a0, b0 = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    (a, aw), (b, bw) = _dev(a0), _dev(b0)
    ops.swap_f32(a, b)
    _same_bits(a, b0, "a after the swap")
    _same_bits(b, a0, "b after the swap")
    assert bool((aw[n:] == SENTINEL).all()) and bool((bw[n:] == SENTINEL).all())
    ops.swap_f32(a, b)
    _same_bits(a, a0, "a after two swaps")
    _same_bits(b, b0, "b after two swaps")


# ---- TrainStep on the avse_S golden shape --------------------------------------------------------------------------------------------
def _seeded_models(golden_dir, count):
    from oracle import avse_ref_cpu as orc
    z = np.load(os.path.join(golden_dir, "avse_S.npz"), allow_pickle=False)
    m = {k[5:]: z[k].item() for k in z.files if k.startswith("meta_")}
    n_bins, t_a = m["fft_len"] // 2 + 1, m["hops_per_frame"] * m["frames"]
    shapes = ([m["batch"], 2, t_a, n_bins], [m["batch"], 1, m["frames"], m["width"], m["width"]], m["hops_per_frame"])
    sd = orc.seeded_state_dict(orc.AVFusionFramesRef(*shapes), m["seed"])
    models = []
    for _ in range(count):
        model = maavss_amd.AV_Fusion_Model_Frames(*shapes, precise=True)
        model.load_state_dict(sd, strict=True)
        models.append(model.to("cuda").train())
    batch = [t.cuda() for t in orc.synthetic_batch(m["batch"], m["frames"], m["width"], t_a, n_bins, m["hops_per_frame"], m["seed"] + 1)]
    return m, models, batch


def _follow(step, batch, source=None):
    """forward + backward of `step` without its optimizer step (marks the touched tensors); with `source` the gradient bytes are
    then replaced by that step's, whatever the backward's summation order"""
    step(*batch, optimizer_step=False)
    if source is not None:
        step.flat.grads.copy_(source.flat.grads)


def test_trainstep_decay_average_and_schedule_on_the_small_model(golden_dir):
    m, (m_ext, m_nodecay, m_off, m_plain, m_ema), batch = _seeded_models(golden_dir, 5)
    lr, coeff, wd = 100.0 * m["lr"], m["loss_coeff"], 0.1
    sched = lambda: maavss_amd.LRSchedule(lr, warmup_steps=2)      # noqa: E731
    ext = maavss_amd.TrainStep(m_ext, lr=sched(), loss_coeff=coeff, weight_decay=wd, ema_decay=D)
    nodecay = maavss_amd.TrainStep(m_nodecay, lr=sched(), loss_coeff=coeff, weight_decay=0.0, ema_decay=D)
    off = maavss_amd.TrainStep(m_off, lr=lr, loss_coeff=coeff, weight_decay=0.0, decay_filter=None, ema_decay=None, ema_warmup=False,
                               skip_nonfinite=False)
    plain = maavss_amd.TrainStep(m_plain, lr=lr, loss_coeff=coeff)
    assert ext.opt.extended and nodecay.opt.extended and not off.opt.extended and not plain.opt.extended
    flat = ext.flat
    twin = tw.Twin(flat.params.cpu().numpy(), "f32", ema=True)
    assert np.array_equal(_bits(ext.opt.ema), _bits(flat.params))
    decay_of = {n: wd for n in flat.names if ext.opt.decayed[n]}
    for t in range(3):
        _follow(ext, batch)
        runs = ext.opt._runs()
        assert runs and all(r[2] == t + 1 for r in runs)
        g = flat.grads.cpu().numpy()                               # the gradient bytes the kernel is about to read
        ext.opt.step()
        assert ext.opt.lr == lr * (t + 1) / 3 if t < 2 else ext.opt.lr == lr
        stepped = set()
        for ln in trainer.plan_launches(runs, flat, decay_of):
            twin.step(g, ext.opt.lr, ln["step"], seg_ends=ln["ends"], seg_wd=ln["wd"], ema_decay=D, sel=slice(ln["lo"], ln["hi"]))
            stepped.update(ln["names"])
        assert not any(n.startswith("stft_decoder.") for n in stepped) and "fc1.weight" in stepped
        for dev, host, what in ((flat.params, twin.p, "params"), (ext.opt.exp_avg, twin.m, "exp_avg"), (ext.opt.exp_avg_sq, twin.v, "exp_avg_sq"),
                                (ext.opt.ema, twin.e, "ema")):
            _same_bits(dev, host, f"{what}, step {t + 1}")
        # the same gradient bytes without decay: the undecayed tensors take the same steps, the decayed ones do not
        _follow(nodecay, batch, source=ext)
        nodecay.opt.step()
        for n in stepped:
            same = torch.equal(nodecay.flat.param_views[n], flat.param_views[n])
            assert same != ext.opt.decayed[n], (n, t)
        # all new keywords at their defaults: bit-identical to a TrainStep built without them
        _follow(off, batch)
        _follow(plain, batch, source=off)
        off.opt.step()
        plain.opt.step()
        assert torch.equal(off.flat.params, plain.flat.params) and torch.equal(off.opt.exp_avg, plain.opt.exp_avg)
        assert torch.equal(off.opt.exp_avg_sq, plain.opt.exp_avg_sq) and off.opt.steps == plain.opt.steps
    assert ext.opt.ema_updates == 3 and ext.opt.state_dict()["param_groups"][0]["lr"] == lr
    # frozen tensors were never stepped: their average is still their weight
    for n in flat.names:
        if n.startswith("stft_decoder."):
            o, k = flat.offsets[n], trainer._numel(flat.shapes[n])
            assert torch.equal(ext.opt.ema[o:o + k], flat.params[o:o + k]), n

    # ---- FusedAdam(skip_nonfinite=True) without clipping: the norm pass runs with max_norm = inf; one NaN skips the whole step
    guard = maavss_amd.FusedAdam(nodecay.flat, lr=lr, ema_decay=D, skip_nonfinite=True)
    nf = nodecay.flat
    keep = nf.grad_views["fc2.weight"][3, 5].clone()
    nf.grad_views["fc2.weight"][3, 5] = float("nan")
    before = nf.params.clone()
    guard.step()
    assert guard.skipped_steps.item() == 1 and np.isnan(guard.grad_norm.item())
    assert torch.equal(nf.params, before) and torch.equal(guard.ema, before) and not guard.exp_avg.any() and guard.step_count == 1
    nf.grad_views["fc2.weight"][3, 5] = keep
    guard.step()
    assert guard.skipped_steps.item() == 1 and guard.clip_scale.item() == 1.0 and np.isfinite(guard.grad_norm.item())
    assert not torch.equal(nf.params, before) and guard.step_count == 2

    # ---- ema_weights(): the swap, Validator inside the block, no synchronisation
    raw, avg = flat.params.clone(), ext.opt.ema.clone()
    assert not torch.equal(raw, avg)
    m_ema.load_state_dict(m_ext.state_dict(), strict=True)                       # the live BatchNorm statistics ...
    esd = ext.opt.ema_state_dict()
    assert int(esd.pop("num_updates")) == 3
    missing, unexpected = m_ema.load_state_dict(esd, strict=False)              # ... and the averaged parameters
    assert not unexpected and all(not k.split(".")[-1] in ("weight", "bias") or k.startswith("stft_autoencoder.") for k in missing), missing
    m_ext.eval()
    m_ema.eval()
    val_in, val_ref, val_raw = (maavss_amd.Validator(mm, loss_coeff=coeff) for mm in (m_ext, m_ema, m_ext))
    prev = maavss_amd.set_deterministic(True)           # no f32 atomics in the Linear kernels: two forward passes give the same bytes
    val_raw.add_windows(*batch)                                                  # raw weights; also warms every allocation up
    val_ref.add_windows(*batch)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")             # any blocking call of torch's raises
    try:
        with ext.ema_weights():
            val_in.add_windows(*batch)
            inside_p, inside_e = flat.params.clone(), ext.opt.ema.clone()
            inside_sd = {k: v.clone() for k, v in m_ext.state_dict().items()}
            with pytest.raises(_lib.MaavssError, match="not re-entrant"):
                ext.ema_weights().__enter__()
            with pytest.raises(_lib.MaavssError, match="inside ema_weights"):
                ext.opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        maavss_amd.set_deterministic(prev)
    assert torch.equal(inside_p, avg) and torch.equal(inside_e, raw), "inside the block the parameter buffer holds the average"
    assert torch.equal(flat.params, raw) and torch.equal(ext.opt.ema, avg), "after the block both buffers are restored"
    ref_sd = m_ema.state_dict()
    for k, v in inside_sd.items():
        assert torch.equal(v, ref_sd[k]), k
    assert torch.equal(val_in._buf, val_ref._buf), "Validator inside ema_weights() == a second model loaded from ema_state_dict()"
    assert not torch.equal(val_in._buf, val_raw._buf)
