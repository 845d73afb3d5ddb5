"""CPU-only part of the optimizer extension (csrc/optim.hip, FusedAdam's weight decay / weight average / non-finite skip,
maavss_amd.LRSchedule): the float64 twin against torch.optim.AdamW, the schedule, launch planning, state dicts, checkpoints and the
argument checks of the two entry points (every call below fails before any launch)."""
import ctypes
import inspect
import os
import types

import numpy as np
import pytest
import torch

import maavss_amd
import optim_twin as tw
from maavss_amd import _lib, trainer

SHAPES = ([2, 2, 64, 129], [2, 1, 8, 128, 128], 8)


# ---- the twin ------------------------------------------------------------------------------------------------------------------------
def test_f64_twin_equals_torch_adamw_on_double_tensors():
    """Mixed decayed / undecayed tensors, a gradient scale, 5 steps.  Bound per step and element, u = 2^-53:
    * p * decay and the final subtraction: one rounding each in either implementation, of values <= |p|max: 2 * 2 u |p|max;
    * the update lr_bc1 * m / den: torch forms m by lerp (m + (g - m)(1 - b1)), v by mul + addcmul and den by sqrt(v) / sqrt(bc2) + eps,
      the twin by the expressions of optim_twin -- a handful (< 16) of roundings each.  An absolute error dm of m enters the update as
      lr_bc1 * dm / den with den >= sqrt(v) >= sqrt(1 - b2) b2^(k/2) |g_k| for every past gradient g_k that m still holds with weight
      (1 - b1) b1^k, so |dm| / den <= 16 u / sqrt(1 - b2) (b1 < sqrt(b2)) and lr_bc1 <= lr / (1 - b1): the update differs by at most
      lr * 16 u / ((1 - b1) sqrt(1 - b2)) < 5100 lr u; the relative errors of den add < 16 u |update|, |update| <= lr_bc1 |m| / den
      <= the same bound's scale, covered by doubling it.
    Over T steps the differences add (the state error is carried along): T * (4 |p|max + 10200 lr) * u."""
    rng = np.random.default_rng(0)
    sizes, wds = [5, 64, 7, 130], [0.05, 0.0, 0.3, 0.0]
    lr, betas, eps, scale, steps = 1e-2, (0.9, 0.999), 1e-8, 0.37, 5
    ps = [rng.uniform(-2, 2, k) for k in sizes]
    params = [torch.nn.Parameter(torch.tensor(p, dtype=torch.float64)) for p in ps]
    topt = torch.optim.AdamW([dict(params=[q], weight_decay=w) for q, w in zip(params, wds)], lr=lr, betas=betas, eps=eps)
    ends = list(np.cumsum(sizes))
    twin = tw.Twin(np.concatenate(ps), mode="f64", betas=betas, eps=eps)
    pmax = 0.0
    for t in range(1, steps + 1):
        gs = [rng.normal(0, 3, k) for k in sizes]
        for q, g in zip(params, gs):
            q.grad = torch.tensor(g * scale, dtype=torch.float64)
        topt.step()
        twin.step(np.concatenate(gs), lr, t, seg_ends=ends, seg_wd=wds, grad_scale=scale)
        want = np.concatenate([q.detach().numpy() for q in params])
        pmax = max(pmax, np.abs(want).max())
        err, bound = np.abs(twin.p - want).max(), t * (4 * pmax + 10200 * lr) * tw.U53
        print(f"step {t}: max |twin - torch| {err:.3g}, bound {bound:.3g}")
        assert err <= bound
    # the decay did something, and only where it was asked for
    plain = tw.Twin(np.concatenate(ps), mode="f64", betas=betas, eps=eps)
    rng = np.random.default_rng(0)
    [rng.uniform(-2, 2, k) for k in sizes]
    for t in range(1, steps + 1):
        plain.step(np.concatenate([rng.normal(0, 3, k) for k in sizes]), lr, t, grad_scale=scale)
    same = plain.p == twin.p
    assert same[5:69].all() and same[76:].all() and not same[:5].any() and not same[69:76].any()


def test_twin_average_equals_the_plain_recurrence_and_torch_lerp():
    rng = np.random.default_rng(1)
    n, d, lr = 50, 0.9, 1e-2
    p0 = rng.uniform(-1, 1, n)
    twin = tw.Twin(p0, mode="f64", ema=True)
    e, et = p0.copy(), torch.tensor(p0)
    assert np.array_equal(twin.e, p0)
    for t in range(1, 6):
        twin.step(rng.normal(0, 1, n), lr, t, ema_decay=d)
        e = d * e + (1.0 - d) * twin.p
        et.lerp_(torch.tensor(twin.p), 1.0 - d)
        assert np.array_equal(twin.e, e)                                        # the same three roundings
        assert np.abs(twin.e - et.numpy()).max() <= 4 * tw.U53 * np.abs(e).max()      # lerp's form: e + (p - e)(1 - d), 3 roundings too
    assert not np.array_equal(twin.e, twin.p)
    assert [tw.ema_warmup_decay(0.999, t) for t in (0, 1, 90)] == [0.1, 2.0 / 11.0, 91.0 / 100.0] and tw.ema_warmup_decay(0.5, 90) == 0.5


def test_f32_twin_rounds_every_operation_in_float32():
    """The f32 mode stays in float32 (Twin.step asserts the dtypes) and differs from the f64 mode by f32 rounding, not more."""
    p, gs = tw.make_case(4 * 1031 + 3, 3)
    a, b = tw.Twin(p, "f32", ema=True), tw.Twin(p, "f64", ema=True)
    for t, g in enumerate(gs, 1):
        a.step(g, 1e-3, t, seg_ends=[4096, 4192], seg_wd=[0.1, 0.0], grad_scale=0.37, ema_decay=0.9)
        b.step(g, 1e-3, t, seg_ends=[4096, 4192], seg_wd=[0.1, 0.0], grad_scale=0.37, ema_decay=0.9)
    assert a.p.dtype == a.m.dtype == a.v.dtype == a.e.dtype == np.float32
    assert np.abs(a.p - b.p).max() <= 3 * 16 * tw.U24 * 2.0 and not np.array_equal(a.p.astype(np.float64), b.p)
    fin = np.concatenate([a.p, a.m, a.v, a.e])
    assert not np.any((fin != 0) & (np.abs(fin) < np.finfo(np.float32).tiny)), "no subnormal in the test data's results"


# ---- LRSchedule ----------------------------------------------------------------------------------------------------------------------
def test_lr_schedule_values():
    s = maavss_amd.LRSchedule(1e-3, warmup_steps=4, total_steps=20, kind="cosine", min_lr=1e-5)
    assert s.lr(0) == 1e-3 / 5 and s.lr(1) == 1e-3 * 2 / 5 and s.lr(3) == 1e-3 * 4 / 5
    assert s.lr(4) == 1e-3                                                       # the warm-up's end: the base rate
    assert abs(s.lr(12) - (1e-5 + (1e-3 - 1e-5) * 0.5)) < 1e-18                  # half way down the cosine
    assert s.lr(19) > s.lr(20) == 1e-5 == s.lr(21) == s.lr(10 ** 6)              # at total_steps and beyond: min_lr, constant
    assert all(s.lr(t) > s.lr(t + 1) for t in range(4, 20))
    lin = maavss_amd.LRSchedule(1.0, warmup_steps=0, total_steps=10, kind="linear", min_lr=0.5)
    assert lin.lr(0) == 1.0 and lin.lr(5) == 0.75 and lin.lr(10) == 0.5 == lin.lr(11)
    const = maavss_amd.LRSchedule(2e-4, warmup_steps=2)
    assert [const.lr(t) for t in range(4)] == [2e-4 / 3, 2e-4 * 2 / 3, 2e-4, 2e-4]
    const.scale = 0.5
    assert const.lr(7) == 1e-4
    for bad in (dict(kind="step"), dict(kind="cosine"), dict(kind="linear", total_steps=3, warmup_steps=3), dict(warmup_steps=-1)):
        with pytest.raises(ValueError):
            maavss_amd.LRSchedule(1e-3, **bad)


def test_lr_schedule_state_dict_round_trip():
    s = maavss_amd.LRSchedule(1e-3, warmup_steps=3, total_steps=9, kind="linear", min_lr=1e-4)
    got = [s.next_lr() for _ in range(5)]
    assert got == [s.lr(t) for t in range(5)] and s.t == 5
    s.scale = 0.25
    sd = s.state_dict()
    assert all(isinstance(v, (int, float, str, type(None))) for v in sd.values())        # loads under torch.load(weights_only=True)
    r = maavss_amd.LRSchedule(7.0)
    r.load_state_dict(sd)
    assert r.state_dict() == sd and r.t == 5
    assert [r.next_lr() for _ in range(6)] == [s.next_lr() for _ in range(6)]


# ---- FusedAdam: planning, state, defaults ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return maavss_amd.AV_Fusion_Model_Frames(*SHAPES)


def _check_plan(plan, flat, runs):
    """the launches tile the runs; ends ascend, are multiples of 4 and the last covers the launch"""
    assert sum(len(ln["names"]) for ln in plan) == sum(len(r[3]) for r in runs)
    for ln in plan:
        assert len(ln["ends"]) == len(ln["wd"]) == len(ln["names"]) <= 64
        assert ln["lo"] == flat.offsets[ln["names"][0]] and ln["lo"] % 64 == 0 and ln["hi"] <= flat.total
        assert all(e % 4 == 0 for e in ln["ends"]) and all(a < b for a, b in zip(ln["ends"], ln["ends"][1:]))
        assert ln["ends"][-1] >= ln["hi"] - ln["lo"]
        for n, e in zip(ln["names"], ln["ends"]):
            assert ln["lo"] + e >= flat.offsets[n] + trainer._numel(flat.shapes[n])


def test_launch_planning_on_the_small_model(model):
    opt = maavss_amd.FusedAdam(model, lr=1e-3, weight_decay=0.01)
    flat = opt.flat
    assert opt.extended
    # default filter: two or more dimensions
    for n in flat.names:
        assert opt.decayed[n] == (len(flat.shapes[n]) >= 2), n
    assert opt.decayed["lstm.weight_hh_l0"] and opt.decayed["fc1.weight"] and opt.decayed["visual_encoder.0.weight"]
    assert not opt.decayed["visual_encoder.1.weight"] and not opt.decayed["visual_encoder.1.bias"]      # BatchNorm weight and bias
    flat.mark(flat.names)
    runs = opt._runs()
    assert len(runs) == 1 and runs[0][0] == 0 and runs[0][2] == 1
    wd = {n: 0.01 for n in flat.names if opt.decayed[n]}
    plan = trainer.plan_launches(runs, flat, wd)
    _check_plan(plan, flat, runs)
    assert len(plan) == -(-len(flat.names) // 64)
    assert [w for ln in plan for w in ln["wd"]] == [0.01 if opt.decayed[n] else 0.0 for n in flat.names]
    # a smaller table capacity forces a split: consecutive launches, each its own table relative to its own start
    small = trainer.plan_launches(runs, flat, wd, max_segments=4)
    _check_plan(small, flat, runs)
    assert len(small) == -(-len(flat.names) // 4) and all(a["hi"] <= b["lo"] for a, b in zip(small, small[1:]))
    # a custom filter
    only = maavss_amd.FusedAdam(flat, lr=1e-3, weight_decay=0.01, decay_filter=lambda n, p: n.startswith("fc"))
    assert [n for n in flat.names if only.decayed[n]] == [n for n in flat.names if n.startswith("fc")]
    # frozen tensors: left out of the runs, which then split; every launch's table starts at its own first tensor
    frozen = [n for n in flat.names if n.startswith("fc1.")]
    for n in frozen:
        flat.tensors[n].requires_grad_(False)
    try:
        runs = opt._runs()
        assert len(runs) == 2 and not any(n in frozen for r in runs for n in r[3])
        plan = trainer.plan_launches(runs, flat, wd)
        _check_plan(plan, flat, runs)
        lo, hi = flat.offsets[frozen[0]], flat.offsets[frozen[-1]] + trainer._numel(flat.shapes[frozen[-1]])
        assert all(ln["hi"] <= lo or ln["lo"] >= hi for ln in plan)
    finally:
        for n in frozen:
            flat.tensors[n].requires_grad_(True)
        flat.touched.clear()


def test_more_than_64_segments_are_split():
    names = [f"t{i}" for i in range(150)]
    numels = [1 + (i * 37) % 200 for i in range(150)]
    offsets, off = [], 0
    for k in numels:
        offsets.append(off)
        off = trainer._align(off + k)
    flat = types.SimpleNamespace(names=names, offsets=dict(zip(names, offsets)), shapes={n: (k,) for n, k in zip(names, numels)}, total=off)
    runs = [(0, off, 1, names)]
    plan = trainer.plan_launches(runs, flat, {n: 0.1 for n in names[::2]})
    _check_plan(plan, flat, runs)
    assert [len(ln["names"]) for ln in plan] == [64, 64, 22]
    assert plan[1]["lo"] == offsets[64] and plan[2]["lo"] == offsets[128] and plan[2]["hi"] == off
    assert plan[1]["wd"][:2] == [0.1, 0.0]


def test_signature_defaults_are_the_off_values(model):
    for cls in (maavss_amd.FusedAdam, maavss_amd.TrainStep):
        p = inspect.signature(cls.__init__).parameters
        assert p["weight_decay"].default == 0.0 and p["decay_filter"].default is None and p["ema_decay"].default is None
        assert p["ema_warmup"].default is False and p["skip_nonfinite"].default is False and p["max_grad_norm"].default is None
    opt = maavss_amd.FusedAdam(model, lr=1e-3)
    assert not opt.extended and opt.ema is None and opt.skipped_steps is None and opt.schedule is None
    assert opt.state_dict()["param_groups"][0]["weight_decay"] == 0 and "decoupled_weight_decay" not in opt.state_dict()["param_groups"][0]
    for kw in (dict(weight_decay=0.1), dict(ema_decay=0.9), dict(skip_nonfinite=True)):
        assert maavss_amd.FusedAdam(opt.flat, lr=1e-3, **kw).extended
    for bad in (dict(weight_decay=-1.0), dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(weight_decay=float("inf"))):
        with pytest.raises(ValueError):
            maavss_amd.FusedAdam(opt.flat, lr=1e-3, **bad)


def test_schedule_drives_the_rate_and_the_param_group(model):
    s = maavss_amd.LRSchedule(1e-3, warmup_steps=2)
    opt = maavss_amd.FusedAdam(model, lr=s)
    assert opt.lr == s.lr(0) == opt.state_dict()["param_groups"][0]["lr"]
    for t in range(3):
        opt.step()                       # nothing touched: no launch, but the schedule moves on
        assert opt.lr == s.lr(t) == opt.state_dict()["param_groups"][0]["lr"]
    assert s.t == 3


def test_adamw_state_dict_round_trip_with_torch(model):
    from oracle import avse_ref_cpu as orc
    twin = orc.AVFusionFramesRef(*SHAPES)
    model.load_state_dict(orc.seeded_state_dict(twin, 9), strict=True)
    fopt = maavss_amd.FusedAdam(model, lr=3e-4, weight_decay=0.02)
    g = torch.Generator().manual_seed(1)
    fopt.exp_avg.copy_(torch.randn(fopt.exp_avg.shape, generator=g))
    fopt.exp_avg_sq.copy_(torch.rand(fopt.exp_avg_sq.shape, generator=g))
    fopt.step_count = 7
    sd = fopt.state_dict()
    assert sd["param_groups"][0]["weight_decay"] == 0.02 and sd["param_groups"][0]["decoupled_weight_decay"] is True
    topt = torch.optim.AdamW(twin.parameters(), lr=1.0, weight_decay=0.5)
    topt.load_state_dict(sd)                                  # torch validates group sizes and parameter counts
    grp = topt.param_groups[0]
    assert grp["lr"] == 3e-4 and grp["weight_decay"] == 0.02 and grp["decoupled_weight_decay"] is True
    for n, p in twin.named_parameters():
        o = fopt.flat.offsets[n]
        assert float(topt.state[p]["step"]) == 7.0 and torch.equal(topt.state[p]["exp_avg"].reshape(-1), fopt.exp_avg[o:o + p.numel()]), n
    # and back: torch's own state dict into a fresh FusedAdam
    back = maavss_amd.FusedAdam(maavss_amd.AV_Fusion_Model_Frames(*SHAPES), lr=1.0)
    assert not back.extended
    back.load_state_dict(topt.state_dict())
    assert back.weight_decay == 0.02 and back.extended and back.lr == 3e-4 and back.step_count == 7
    for n in fopt.flat.names:                                # tensor by tensor: the alignment gaps between them are nobody's state
        o, k = fopt.flat.offsets[n], trainer._numel(fopt.flat.shapes[n])
        assert torch.equal(back.exp_avg[o:o + k], fopt.exp_avg[o:o + k]) and torch.equal(back.exp_avg_sq[o:o + k], fopt.exp_avg_sq[o:o + k]), n
    # plain Adam's L2 decay is another update: refused
    l2 = torch.optim.Adam(twin.parameters(), lr=1.0, weight_decay=0.1).state_dict()
    with pytest.raises(ValueError, match="L2"):
        back.load_state_dict(l2)


def test_ema_state_dict_and_checkpoint_keys(model, tmp_path):
    opt = maavss_amd.FusedAdam(model, lr=1e-3, ema_decay=0.99, ema_warmup=True)
    flat = opt.flat
    assert torch.equal(opt.ema, flat.params) and opt.ema.data_ptr() != flat.params.data_ptr()
    assert [opt._next_ema_decay()] == [0.1]
    opt.ema.add_(1.0)
    opt.ema_updates = 4
    esd = opt.ema_state_dict()
    msd = model.state_dict()
    assert set(esd) - {"num_updates"} == set(flat.names) <= set(msd) and int(esd["num_updates"]) == 4
    for n in flat.names:
        assert esd[n].shape == msd[n].shape and torch.equal(esd[n], msd[n] + 1.0), n
    sched = maavss_amd.LRSchedule(1e-3, warmup_steps=5)
    sched.next_lr()
    # written only when given
    maavss_amd.save_checkpoint(msd, opt.state_dict(), 1, 0.5, "plain", str(tmp_path))
    assert sorted(torch.load(os.path.join(tmp_path, "plain.pt"), weights_only=True)) == ["epoch", "loss", "model_state_dict", "optimizer_state_dict"]
    maavss_amd.save_checkpoint(msd, opt.state_dict(), 2, 0.4, "full", str(tmp_path), ema_dict=esd, schedule_dict=sched.state_dict())
    cp = torch.load(os.path.join(tmp_path, "full.pt"), weights_only=True)
    assert sorted(cp) == ["ema_state_dict", "epoch", "loss", "lr_schedule_state_dict", "model_state_dict", "optimizer_state_dict"]
    fresh = maavss_amd.AV_Fusion_Model_Frames(*SHAPES)
    fopt = maavss_amd.FusedAdam(fresh, lr=1e-3, ema_decay=0.99)
    fs = maavss_amd.LRSchedule(1.0)
    maavss_amd.load_checkpoint(fresh, fopt, str(tmp_path), auto=False, path=os.path.join(tmp_path, "full.pt"), load_ema=True, schedule=fs)
    for n in flat.names:
        o, k = flat.offsets[n], trainer._numel(flat.shapes[n])
        assert torch.equal(fopt.ema[o:o + k], opt.ema[o:o + k]), n
    assert fopt.ema_updates == 4 and fs.state_dict() == sched.state_dict()
    assert torch.equal(fopt.flat.params, flat.params)
    # a file without the keys: reported, not raised; nothing changes
    before = fopt.ema.clone()
    maavss_amd.load_checkpoint(fresh, fopt, str(tmp_path), auto=False, path=os.path.join(tmp_path, "plain.pt"), load_ema=True, schedule=fs)
    assert torch.equal(fopt.ema, before) and fs.state_dict() == sched.state_dict()
    opt.ema_reset()
    assert torch.equal(opt.ema, flat.params) and opt.ema_updates == 0
    with pytest.raises(_lib.MaavssError, match="no weight average"):
        maavss_amd.FusedAdam(flat, lr=1e-3).ema_weights().__enter__()


# ---- the entry points ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_in_the_header_and_the_library_and_the_abi_is_401():
    protos = _lib.parse_header()
    lib = _lib.lib()
    for name in ("maavss_adamw_ema_step", "maavss_swap_f32"):
        assert name in protos and hasattr(lib.cdll, name)
    assert [a for _, a in protos["maavss_adamw_ema_step"][1]] == [
        "p", "g", "m", "v", "ema", "n", "lr", "beta1", "beta2", "eps", "step", "grad_scale", "scale_dev", "norm_dev", "skip_nonfinite",
        "skipped", "count_skip", "host_seg_end", "host_seg_wd", "n_seg", "ema_decay", "stream"]
    assert _lib.header_abi_version() == 402 == lib.cdll.maavss_version()
    text = open(_lib.HEADER).read()
    block = text[text.index("EXTENSION: AdamW decay"):text.index("int maavss_adamw_ema_step(")]
    assert "NOT in the reference" in block and "GradScaler" in block


def _step_args(**over):
    a = dict(p=256, g=256, m=256, v=256, ema=None, n=8, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step=1, gs=1.0, scale=None, norm=None, skip=0,
             skipped=None, count=0, ends=[8], wd=[0.0], n_seg=None, d=0.0)
    a.update(over)
    ends = (ctypes.c_int64 * max(len(a["ends"]), 1))(*a["ends"]) if a["ends"] is not None else None
    wd = (ctypes.c_float * max(len(a["wd"]), 1))(*a["wd"]) if a["wd"] is not None else None
    n_seg = a["n_seg"] if a["n_seg"] is not None else (1 if a["ends"] is None else len(a["ends"]))
    return (ends, wd), (a["p"], a["g"], a["m"], a["v"], a["ema"], a["n"], a["lr"], a["b1"], a["b2"], a["eps"], a["step"], a["gs"], a["scale"],
                        a["norm"], a["skip"], a["skipped"], a["count"], None if ends is None else ctypes.addressof(ends),
                        None if wd is None else ctypes.addressof(wd), n_seg, a["d"], None)


@pytest.mark.parametrize("over,match", [
    (dict(p=None), "adamw_ema_step: bad arguments"),
    (dict(g=None), "adamw_ema_step: bad arguments"),
    (dict(m=None), "adamw_ema_step: bad arguments"),
    (dict(v=None), "adamw_ema_step: bad arguments"),
    (dict(n=0), "adamw_ema_step: bad arguments"),
    (dict(step=0), "adamw_ema_step: bad arguments"),                       # step counts from 1
    (dict(g=260), "16-byte aligned"),
    (dict(ema=264, d=0.5), "16-byte aligned"),
    (dict(scale=258), "scale_dev must be 4-byte aligned"),
    (dict(skip=1), "skip_nonfinite needs norm_dev"),
    (dict(skip=1, norm=258), "norm_dev must be 4-byte aligned"),
    (dict(count=1), "count_skip needs skip_nonfinite and skipped"),
    (dict(skip=1, norm=256, count=1), "count_skip needs skip_nonfinite and skipped"),
    (dict(skip=1, norm=256, count=1, skipped=258), "skipped must be 4-byte aligned"),
    (dict(ema=256, d=1.0), r"ema_decay must be in \[0, 1\)"),
    (dict(ema=256, d=-0.5), r"ema_decay must be in \[0, 1\)"),
    (dict(ema=256, d=float("nan")), r"ema_decay must be in \[0, 1\)"),
    (dict(ends=None), "decay table is missing"),
    (dict(wd=None), "decay table is missing"),
    (dict(n_seg=0), "n_seg must be in 1..64"),
    (dict(ends=list(range(4, 4 * 66, 4)), wd=[0.0] * 65, n=256), "n_seg must be in 1..64"),
    (dict(ends=[8, 8], wd=[0.0, 0.0]), "must ascend"),
    (dict(ends=[0, 8], wd=[0.0, 0.0]), "must ascend"),
    (dict(ends=[6, 8], wd=[0.0, 0.0]), "multiples of 4"),
    (dict(ends=[4], wd=[0.0]), "before n = 8"),
    (dict(wd=[-0.1]), "finite and >= 0"),
    (dict(wd=[float("inf")]), "finite and >= 0"),
])
def test_adamw_ema_step_refuses_bad_arguments_before_any_launch(over, match):
    keep, args = _step_args(**over)
    with pytest.raises(_lib.MaavssError, match=match):
        _lib.call("maavss_adamw_ema_step", *args)
    del keep


def test_swap_f32_refuses_bad_arguments_before_any_launch():
    for args, match in (((None, 256, 8, None), "swap_f32: bad arguments"), ((256, None, 8, None), "swap_f32: bad arguments"),
                        ((256, 512, 0, None), "swap_f32: bad arguments"), ((256, 516, 8, None), "16-byte aligned"),
                        ((256, 272, 8, None), "overlap"), ((272, 256, 5, None), "overlap"), ((256, 256, 4, None), "overlap")):
        with pytest.raises(_lib.MaavssError, match=match):
            _lib.call("maavss_swap_f32", *args)
