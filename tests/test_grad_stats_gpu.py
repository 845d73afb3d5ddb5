"""csrc/tensor_stats.hip, maavss_adam_step_dscale, gradient-norm clipping and ModelWatch on the GPU against the float64 twin
(tests/stats_twin.py, where the bounds are derived).

Synthetic layout (tests 1-3): the twelve segments of stats_twin.make_cases -- lengths 1, 3, 4, 5, 63, 64, 65, CH - 1, CH, CH + 1,
2 CH + 7, 16 at 64-aligned offsets: the scalar tail (length % 4), a single workgroup, a chunk that is exactly full, one element past
it, three chunks; all zeros, one repeated value (lo == hi), integers on the bin edges, a NaN, infinities, nothing finite."""
import math
import os

import numpy as np
import pytest
import torch

import maavss_amd
import stats_twin as tw
from maavss_amd import ops
from maavss_amd.tensor_stats import TensorStats, chunk_len

pytestmark = pytest.mark.gpu

FINITE_IDX = [i for i, f in enumerate(tw.FINITE) if f]


@pytest.fixture(scope="module")
def case():
    names, offsets, lens, buf = tw.make_cases(chunk_len())
    dev = torch.from_numpy(buf).cuda()
    flat = tw.fake_flat(names, offsets, lens, buf.size, params=dev, grads=dev)
    stats = [tw.seg_stats(buf[o:o + k]) for o, k in zip(offsets, lens)]
    return dict(names=names, offsets=offsets, lens=lens, buf=buf, dev=dev, flat=flat, stats=stats)


def _host(out):
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy().copy()) for k, v in out.items()}


@pytest.mark.parametrize("bins", tw.BINS)
def test_per_segment_statistics_and_histogram_equal_the_twin(case, bins):
    ts = TensorStats(case["flat"], bins=bins)
    got = _host(ts.run(case["dev"], hist=True))
    for i, (st, n) in enumerate(zip(case["stats"], case["lens"])):
        err, bound = abs(got["sumsq"][i] - st["sumsq"]), (n - 1) * tw.U53 * st["sumsq"]
        print(f"segment {i:2d} ({tw.KINDS[i]:13s}) n {n:6d} sumsq {got['sumsq'][i]:.17g} |err| {err:.3g} bound {bound:.3g}")
        assert err <= bound, (i, got["sumsq"][i], st["sumsq"])
        if math.isnan(st["min"]):
            assert math.isnan(got["min"][i]) and math.isnan(got["max"][i])
        else:
            assert got["min"][i] == st["min"] and got["max"][i] == st["max"], (i, got["min"][i], st["min"], got["max"][i], st["max"])
        assert tuple(got["nonfinite"][i]) == (st["nan"], st["posinf"], st["neginf"]), i
        x = case["buf"][case["offsets"][i]:case["offsets"][i] + n]
        np.testing.assert_array_equal(got["hist"][i].astype(np.int64), tw.hist_f32(x, bins), err_msg=f"segment {i} ({tw.KINDS[i]}), {bins} bins")
    host = ts.to_host()
    name = case["names"][8]
    assert host[name]["counts"].sum() == case["lens"][8] and host[name]["edges"].shape == (bins + 1,)
    assert host[name]["norm"] == math.sqrt(got["sumsq"][8]) and host[case["names"][6]]["nan"] == 1


def test_runs_are_bit_identical_and_a_names_subset_changes_only_norm_and_scale(case):
    ts = TensorStats(case["flat"], bins=64)
    names = [case["names"][i] for i in FINITE_IDX]
    ts.run(case["dev"], names=names, hist=True, max_norm=1.0)
    torch.cuda.synchronize()
    first = ts._out.clone()
    ts.run(case["dev"], names=names, hist=True, max_norm=1.0)
    torch.cuda.synchronize()
    assert torch.equal(first, ts._out), "two runs differ"
    full = _host(ts.run(case["dev"], names=names, hist=True, max_norm=1.0))
    sub_idx = [0, 4, 8, 10]
    sub = _host(ts.run(case["dev"], names=[case["names"][i] for i in sub_idx], hist=True, max_norm=1.0))
    for k in ("sumsq", "min", "max", "nonfinite", "hist"):
        assert full[k].tobytes() == sub[k].tobytes(), k
    _, norm, scale = tw.clip([case["stats"][i] for i in sub_idx], 1.0)
    _, norm_full, _ = tw.clip([case["stats"][i] for i in FINITE_IDX], 1.0)
    assert abs(norm - norm_full) > 1e-3 * norm_full                       # the subset has another norm: the check below sees the mask
    assert abs(sub["norm"][0] - norm) <= tw.U23 * norm and abs(sub["scale"][0] - scale) <= tw.U23 * scale
    assert abs(full["norm"][0] - norm_full) <= tw.U23 * norm_full


@pytest.mark.parametrize("factor,grad_scale", [(0.5, 1.0), (2.0, 1.0), (0.5, 0.5), (2.0, 0.5)])
def test_norm_and_scale_equal_the_twin(case, factor, grad_scale):
    ts = TensorStats(case["flat"], bins=1)
    sel = [case["stats"][i] for i in FINITE_IDX]
    names = [case["names"][i] for i in FINITE_IDX]
    _, norm0, _ = tw.clip(sel, None, grad_scale)
    max_norm = factor * norm0
    _, norm, scale = tw.clip(sel, max_norm, grad_scale)
    got = _host(ts.run(case["dev"], names=names, hist=False, max_norm=max_norm, grad_scale=grad_scale))
    print(f"norm {got['norm'][0]!r} twin {norm!r}; scale {got['scale'][0]!r} twin {scale!r}")
    assert got["hist"] is None
    assert abs(got["norm"][0] - norm) <= tw.U23 * norm
    assert abs(got["scale"][0] - scale) <= tw.U23 * scale
    if factor > 1:
        assert got["scale"][0] == np.float32(grad_scale)                  # no clipping: the scale is grad_scale exactly
    else:
        assert got["scale"][0] < np.float32(grad_scale)


def test_nonfinite_gradients_give_nan_or_inf_and_zero(case):
    ts = TensorStats(case["flat"], bins=1)
    n = case["names"]
    got = _host(ts.run(case["dev"], names=[n[5], n[6]], hist=False, max_norm=1.0))          # a NaN
    assert math.isnan(got["norm"][0]) and math.isnan(got["scale"][0])
    got = _host(ts.run(case["dev"], names=[n[5], n[7]], hist=False, max_norm=1.0))          # +inf and -inf, no NaN
    assert got["norm"][0] == np.inf and got["scale"][0] == 0.0
    got = _host(ts.run(case["dev"], names=None, hist=False, max_norm=1.0))                  # everything: a NaN wins over the infinities
    assert math.isnan(got["norm"][0]) and math.isnan(got["scale"][0])
    got = _host(ts.run(case["dev"], names=[n[5]], hist=False, max_norm=1.0))                # and the finite ones are untouched by them
    _, norm, scale = tw.clip([case["stats"][5]], 1.0)
    assert abs(got["norm"][0] - norm) <= tw.U23 * norm and abs(got["scale"][0] - scale) <= tw.U23 * scale


def test_adam_with_the_device_scale_equals_adam_with_the_host_scale():
    n = 4 * 1031 + 3                                   # five workgroups of float4 lanes and a three-element scalar tail
    g = torch.Generator().manual_seed(5)
    p0, grad = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    scale = torch.tensor([0.37], dtype=torch.float32).cuda()
    scale_host = scale.item()
    state = []
    for dev_scale in (True, False):
        p, m, v, gr = p0.cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda(), grad.cuda()
        for step in (1, 2, 3):
            if dev_scale:
                ops.adam_step_dscale(p, gr, m, v, 1e-3, step, scale)
            else:
                ops.adam_step(p, gr, m, v, 1e-3, step, grad_scale=scale_host)
        torch.cuda.synchronize()
        state.append((p, m, v))
    for a, b in zip(*state):
        assert torch.equal(a, b)
    assert not torch.equal(state[0][0], p0.cuda())


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


def _twin_clip(step, max_norm, grad_scale=1.0):
    """the twin's (norm, scale) over the parameters the step updates, from the gradients copied to the host"""
    flat = step.flat
    g = flat.grads.cpu().numpy()
    names = [n for n in flat.names if n in flat.touched and flat.tensors[n].requires_grad]
    stats = [tw.seg_stats(g[flat.offsets[n]:flat.offsets[n] + flat.tensors[n].numel()], exact=False) for n in names]
    _, norm, scale = tw.clip(stats, max_norm, grad_scale)
    return names, norm, scale


def _same_state(a, b):
    return torch.equal(a.flat.params, b.flat.params) and torch.equal(a.opt.exp_avg, b.opt.exp_avg) and torch.equal(a.opt.exp_avg_sq, b.opt.exp_avg_sq)


def test_trainstep_clipping_and_model_watch_on_the_small_model(golden_dir):
    """TrainStep(max_grad_norm) on the avse_S shape against an unclipped TrainStep whose Adam is handed the same gradient bytes and
    the reported scale on the host; frozen encoders stay out of the norm; ModelWatch's histograms equal torch.histc of the host copies."""
    m, (mc, mu), (x_a, x_v, y_a, y_v) = _seeded_models(golden_dir, 2)
    plain = maavss_amd.TrainStep(mu, lr=m["lr"], loss_coeff=m["loss_coeff"])
    plain(x_a, x_v, y_a, y_v, optimizer_step=False)
    _, norm1, _ = _twin_clip(plain, None)
    assert norm1 > 0

    # A: max_grad_norm = half the norm
    c = 0.5 * norm1
    clipped = maavss_amd.TrainStep(mc, lr=m["lr"], loss_coeff=m["loss_coeff"], max_grad_norm=c)
    clipped(x_a, x_v, y_a, y_v)
    names, norm, scale = _twin_clip(clipped, c)                    # flat.grads still holds the unclipped gradient
    got_norm, got_scale = clipped.opt.grad_norm.item(), clipped.opt.clip_scale.item()
    print(f"A: norm {got_norm!r} twin {norm!r}; scale {got_scale!r} twin {scale!r}; {len(names)} tensors")
    assert abs(got_norm - norm) <= tw.U23 * norm and abs(got_scale - scale) <= tw.U23 * scale
    assert 0.49 < got_scale < 0.51
    plain.flat.grads.copy_(clipped.flat.grads)                     # the same gradient bytes, whatever the backward's summation order
    plain.opt.step(grad_scale=got_scale)
    assert _same_state(clipped, plain)
    assert clipped.opt.steps == plain.opt.steps

    # B: max_grad_norm = twice the norm: the step is the unclipped step, bit for bit
    plain(x_a, x_v, y_a, y_v, optimizer_step=False)
    _, norm2, _ = _twin_clip(plain, None)
    clipped.opt.max_grad_norm = 2.0 * norm2
    clipped(x_a, x_v, y_a, y_v)
    assert clipped.opt.clip_scale.item() == 1.0
    plain.flat.grads.copy_(clipped.flat.grads)
    plain.opt.step()
    assert _same_state(clipped, plain)

    # frozen encoders: their (stale) gradients are left out of the norm
    mc.toggle_enc_grads(False)
    clipped(x_a, x_v, y_a, y_v)
    names, norm, _ = _twin_clip(clipped, clipped.opt.max_grad_norm)
    assert names and not any(n.startswith(("visual_encoder.", "stft_encoder.")) for n in names)
    g = clipped.flat.grads.cpu().numpy()
    everything = math.sqrt(float((g.astype(np.float64) ** 2).sum()))
    got_norm = clipped.opt.grad_norm.item()
    print(f"frozen: norm {got_norm!r} twin {norm!r}; over the whole buffer {everything!r}")
    assert everything - norm > 16 * tw.U23 * norm, "the frozen encoders' stale gradients must be able to show"
    assert abs(got_norm - norm) <= tw.U23 * norm

    # ModelWatch: one BatchNorm bias, fc2.weight, one conv weight
    watch = maavss_amd.ModelWatch(clipped, log_freq=1, bins=64)
    logs = watch.after_step()
    p = clipped.flat.params.cpu()
    gt = torch.from_numpy(g)
    for name in ("visual_encoder.1.bias", "fc2.weight", "visual_encoder.4.weight"):
        o, k = clipped.flat.offsets[name], clipped.flat.tensors[name].numel()
        for kind, host in (("gradients", gt), ("parameters", p)):
            counts, edges = logs[f"{kind}/{name}"]
            x = host[o:o + k]
            np.testing.assert_array_equal(counts.astype(np.int64), torch.histc(x, bins=64).numpy().astype(np.int64), err_msg=f"{kind}/{name}")
            assert edges.shape == (65,) and counts.sum() == k
            if x.min() != x.max():
                assert edges[0] == x.min().item() and edges[-1] == x.max().item()
    assert not any(k.startswith("nonfinite/") for k in logs)
