"""CPU-only part of the gradient statistics (maavss_amd/tensor_stats.py, csrc/tensor_stats.hip): the float64 twin against torch, the
chunk planner, the argument checks of the new entry points (every call below fails before any launch) and ModelWatch's bookkeeping."""
import math

import numpy as np
import pytest
import torch

import stats_twin as tw
from maavss_amd import _lib

CH = 16384        # the twin's table is built for the library's chunk length; test_chunk_length_is_the_librarys pins the two together


@pytest.fixture(scope="module")
def table():
    names, offsets, lens, buf = tw.make_cases(CH)
    return names, offsets, lens, buf


def _seg(table, i):
    _, offsets, lens, buf = table
    return buf[offsets[i]:offsets[i] + lens[i]]


def test_chunk_length_is_the_librarys():
    import maavss_amd.tensor_stats as ts
    assert ts.chunk_len() == CH == _lib.query("maavss_tensor_stats_chunk")


def test_case_table_is_what_the_issue_lists(table):
    names, offsets, lens, buf = table
    assert lens == [1, 3, 4, 5, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 7, 16]
    assert all(o % 64 == 0 for o in offsets)
    fin = buf[np.isfinite(buf)]
    assert not np.any((fin != 0) & (np.abs(fin) < np.finfo(np.float32).tiny)), "no denormal inputs"
    st = [tw.seg_stats(_seg(table, i)) for i in range(len(lens))]
    assert st[2]["min"] == st[2]["max"] == 0 and st[3]["min"] == st[3]["max"] != 0          # all zeros; one repeated value
    assert np.all(_seg(table, 4) == np.round(_seg(table, 4))) and np.all(_seg(table, 9) == np.round(_seg(table, 9)))
    assert st[6]["nan"] == 1 and st[7]["posinf"] == 2 and st[7]["neginf"] == 1
    assert st[1]["nan"] + st[1]["posinf"] + st[1]["neginf"] == lens[1] and math.isnan(st[1]["min"])


@pytest.mark.parametrize("bins", tw.BINS)
def test_twin_histogram_equals_torch_histc(table, bins):
    for i, finite in enumerate(tw.FINITE):
        if not finite:
            continue
        x = _seg(table, i)
        want = torch.histc(torch.from_numpy(x.copy()), bins=bins).numpy().astype(np.int64)
        got = tw.hist_f32(x, bins)
        assert got.sum() == x.size
        np.testing.assert_array_equal(got, want, err_msg=f"segment {i} ({tw.KINDS[i]}), {bins} bins")


def test_twin_histogram_leaves_nonfinite_elements_out(table):
    for i in (1, 6, 7):
        x = _seg(table, i)
        fin = x[np.isfinite(x)]
        got = tw.hist_f32(x, 64)
        assert got.sum() == fin.size
        if fin.size:
            np.testing.assert_array_equal(got, torch.histc(torch.from_numpy(fin.copy()), bins=64).numpy().astype(np.int64))


def test_twin_norm_equals_vector_norm_in_float64(table):
    for i, finite in enumerate(tw.FINITE):
        if finite:
            x = torch.from_numpy(_seg(table, i).copy()).double()
            want = torch.linalg.vector_norm(x).item()
            assert abs(math.sqrt(tw.seg_stats(x.numpy())["sumsq"]) - want) <= 4 * tw.U53 * want * max(1, math.log2(x.numel() + 1))


@pytest.mark.parametrize("factor,grad_scale", [(0.5, 1.0), (2.0, 1.0), (0.5, 0.5)])
def test_twin_clip_equals_clip_grad_norm_on_float64_copies(table, factor, grad_scale):
    sel = [i for i, f in enumerate(tw.FINITE) if f]
    stats = [tw.seg_stats(_seg(table, i)) for i in sel]
    _, norm, _ = tw.clip(stats, None, grad_scale)
    max_norm = factor * norm
    _, norm2, scale = tw.clip(stats, max_norm, grad_scale)
    ps = [torch.nn.Parameter(torch.zeros(_seg(table, i).size, dtype=torch.float64)) for i in sel]
    for p, i in zip(ps, sel):
        p.grad = torch.from_numpy(_seg(table, i).copy()).double() * grad_scale
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm).item()
    assert abs(norm2 - total) <= 1e-13 * total
    if factor > 1:
        assert scale == grad_scale
    for p, i in zip(ps, sel):
        want = p.grad.numpy()
        got = _seg(table, i).astype(np.float64) * scale
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)


def test_twin_clip_with_nonfinite_gradients(table):
    st = [tw.seg_stats(_seg(table, i)) for i in range(len(tw.KINDS))]
    _, norm, scale = tw.clip([st[5], st[6]], 1.0)
    assert math.isnan(norm) and math.isnan(scale)
    _, norm, scale = tw.clip([st[5], st[7]], 1.0)
    assert norm == float("inf") and scale == 0.0
    # torch agrees (error_if_nonfinite=False)
    for i, check in ((6, math.isnan), (7, lambda c: c == 0.0)):
        p = torch.nn.Parameter(torch.zeros(_seg(table, i).size, dtype=torch.float64))
        p.grad = torch.from_numpy(_seg(table, i).copy()).double()
        g0 = p.grad[0].item()
        torch.nn.utils.clip_grad_norm_([p], 1.0)
        assert check(p.grad[0].item() / g0)


def test_plan_chunks_covers_every_element_once_in_buffer_order(table):
    import maavss_amd
    names, offsets, lens, buf = table
    for ch in (1, 7, 64, CH):
        offs, ks = (offsets, lens) if ch >= 64 else (offsets[:7], lens[:7])
        rows = maavss_amd.plan_chunks(offs, ks, ch)
        seen = np.zeros(buf.size, dtype=np.int32)
        prev_end = 0
        for sg, a, k in rows:
            assert 1 <= k <= ch
            assert offs[sg] <= a and a + k <= offs[sg] + ks[sg], "a chunk crosses its segment's boundary"
            assert a >= prev_end, "table order is buffer order"
            prev_end = a + k
            seen[a:a + k] += 1
        inside = np.zeros(buf.size, dtype=np.int32)
        for o, k in zip(offs, ks):
            inside[o:o + k] = 1
        np.testing.assert_array_equal(seen, inside)
        assert len(rows) == sum((k + ch - 1) // ch for k in ks)
        assert [r[0] for r in rows] == sorted(r[0] for r in rows)
    assert maavss_amd.plan_chunks([0, 64], [0, 5], 4) == [(1, 64, 4), (1, 68, 1)]        # an empty tensor has no chunk
    with pytest.raises(ValueError):
        maavss_amd.plan_chunks([64, 0], [5, 5], 4)


def test_workspace_size_is_the_layout_of_the_header():
    def r256(b):
        return (b + 255) // 256 * 256
    for n_chunks, n_seg, bins in ((0, 1, 1), (1, 1, 64), (17, 12, 1024), (4500, 170, 64), (1 << 20, 3, 1)):
        assert _lib.query("maavss_tensor_stats_ws_bytes", n_chunks, n_seg, bins) == r256(32 * n_chunks) + r256(8 * n_seg)
    for bad in ((4, 3, 0), (4, 3, 1025), (4, 0, 64), (-1, 3, 64)):
        assert _lib.query("maavss_tensor_stats_ws_bytes", *bad) == 0


def _stats_args(**over):
    """A call of maavss_tensor_stats whose every argument passes (fake, aligned device addresses: never launched in these tests
    because one override makes a check fail)."""
    off = np.array([0, 64], dtype=np.int64)
    num = np.array([40, CH + 1], dtype=np.int64)
    a = dict(buf=4096, n=64 + CH + 1, chunks=8192, n_chunks=3, seg_first=4096, off=off, num=num, n_segments=2, mask=None, sumsq=4096,
             mn=4096, mx=4096, nonfinite=4096, hist=4096, bins=64, max_norm=-1.0, grad_scale=1.0, total=None, norm=None, scale=None,
             ws=4096, ws_bytes=1 << 20, stream=None)
    a.update(over)
    keep = (a["off"], a["num"])
    return keep, (a["buf"], a["n"], a["chunks"], a["n_chunks"], a["seg_first"], a["off"].ctypes.data if a["off"] is not None else None,
                  a["num"].ctypes.data if a["num"] is not None else None, a["n_segments"], a["mask"], a["sumsq"], a["mn"], a["mx"],
                  a["nonfinite"], a["hist"], a["bins"], a["max_norm"], a["grad_scale"], a["total"], a["norm"], a["scale"], a["ws"],
                  a["ws_bytes"], a["stream"])


@pytest.mark.parametrize("over,match", [
    (dict(buf=None), "null pointer"),
    (dict(chunks=None), "null pointer"),
    (dict(off=None), "null pointer"),
    (dict(sumsq=None), "null pointer"),
    (dict(ws=None), "null pointer"),
    (dict(max_norm=1.0), "null pointer"),                       # a clip without its outputs
    (dict(bins=0), "bins must be in 1..1024"),
    (dict(bins=1025), "bins must be in 1..1024"),
    (dict(buf=4100), "16-byte aligned"),
    (dict(ws=4100), "8-byte aligned"),
    (dict(num=np.array([40, 1 << 31], dtype=np.int64), n=(1 << 31) + 64), "2\\^31 or more are refused"),
    (dict(n=100), "leaves the buffer"),
    (dict(n_chunks=2), "chunks given"),
    (dict(ws_bytes=64), "workspace of 64 bytes"),
])
def test_tensor_stats_refuses_bad_arguments_before_any_launch(over, match):
    keep, args = _stats_args(**over)
    with pytest.raises(_lib.MaavssError, match=match):
        _lib.call("maavss_tensor_stats", *args)
    del keep


def test_adam_step_dscale_refuses_bad_arguments_before_any_launch():
    with pytest.raises(_lib.MaavssError, match="adam_step_dscale: bad arguments"):
        _lib.call("maavss_adam_step_dscale", 256, 256, 256, 256, 8, 1e-3, 0.9, 0.999, 1e-8, 1, None, None)      # no device scale
    with pytest.raises(_lib.MaavssError, match="adam_step_dscale: bad arguments"):
        _lib.call("maavss_adam_step_dscale", None, 256, 256, 256, 8, 1e-3, 0.9, 0.999, 1e-8, 1, 256, None)
    with pytest.raises(_lib.MaavssError, match="adam_step_dscale: bad arguments"):
        _lib.call("maavss_adam_step_dscale", 256, 256, 256, 256, 8, 1e-3, 0.9, 0.999, 1e-8, 0, 256, None)        # step counts from 1
    with pytest.raises(_lib.MaavssError, match="16-byte aligned"):
        _lib.call("maavss_adam_step_dscale", 256, 260, 256, 256, 8, 1e-3, 0.9, 0.999, 1e-8, 1, 256, None)
    with pytest.raises(_lib.MaavssError, match="4-byte aligned"):
        _lib.call("maavss_adam_step_dscale", 256, 256, 256, 256, 8, 1e-3, 0.9, 0.999, 1e-8, 1, 258, None)


class _FakeStats:
    """What ModelWatch needs of a TensorStats: run() and to_host()."""
    made = []

    def __init__(self, flat, bins=64):
        self.flat, self.bins, self.runs = flat, bins, []
        _FakeStats.made.append(self)

    def run(self, buffer, hist=True):
        self.runs.append((buffer, hist))

    def to_host(self):
        out = {}
        for i, n in enumerate(self.flat.names):
            out[n] = dict(norm=1.0, min=-1.0, max=1.0, nan=0, posinf=0, neginf=0, counts=np.full(self.bins, i, dtype=np.int32),
                          edges=np.linspace(-1, 1, self.bins + 1))
        out["b"].update(nan=2, neginf=1)
        out["c"].update(min=float("nan"), max=float("nan"), nan=5, counts=np.zeros(self.bins, dtype=np.int32))
        return out


def test_model_watch_period_and_key_naming():
    import maavss_amd
    flat = tw.fake_flat(["a", "b", "c"], [0, 64, 128], [3, 4, 5], 192, params="PARAMS", grads="GRADS")
    _FakeStats.made = []
    holder = type("Opt", (), {"flat": flat})()                 # a TrainStep / FusedAdam: anything with .flat
    watch = maavss_amd.ModelWatch(holder, log_freq=3, bins=8, log="all", stats_cls=_FakeStats)
    got = [watch.after_step() for _ in range(7)]
    assert [g is not None for g in got] == [False, False, True, False, False, True, False]
    logs = got[2]
    assert sorted(logs) == ["gradients/a", "gradients/b", "nonfinite/gradients/b", "nonfinite/gradients/c", "nonfinite/parameters/b",
                            "nonfinite/parameters/c", "parameters/a", "parameters/b"]
    counts, edges = logs["gradients/b"]
    assert isinstance(counts, np.ndarray) and isinstance(edges, np.ndarray) and counts.shape == (8,) and edges.shape == (9,)
    assert logs["nonfinite/gradients/b"] == {"nan": 2, "posinf": 0, "neginf": 1}
    g, p = _FakeStats.made
    assert g.runs == [("GRADS", True)] * 2 and p.runs == [("PARAMS", True)] * 2          # statistics only in the logging steps
    only = maavss_amd.ModelWatch(flat, log_freq=1, log="gradients", stats_cls=_FakeStats)
    assert all(k.split("/")[0] in ("gradients", "nonfinite") for k in only.after_step())
    with pytest.raises(ValueError):
        maavss_amd.ModelWatch(flat, log="everything", stats_cls=_FakeStats)
    with pytest.raises(ValueError):
        maavss_amd.ModelWatch(flat, log_freq=0, stats_cls=_FakeStats)


def test_new_names_are_exported_and_clipping_is_off_by_default():
    import inspect
    import maavss_amd
    for name in ("TensorStats", "ModelWatch", "plan_chunks"):
        assert hasattr(maavss_amd, name)
    assert inspect.signature(maavss_amd.FusedAdam.__init__).parameters["max_grad_norm"].default is None
    assert inspect.signature(maavss_amd.TrainStep.__init__).parameters["max_grad_norm"].default is None
    flat = maavss_amd.trainer.FlatParams.__new__(maavss_amd.trainer.FlatParams)       # the layout alone: no model behind it
    flat.__dict__.update(vars(tw.fake_flat(["a"], [0], [4], 64, params=torch.zeros(64))))
    with pytest.raises(ValueError):
        maavss_amd.FusedAdam(flat, max_grad_norm=-1.0)
    assert maavss_amd.FusedAdam(flat).max_grad_norm is None
