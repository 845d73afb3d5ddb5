"""CPU-only: the float64 twin of the image-source room responses (tests/room_twin.py) held to its own definition -- closed forms,
an independent brute-force formulation, order independence of the integer sums, row independence -- and the host layer of
maavss_amd.Reverb's room methods: draws, groupings and every refusal, none of which touches a device."""
import json
import math
import os

import numpy as np
import pytest
import torch

import room_twin as tw
from maavss_amd import Reverb, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, MIC, SRC = (4.0, 3.5, 2.5), (1.7, 1.9, 1.2), (2.9, 0.8, 1.4)


def test_six_absorbing_walls_leave_the_direct_path():
    for k in (1, 5, 700):
        res = tw.response(DIMS, MIC, SRC, (0.0,) * 6, k)
        want = np.zeros(k, dtype=np.float32)
        want[0] = 1.0
        assert res.h.tobytes() == want.tobytes() and res.acc[0] == 1 << 40


@pytest.mark.parametrize("wall", range(6))
def test_one_reflecting_wall_is_the_direct_impulse_plus_one_image(wall):
    k, h, r, sr, b = 400, 8, 32, 16000, 0.8
    beta = [0.0] * 6
    beta[wall] = b
    res = tw.response(DIMS, MIC, SRC, beta, k, sr, h, r)
    # the image: the source mirrored in that wall
    axis, far = divmod(wall, 2)
    mirrored = list(SRC)
    mirrored[axis] = 2.0 * DIMS[axis] - SRC[axis] if far else -SRC[axis]
    d0, d1 = math.dist(SRC, MIC), math.dist(mirrored, MIC)
    tau, amp = (d1 - d0) * sr / 343.0, b * d0 / d1
    want = amp * tw.g_direct(np.arange(k) - tau, h)
    want[0] += 1.0
    assert 2 * h < tau < k - h, "the image's kernel stays clear of the direct path and of the last tap in this room"
    bound = tw.lerp_bound(amp, want, h, r, tau_err=2.0 ** -40)
    err = np.abs(res.h.astype(np.float64) - want)
    assert (err <= bound).all(), (wall, float(err.max()), float(bound.min()))
    assert res.h[0] == 1.0 and np.count_nonzero(res.amp) == 2
    assert np.count_nonzero(res.h) <= 1 + 2 * h


def test_the_twin_agrees_with_a_brute_force_float_sum():
    k, h, r, sr = 800, 4, 16, 16000
    for dims, mic, src, beta in ((DIMS, MIC, SRC, tw.SIX), tw.SMALL[:2] + (tw.SMALL[2][0], tw.SMALL[3])):
        table = tw.kernel_table(h, r)
        bounds = tw.lattice_bounds(dims, mic, src, k, h, sr)
        res = tw.response(dims, mic, src, beta, k, sr, h, r, bounds=bounds)
        brute = tw.brute_force(dims, mic, src, beta, k, sr, h, r, table, bounds)
        exact = res.acc.astype(np.float64) * 2.0 ** -40
        err, bound = np.abs(exact - brute), tw.float_sum_bound(res.count, res.abs_sum)
        assert res.n_images > 100 and (err <= bound).all(), (float(err.max()), float(bound[err.argmax()]))
        assert (err[res.count > 0] > 0).any(), "the two formulations are not the same computation"


def test_the_integer_sum_does_not_depend_on_the_order_of_the_images():
    k, h, r, sr = 1000, 8, 32, 16000
    dims, mic, srcs, beta = tw.SMALL
    table = tw.kernel_table(h, r)
    amp, tau, _ = tw.images(dims, mic, srcs[0], beta, k, sr, h)
    acc = tw.taps(amp, tau, k, table, h, r)[0]
    n = amp.shape[0]
    assert n > 1000 and int(tw.taps(amp, tau, k, table, h, r)[1].max()) > 50
    for order in (np.arange(n)[::-1], np.random.default_rng(0).permutation(n), np.random.default_rng(1).permutation(n)):
        assert np.array_equal(tw.taps(amp, tau, k, table, h, r, order=order)[0], acc)
    # a larger lattice box holds the same images that count
    bigger = [b + 2 for b in tw.lattice_bounds(dims, mic, srcs[0], k, h, sr)]
    assert np.array_equal(tw.response(dims, mic, srcs[0], beta, k, sr, h, r, bounds=bigger).acc, acc)


def test_rows_do_not_depend_on_each_other():
    k = 500
    dims, mic, srcs, beta = tw.MID3
    table = tw.table_of([tw.MID3], k)
    moved = [srcs[0], (0.7, 2.6, 1.9), srcs[2]]
    other = tw.table_of([(dims, mic, moved, beta)], k)
    assert other[0].tobytes() == table[0].tobytes() and other[2].tobytes() == table[2].tobytes() and other[1].tobytes() != table[1].tobytes()
    many = tw.table_of([(tw.LARGE[0], tw.LARGE[1], tw.LARGE[2] * 3, tw.LARGE[3]), tw.MID3, (tw.NEAR[0], tw.NEAR[1], tw.NEAR[2] * 3, tw.NEAR[3])], k)
    assert many[3:6].tobytes() == table.tobytes()


def test_integer_delays_occur_in_the_axial_case_and_stay_clean_impulses():
    _, k, h, r, sr, rooms = next(c for c in tw.CASES if c[0] == "axial")
    dims, mic, srcs, beta = rooms[0]
    res = tw.response(dims, mic, srcs[0], beta, k, sr, h, r)
    assert res.integer_tau > 0
    # such an image alone: one wall, the image on a sample -> exactly one tap besides the direct path
    one = tw.response(dims, mic, srcs[0], (0.5, 0, 0, 0, 0, 0), k, sr, h, r)
    assert one.integer_tau == 1 and np.count_nonzero(one.h) == 2


def test_eyring_beta_and_the_decay_it_gives():
    dims = torch.tensor([[5.0, 4.0, 3.0], [8.0, 6.0, 3.5]])
    beta = Reverb.eyring_beta(dims, [0.4, 0.6])
    v, a = 60.0, 2.0 * (20.0 + 12.0 + 15.0)
    assert tuple(beta.shape) == (2, 6) and beta.dtype == torch.float64
    assert abs(float(beta[0, 0]) - math.exp(-0.0805 * v / (a * 0.4))) < 1e-15 and bool((beta[0] == beta[0, 0]).all())
    assert abs(float(beta[1, 3]) - tw.eyring_beta((8.0, 6.0, 3.5), 0.6)) < 1e-15
    assert float(Reverb.eyring_beta([[3.0, 3.0, 3.0]], 1e9)[0, 0]) <= 1.0 and float(Reverb.eyring_beta([[3.0, 3.0, 3.0]], 1e-9)[0, 0]) == 0.0
    with pytest.raises(ValueError, match="finite and positive"):
        Reverb.eyring_beta([[3.0, 3.0, 3.0]], 0.0)
    assert "nominal" in Reverb.eyring_beta.__doc__.lower() and "more slowly than eyring" in " ".join(Reverb.eyring_beta.__doc__.lower().split())
    # T20 of the twin's response: monotone in beta; its ratio to the nominal figure is recorded, not gated (the model's physics)
    sr, h = 8000, 4
    rooms = [((5.0, 4.0, 3.0), (2.0, 1.5, 1.2), (3.5, 3.0, 1.6), 0.30), ((7.0, 5.0, 3.2), (3.0, 2.0, 1.4), (5.5, 3.8, 1.8), 0.50),
             ((3.5, 3.0, 2.5), (1.2, 1.4, 1.1), (2.6, 2.0, 1.5), 0.25)]
    record = []
    for dims, mic, src, nominal in rooms:
        t20 = []
        for scale in (0.6, 1.0):
            b = tw.eyring_beta(dims, nominal * scale)
            t20.append(tw.t20(tw.response(dims, mic, src, (b,) * 6, int(1.5 * nominal * sr), sr, h, 32).h, sr))
        assert all(math.isfinite(t) and t > 0 for t in t20) and t20[0] < t20[1], t20
        record.append(dict(dims=dims, nominal_rt60=nominal, beta=tw.eyring_beta(dims, nominal), t20=round(t20[1], 4), ratio=round(t20[1] / nominal, 4)))
    print("[room_rir] T20 / nominal rt60:", [x["ratio"] for x in record])
    try:                                                      # a record, not a gate: a read-only checkout keeps the committed one
        with open(os.path.join(ROOT, "profiles", "room_rir_decay.json"), "w") as f:
            f.write(json.dumps(dict(check="room_rir_decay", sr=sr, half_width=h, rooms=record)) + "\n")
    except OSError:
        pass


def test_kernel_table_is_the_twin_s_with_exact_nodes():
    for h, r in ((8, 32), (1, 1), (32, 256), (3, 5)):
        t = Reverb.kernel_table(h, r).numpy()
        assert t.shape == (2 * h * r + 1,) and t[h * r] == 1.0 and not t[::r][np.arange(2 * h + 1) != h].any()
        assert np.abs(t - tw.kernel_table(h, r)).max() <= 2.0 ** -50
    for bad in (dict(half_width=0), dict(half_width=33), dict(resolution=0), dict(resolution=257), dict(half_width=8.0)):
        with pytest.raises(ValueError):
            Reverb.kernel_table(**bad)


def test_sample_rooms_draw_order_and_margins():
    rv = Reverb(256, rt60=(0.2, 0.6))
    n, s = 50, 3
    dims, mic, src, rt60 = rv.sample_rooms(n, torch.Generator().manual_seed(3), sources=s, min_distance=1.2)
    assert dims.dtype == mic.dtype == src.dtype == rt60.dtype == torch.float64
    assert tuple(dims.shape) == (n, 3) and tuple(mic.shape) == (n, 3) and tuple(src.shape) == (n, s, 3) and tuple(rt60.shape) == (n,)
    u = torch.rand(n, 7 + 3 * s, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    lo, hi = torch.tensor([3.0, 3.0, 2.4], dtype=torch.float64), torch.tensor([8.0, 8.0, 3.5], dtype=torch.float64)
    assert torch.equal(dims, lo + (hi - lo) * u[:, :3]) and torch.equal(rt60, 0.2 + (0.6 - 0.2) * u[:, 3])
    assert torch.equal(mic, 0.3 + (dims - 0.6) * u[:, 4:7])
    first = 0.3 + (dims - 0.6)[:, None, :] * u[:, 7:].reshape(n, s, 3)
    kept = ((first - mic[:, None, :]) ** 2).sum(2).sqrt() >= 1.2
    assert torch.equal(src[kept], first[kept]) and not bool(kept.all()), "sources far enough keep their first draw; some were redrawn"
    assert bool((((src - mic[:, None, :]) ** 2).sum(2).sqrt() >= 1.2).all())
    for p in (mic, src.reshape(-1, 3)):
        d = dims if p is mic else dims[:, None, :].expand(n, s, 3).reshape(-1, 3)
        assert bool(((p >= 0.3) & (p <= d - 0.3)).all())
    again = rv.sample_rooms(n, torch.Generator().manual_seed(3), sources=s, min_distance=1.2)
    assert all(torch.equal(a, b) for a, b in zip((dims, mic, src, rt60), again))
    assert torch.equal(rv.sample_rooms(4, torch.Generator().manual_seed(1), rt60=(0.7, 0.7))[3], torch.full((4,), 0.7, dtype=torch.float64))
    for bad, match in ((dict(sources=0), "sources"), (dict(dims=((3.0, 8.0), (3.0, 8.0))), "three"), (dict(wall_margin=1.5), "no space"),
                       (dict(wall_margin=0.0), "wall_margin"), (dict(min_distance=50.0), "too close"), (dict(rt60=(0.0, 1.0)), "rt60"),
                       (dict(dims=((0.0, 8.0), (3.0, 8.0), (2.4, 3.5))), "dims")):
        with pytest.raises(ValueError, match=match):
            rv.sample_rooms(4, torch.Generator().manual_seed(0), **bad)


def _with_table(rv, rows, s):
    """What make_room_rirs / make_rirs leave behind, without a device."""
    rv.rirs, rv.sources_per_room = torch.zeros(rows, rv.rir_len), s
    return rv


def test_sample_room_index_groups_clips_in_rooms():
    rv = _with_table(Reverb(16), 7 * 4, 4)
    for group in (1, 2, 3, 4):
        batch = 12 * group
        idx = rv.sample_room_index(batch, torch.Generator().manual_seed(group), group)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (batch,) and bool(((idx >= 0) & (idx < 28)).all())
        rooms, srcs = (idx // 4).view(-1, group), (idx % 4).view(-1, group)
        assert bool((rooms == rooms[:, :1]).all()), "a group shares one room"
        assert all(len(set(row.tolist())) == group for row in srcs), "and has distinct sources of it"
        g = torch.Generator().manual_seed(group)
        want_room = torch.randint(0, 7, (12,), generator=g)
        want_src = torch.rand(12, 4, generator=g, dtype=torch.float64).argsort(dim=1)[:, :group]
        assert torch.equal(rooms[:, 0].long(), want_room) and torch.equal(srcs.long(), want_src)
    many = rv.sample_room_index(4000, torch.Generator().manual_seed(0), 2)
    assert len(set((many // 4).tolist())) == 7 and len(set(many.tolist())) == 28
    with pytest.raises(ValueError, match="distinct sources"):
        rv.sample_room_index(10, torch.Generator(), 5)
    with pytest.raises(ValueError, match="no multiple"):
        rv.sample_room_index(10, torch.Generator(), 4)
    with pytest.raises(ValueError, match="group"):
        rv.sample_room_index(10, torch.Generator(), 0)
    with pytest.raises(ValueError, match="make_rirs'"):
        _with_table(Reverb(16), 28, None).sample_room_index(4, torch.Generator(), 2)
    with pytest.raises(ValueError, match="no room responses yet"):
        Reverb(16).sample_room_index(4, torch.Generator(), 2)


def test_every_refusal_comes_before_any_device_work():
    rv = Reverb(4096, device="cpu")                           # a device call would raise MaavssError, not ValueError
    dims, mic, src, beta = [list(DIMS)], [list(MIC)], [[list(SRC)]], [[0.5] * 6]

    def refuse(match, **kw):
        args = dict(dims=dims, mic=mic, sources=src, beta=beta)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            rv.make_room_rirs(args.pop("dims"), args.pop("mic"), args.pop("sources"), **args)

    refuse("exactly one", rt60=[0.3])
    refuse("exactly one", beta=None)
    refuse("strictly inside", mic=[[0.0, 1.9, 1.2]])                          # on a wall
    refuse("strictly inside", mic=[[1.7, 3.5, 1.2]])
    refuse("strictly inside", sources=[[[2.9, 0.8, 2.6]]])                     # outside
    refuse("strictly inside", sources=[[[float("nan"), 0.8, 1.4]]])
    refuse("on its microphone", sources=[[list(MIC)]])
    refuse(r"beta must lie in \[0, 1\]", beta=[[0.5, 0.5, 0.5, 1.01, 0.5, 0.5]])
    refuse(r"beta must lie in \[0, 1\]", beta=[[0.5, -0.1, 0.5, 0.5, 0.5, 0.5]])
    refuse(r"beta must lie in \[0, 1\]", beta=[[0.5, float("nan"), 0.5, 0.5, 0.5, 0.5]])
    refuse("finite and positive", dims=[[4.0, 0.0, 2.5]])
    refuse("finite and positive", dims=[[4.0, float("nan"), 2.5]])
    refuse("finite and positive", dims=[[4.0, float("inf"), 2.5]])
    refuse(r"dims must be \[n, 3\]", dims=[4.0, 3.5, 2.5])
    refuse(r"mic must be \[1, 3\]", mic=[list(MIC), list(MIC)])
    refuse(r"sources must be \[1, S, 3\]", sources=[list(SRC)])
    refuse(r"beta must be \[1, 6\]", beta=[[0.5] * 5])
    refuse("rt60 must be a number or hold 1", beta=None, rt60=[0.3, 0.4])
    refuse("finite and positive", beta=None, rt60=[0.0])
    refuse("half_width", half_width=0)
    refuse("half_width", half_width=33)
    refuse("resolution", resolution=257)
    refuse("c must be a positive number", c=0.0)
    refuse("above the cap of 2\\^31", dims=[[0.05, 0.05, 0.05]], mic=[[0.02, 0.02, 0.02]], sources=[[[0.03, 0.03, 0.03]]])
    with pytest.raises(ValueError, match="at most 524288"):
        rv.check_rooms(torch.full((1 << 17, 3), 4.0), torch.full((1 << 17, 3), 1.0), torch.full((1 << 17, 5, 3), 2.0), beta=torch.full((1 << 17, 6), 0.5))
    # what passes reaches the device call, which has no CPU fallback; make_rirs forgets the rooms' grouping
    with pytest.raises(_lib.MaavssError, match="no CPU fallback"):
        rv.make_room_rirs(dims, mic, src, beta=beta)
    assert rv.rirs is None and rv.sources_per_room is None
    geom, bounds, table, s = rv.check_rooms(dims, mic, [[list(SRC), [1.0, 1.0, 1.0]]], rt60=[0.3])
    assert tuple(geom.shape) == (2, 15) and geom.dtype == torch.float64 and tuple(bounds.shape) == (2, 3) and bounds.dtype == torch.int32 and s == 2
    assert geom[0, :6].tolist() == list(DIMS) + list(MIC) and geom[1, 6:9].tolist() == [1.0, 1.0, 1.0] and torch.equal(geom[0, 9:], geom[1, 9:])
    assert bounds[0].tolist() == tw.lattice_bounds(DIMS, MIC, SRC, 4096, 8, 16000)
    assert torch.equal(geom[0, 9:], Reverb.eyring_beta(dims, [0.3])[0])


def test_the_entry_point_checks_the_host_copy_before_any_launch():
    """maavss_room_rir refuses from its arguments and the host tables alone: the device pointers below are never touched."""
    geom = np.array([list(DIMS) + list(MIC) + list(SRC) + [0.5] * 6] * 2, dtype=np.float64)
    bounds = np.array([[3, 3, 4]] * 2, dtype=np.int32)

    def call(match, geom=geom, bounds=bounds, rows=2, h=8, r=32, sr=16000.0, c=343.0, k=300, ld=300, dev=256):
        with pytest.raises(_lib.MaavssError, match=match):
            _lib.call("maavss_room_rir", dev, dev, geom.ctypes.data, bounds.ctypes.data, rows, dev, h, r, sr, c, k, dev, ld, None)

    call("null pointer", dev=None)
    call(r"H = 0 must be in \[1, 32\]", h=0)
    call(r"H = 33 must be in \[1, 32\]", h=33)
    call(r"R = 257 in \[1, 256\]", r=257)
    call(r"K = 32769 must be in", k=32769, ld=40000)
    call("shorter than K", ld=299)
    call("n_rows", rows=0)
    call("n_rows", rows=(1 << 19) + 1)
    call("sr = .* must be positive", sr=0.0)
    call("aligned", dev=260)

    def row1(col, value):
        g = geom.copy()
        g[1, col] = value
        return g

    call("row 1: dimension 1 = 0 must be positive", geom=row1(1, 0.0))
    call("row 1: dimension 2 = nan", geom=row1(2, float("nan")))
    call("row 1: microphone .* strictly inside", geom=row1(3, 4.0))
    call("row 1: .* source 0 must lie strictly inside", geom=row1(6, 0.0))
    call("row 1: .* source nan", geom=row1(8, float("nan")))
    call(r"row 1: beta\[3\] = 1.5", geom=row1(12, 1.5))
    call(r"row 1: beta\[0\] = nan", geom=row1(9, float("nan")))
    on_mic = geom.copy()
    on_mic[0, 6:9] = on_mic[0, 3:6]
    call("row 0: the source lies on the microphone", geom=on_mic)
    neg = bounds.copy()
    neg[1, 2] = -1
    call("row 1: lattice bound -1 on axis 2", bounds=neg)
    big = bounds.copy()
    big[1] = 700
    call(r"row 1: the lattice box \(700, 700, 700\) holds more than 2\^31 images", bounds=big)
