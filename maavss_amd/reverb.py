"""Reverberation: synthetic room impulse responses and their convolution with clips, the third of the augmentations an enhancement
data set rests on (additive noise: STFT; interfering sources: Mixer).  The reference has none (av_dataset.py:217-220 adds white noise
to the STFT coefficients).  The kernels are maavss_rir_synth and maavss_reverb (include/maavss.h, csrc/reverb.hip);
tests/reverb_twin.py restates both definitions in float64.

    h[0] = 1, h[k] = 0 for 1 <= k < predelay, h[k] = s g[k] exp(-ln(1000) k / (rt60 sr)) behind it, g standard normal,
    s such that 10 log10(1 / sum_{k >= predelay} h[k]^2) = drr_db                               (wet = dry + tail)
    wet[b, n] = sum_k h[rir_index[b], k] audio[b, n - k]      in f64, one order of additions, rounded once to f32

The samples in front of a clip are read where they lie: `lead` samples in front of every row of a tensor, or, for the clips of a
ClipBank, the clip's recording back to its first sample (never a neighbouring recording).  A clip convolved from a zero state would
be mostly build-up: a room of rt60 = 0.5 s remembers more than a 0.53 s clip holds.

make_room_rirs fills the same table from geometry instead: the image-source model of a shoebox room with one microphone and S sources
(maavss_room_rir, csrc/room_rir.hip; tests/room_twin.py restates the definition in float64 and the kernel gives its bytes).  Row
room * S + j is source j of a room, so clips that are given rows of one room (sample_room_index) are sources heard in the same walls.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

TARGETS = ("wet", "dry")
FIGURES = ("energy", "edt", "t20", "t30", "c50_db", "drr_db")      # the columns of maavss_rir_measure's output
LEVELS_DB = (-5.0, -10.0, -25.0, -35.0)                            # the Schroeder levels the decay times are read at
# per decay figure: the lower level it is read at, in dB below the start (calibration sizes its scratch table by it)
CALIBRATE = {"t20": 25.0, "t30": 35.0, "edt": 10.0}


def thresholds():
    """The energy thresholds 10^(level / 10) of LEVELS_DB as Python floats: what maavss_rir_measure compares E[j] / E[0] against."""
    return tuple(10.0 ** (level / 10.0) for level in LEVELS_DB)


class Calibration:
    """The search behind make_room_rirs(calibrate=): per room, the uniform wall coefficient whose measured decay time is `target`.
    Host arithmetic only (CPU f64 tensors): the caller measures, `update` moves.  The unknown is x = -1 / ln(beta), which Eyring's
    formula makes the decay time proportional to.  A round: T = the measured time at beta(); a room within tol (relative) of its
    target is done and keeps that coefficient; any other room records its bracket (the largest x seen with T below target, the
    smallest with T above; a NaN, the level not reached inside the measured taps, counts as above) and moves to x target / T, or,
    once both bracket ends exist and that step falls outside them (or T is NaN), to the bracket's midpoint (half of x while there is
    no lower end).  The decay time of an image-source room is not smooth in beta, the plain multiplicative step oscillates in some
    rooms; the bracket makes it settle."""

    def __init__(self, beta0, target, tol):
        self.target = torch.as_tensor(target, dtype=torch.float64).reshape(-1).clone()
        b = torch.as_tensor(beta0, dtype=torch.float64).reshape(-1).clamp(1e-12, 1.0 - 2.0 ** -40)
        self.x = -1.0 / torch.log(b)
        n = self.x.numel()
        self.tol = float(tol)
        self.lo, self.hi = torch.zeros(n, dtype=torch.float64), torch.full((n,), math.inf, dtype=torch.float64)
        self.converged = torch.zeros(n, dtype=torch.bool)
        self.best_x, self.best_t = self.x.clone(), torch.full((n,), math.nan, dtype=torch.float64)
        self.best_err = torch.full((n,), math.inf, dtype=torch.float64)
        self.rounds = 0

    @staticmethod
    def beta_of(x):
        return torch.exp(-1.0 / x)

    def beta(self):
        """The coefficients to measure next, f64 [n]: the kept one for a room that is done."""
        return self.beta_of(torch.where(self.converged, self.best_x, self.x))

    def update(self, measured):
        """measured f64 [n]: the figure of every room at beta() -> True when every room is done."""
        t = torch.as_tensor(measured, dtype=torch.float64).reshape(-1)
        self.rounds += 1
        for r in range(self.x.numel()):
            if bool(self.converged[r]):
                continue
            x, tr, goal = float(self.x[r]), float(t[r]), float(self.target[r])
            err = abs(tr - goal) / goal if math.isfinite(tr) else math.inf
            if err < float(self.best_err[r]) or self.rounds == 1:
                self.best_x[r], self.best_t[r], self.best_err[r] = x, tr, err
            if err <= self.tol:
                self.converged[r] = True
                continue
            if math.isfinite(tr) and tr < goal:
                self.lo[r] = max(float(self.lo[r]), x)
            else:
                self.hi[r] = min(float(self.hi[r]), x)
            lo, hi = float(self.lo[r]), float(self.hi[r])
            step = x * goal / tr if math.isfinite(tr) and tr > 0.0 else math.nan
            if lo > 0.0 and math.isfinite(hi):
                self.x[r] = step if lo < step < hi else 0.5 * (lo + hi)
            else:
                self.x[r] = step if math.isfinite(step) else 0.5 * x
        return bool(self.converged.all())


def _range(name, v, positive=False):
    lo, hi = (float(x) for x in v)
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi or (positive and lo <= 0.0):
        raise ValueError(f"{name} must be a finite {'positive ' if positive else ''}range (lo, hi) with lo <= hi, got {v!r}")
    return lo, hi


def _positive_int(name, v):
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"{name} must be a positive integer, got {v!r}")
    return v


def _int_in(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")
    return v


def bank_floor(bank, indices):
    """The first sample of the recording each clip belongs to, CPU int64 [B] in bank coordinates, from the tables
    bank.check_indices(indices) has built (call that first: it validates the indices)."""
    ends, _, _, sample0, _ = bank._tables
    idx = indices.to(torch.int64) if isinstance(indices, torch.Tensor) else torch.tensor(list(indices), dtype=torch.int64)
    return sample0[torch.bucketize(idx, ends, right=True)]


class Reverb:
    """`reverb = Reverb(rir_len, sr=16000, rt60=(lo, hi), drr_db=(lo, hi), predelay_ms=(lo, hi))`; `reverb.make_rirs(64, seed=e)` once
    per epoch; `wet = reverb(audio, seed=s)` or `wet = reverb.bank_clips(bank, indices, seed=s)` per batch.

    rir_len K: taps per response, 1 <= K <= 32768 (a response is cut there: choose K >= rt60 * sr to keep 60 dB of it).  The ranges
    are what sample() draws from; make_rirs also takes explicit per-room values."""

    def __init__(self, rir_len, sr=16000, rt60=(0.2, 0.8), drr_db=(0.0, 12.0), predelay_ms=(1.0, 5.0), device="cuda"):
        k = _positive_int("rir_len", rir_len)
        if k > 32768:
            raise ValueError(f"rir_len must be at most 32768 taps, got {k}")
        if isinstance(sr, bool) or not isinstance(sr, (int, float)) or not (math.isfinite(sr) and sr > 0):
            raise ValueError(f"sr must be a positive number, got {sr!r}")
        self.rir_len, self.sr = k, sr
        self.rt60 = _range("rt60", rt60, positive=True)
        self.drr_db = _range("drr_db", drr_db)
        self.predelay_ms = _range("predelay_ms", predelay_ms)
        if self.predelay_ms[0] < 0.0:
            raise ValueError(f"predelay_ms must not be negative, got {predelay_ms!r}")
        self.device = torch.device(device)
        self.rirs = None                      # the current table [n, K] on the device, what make_rirs / make_room_rirs made last
        self.sources_per_room = None          # S when make_room_rirs made the table (row room * S + j), None for make_rirs' rooms
        # what make_room_rirs(calibrate=) found (CPU): beta f64 [n, 6], the measured figure f64 [n], converged bool [n], rounds run
        self.room_beta = self.room_measured = self.room_converged = self.calibration_rounds = None

    # ---- host logic: draws and refusals, no device work ---------------------------------------------------
    def sample(self, n, generator):
        """-> (rt60 [n] f64 seconds, drr_db [n] f64, predelay [n] int32 samples), CPU tensors drawn from `generator` (a CPU
        torch.Generator).  Draw order: ONE torch.rand(3, n, float64); row 0 gives rt60 = lo + (hi - lo) u, row 1 drr_db likewise,
        row 2 predelay = max(1, round((lo + (hi - lo) u) * sr / 1000)) samples (the direct path keeps lag 0 to itself)."""
        _positive_int("n", n)
        u = torch.rand(3, n, generator=generator, dtype=torch.float64)
        (r0, r1), (d0, d1), (p0, p1) = self.rt60, self.drr_db, self.predelay_ms
        pre = ((p0 + (p1 - p0) * u[2]) * (self.sr / 1000.0)).round().clamp(min=1.0).to(torch.int32)
        return r0 + (r1 - r0) * u[0], d0 + (d1 - d0) * u[1], pre

    def check_params(self, n, rt60, drr_db, predelay):
        """Every refusal of make_rirs' per-room values -> params f64 [n, 3] = (ln(1000) / (rt60 sr), 10^(drr_db / 10), predelay), the
        table maavss_rir_synth reads."""
        rt = torch.as_tensor(rt60, dtype=torch.float64).reshape(-1)
        dr = torch.as_tensor(drr_db, dtype=torch.float64).reshape(-1)
        pd = torch.as_tensor(predelay)
        if pd.dtype.is_floating_point or pd.dtype == torch.bool:
            raise ValueError(f"predelay must hold integers (samples), got {pd.dtype}")
        pd = pd.reshape(-1).to(torch.int64)
        for name, t in (("rt60", rt), ("drr_db", dr), ("predelay", pd)):
            if t.is_cuda:
                raise ValueError(f"{name} must be a CPU tensor or a number (its values are checked on the host)")
            if t.numel() not in (1, n):
                raise ValueError(f"{name} must be a number or hold {n} values, got {t.numel()}")
        rt, dr, pd = rt.expand(n), dr.expand(n), pd.expand(n)
        if not bool((torch.isfinite(rt) & (rt > 0)).all()):
            raise ValueError("rt60 must be finite and positive")
        lin = torch.pow(10.0, dr / 10.0)
        if not bool((torch.isfinite(dr) & torch.isfinite(lin) & (lin > 0)).all()):
            raise ValueError("drr_db must be finite and 10^(drr_db / 10) a positive float64")
        if bool((pd < 1).any()):
            raise ValueError("predelay must be at least 1 sample: lag 0 is the direct path")
        return torch.stack([math.log(1000.0) / (rt * self.sr), lin, pd.to(torch.float64)], dim=1).contiguous()

    # ---- image-source rooms: host logic --------------------------------------------------------------------
    @staticmethod
    def kernel_table(half_width=8, resolution=32):
        """The fractional-delay kernel maavss_room_rir interpolates in: T f64 [2 H R + 1], g(x) = sinc(x) (1 + cos(pi x / H)) / 2 at
        x = i / R - H, with the entries at integer x set to exactly 0 and the one at x = 0 to exactly 1 (an image that falls on a
        sample stays a clean impulse)."""
        h, r = _int_in("half_width", half_width, 1, 32), _int_in("resolution", resolution, 1, 256)
        x = torch.arange(2 * h * r + 1, dtype=torch.float64) / r - h
        t = torch.sinc(x) * (0.5 * (1.0 + torch.cos(math.pi * x / h)))
        t[::r] = 0.0
        t[h * r] = 1.0
        return t

    @staticmethod
    def eyring_beta(dims, rt60):
        """dims [n, 3] metres, rt60 [n] seconds (CPU, f64) -> beta f64 [n, 6] = exp(-0.0805 V / (A_surf rt60)), the same on all six
        walls, clamped into [0, 1]: Eyring's formula (rt60 = 0.161 V / (-A_surf ln(1 - alpha)), beta^2 = 1 - alpha) solved for beta.
        This is a NOMINAL figure.  An image-source shoebox with uniform walls decays more slowly than Eyring predicts, because the
        axial paths graze fewer walls than a diffuse field does: a CPU prototype of the definition measured T20 of 0.46, 0.85 and
        0.37 s for nominal 0.30, 0.50 and 0.25 s in three rooms (profiles/room_rir_decay.json holds the float64 twin's ratios).
        make_room_rirs(rt60=, calibrate="t20") starts from this figure and searches the coefficient whose MEASURED decay time
        (Reverb.measure) is the one requested."""
        d = torch.as_tensor(dims, dtype=torch.float64).reshape(-1, 3)
        rt = torch.as_tensor(rt60, dtype=torch.float64).reshape(-1)
        if rt.numel() not in (1, d.shape[0]):
            raise ValueError(f"rt60 must be a number or hold {d.shape[0]} values, got {rt.numel()}")
        if not bool((torch.isfinite(d) & (d > 0)).all()) or not bool((torch.isfinite(rt) & (rt > 0)).all()):
            raise ValueError("dims and rt60 must be finite and positive")
        volume = d[:, 0] * d[:, 1] * d[:, 2]
        surface = 2.0 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 0] * d[:, 2])
        beta = torch.exp(-0.0805 * volume / (surface * rt)).clamp(0.0, 1.0)
        return beta[:, None].expand(-1, 6).contiguous()

    def sample_rooms(self, n, generator, sources=1, dims=((3.0, 8.0), (3.0, 8.0), (2.4, 3.5)), rt60=None, wall_margin=0.3, min_distance=0.5):
        """-> (dims [n, 3], mic [n, 3], sources [n, S, 3], rt60 [n]), CPU f64 tensors drawn from `generator` (a CPU torch.Generator).
        Draw order: ONE torch.rand(n, 7 + 3 S, float64) u; columns 0-2 give the dimensions lo + (hi - lo) u from the three `dims`
        ranges, column 3 rt60 likewise (from `rt60`, by default the instance's range), columns 4-6 the microphone
        wall_margin + (L - 2 wall_margin) u per axis, columns 7 + 3 j .. 9 + 3 j source j the same way.  Then, while any source lies
        closer than min_distance to its microphone: ONE torch.rand(bad, 3, float64) redraws those sources, in (room, source) order, by
        the same rule; after 64 rounds that still leave one too close the arguments are refused."""
        _positive_int("n", n)
        s = _positive_int("sources", sources)
        ranges = [_range(f"dims[{a}]", dims[a], positive=True) for a in range(3)] if len(dims) == 3 else None
        if ranges is None:
            raise ValueError(f"dims must be three (lo, hi) ranges, got {dims!r}")
        r0, r1 = self.rt60 if rt60 is None else _range("rt60", rt60, positive=True)
        margin, dist = float(wall_margin), float(min_distance)
        if not (math.isfinite(margin) and margin > 0.0 and math.isfinite(dist) and dist >= 0.0):
            raise ValueError(f"wall_margin must be positive and min_distance non-negative, got {wall_margin!r}, {min_distance!r}")
        if min(lo for lo, _ in ranges) <= 2.0 * margin:
            raise ValueError(f"the smallest room of {dims!r} leaves no space inside wall_margin = {margin}")
        u = torch.rand(n, 7 + 3 * s, generator=generator, dtype=torch.float64)
        lo = torch.tensor([v[0] for v in ranges], dtype=torch.float64)
        hi = torch.tensor([v[1] for v in ranges], dtype=torch.float64)
        size = lo + (hi - lo) * u[:, 0:3]
        span = size - 2.0 * margin
        mic = margin + span * u[:, 4:7]
        src = margin + span[:, None, :] * u[:, 7:].reshape(n, s, 3)
        for _ in range(64):
            bad = ((src - mic[:, None, :]) ** 2).sum(dim=2).sqrt() < dist
            if not bool(bad.any()):
                return size, mic, src, r0 + (r1 - r0) * u[:, 3]
            room = bad.nonzero()[:, 0]
            src[bad] = margin + span[room] * torch.rand(int(bad.sum()), 3, generator=generator, dtype=torch.float64)
        raise ValueError(f"min_distance = {dist} leaves sources too close to the microphone after 64 redraws: the rooms are too small for it")

    def check_rooms(self, dims, mic, sources, beta=None, rt60=None, c=343.0, half_width=8, resolution=32, taps=None):
        """Every refusal of make_room_rirs, from values alone (no device work) -> (geom f64 [n S, 15] = (L, m, s, beta) per row,
        bounds int32 [n S, 3], table f64 [2 H R + 1], S).  The lattice bounds: N_a = floor(Rmax / (2 L_a)) + 1 with
        Rmax = d0 + (K + H) c / sr, beyond which no image reaches a tap below K.  K is rir_len, or `taps` when given (the scratch
        table a calibration measures)."""
        k_taps = self.rir_len if taps is None else taps
        table = self.kernel_table(half_width, resolution)
        if isinstance(c, bool) or not isinstance(c, (int, float)) or not (math.isfinite(c) and c > 0):
            raise ValueError(f"c must be a positive number (m/s), got {c!r}")
        if (beta is None) == (rt60 is None):
            raise ValueError("exactly one of beta [n, 6] and rt60 [n] must be given")
        tensors = {}
        for name, v in (("dims", dims), ("mic", mic), ("sources", sources), ("beta", beta), ("rt60", rt60)):
            if v is None:
                continue
            if isinstance(v, torch.Tensor) and v.is_cuda:
                raise ValueError(f"{name} must be a CPU tensor or nested lists (its values are checked on the host)")
            tensors[name] = torch.as_tensor(v, dtype=torch.float64)
        d, m, src = tensors["dims"], tensors["mic"], tensors["sources"]
        if d.dim() != 2 or d.shape[1] != 3 or d.shape[0] < 1:
            raise ValueError(f"dims must be [n, 3], got {tuple(d.shape)}")
        n = d.shape[0]
        if tuple(m.shape) != (n, 3):
            raise ValueError(f"mic must be [{n}, 3], got {tuple(m.shape)}")
        if src.dim() != 3 or src.shape[0] != n or src.shape[1] < 1 or src.shape[2] != 3:
            raise ValueError(f"sources must be [{n}, S, 3] with S >= 1, got {tuple(src.shape)}")
        s = src.shape[1]
        if n * s > 1 << 19:
            raise ValueError(f"a table holds at most {1 << 19} responses, got {n} rooms x {s} sources")
        if not bool((torch.isfinite(d) & (d > 0)).all()):
            raise ValueError("dims must be finite and positive")
        if not bool(((m > 0) & (m < d)).all()):
            raise ValueError("every microphone must lie strictly inside its room (not on a wall)")
        if not bool(((src > 0) & (src < d[:, None, :])).all()):
            raise ValueError("every source must lie strictly inside its room (not on a wall)")
        if rt60 is not None:
            rt = tensors["rt60"].reshape(-1)
            if rt.numel() not in (1, n):
                raise ValueError(f"rt60 must be a number or hold {n} values, got {rt.numel()}")
            b = self.eyring_beta(d, rt)
        else:
            b = tensors["beta"]
            if tuple(b.shape) != (n, 6):
                raise ValueError(f"beta must be [{n}, 6] (walls x0 x1 y0 y1 z0 z1), got {tuple(b.shape)}")
            if not bool(((b >= 0) & (b <= 1)).all()):
                raise ValueError("beta must lie in [0, 1]")
        diff = src - m[:, None, :]
        d0 = ((diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]).sqrt()         # [n, S]
        if not bool((d0 > 0).all()):
            raise ValueError("a source lies on its microphone")
        rmax = d0 + (k_taps + half_width) * float(c) / float(self.sr)
        bounds = torch.floor(rmax[..., None] / (2.0 * d[:, None, :])) + 1.0                                            # [n, S, 3]
        images = 8.0 * (2.0 * bounds + 1.0).prod(dim=2)
        if not bool((images <= float(1 << 31)).all()):
            r = int((images > float(1 << 31)).nonzero()[0, 0])
            raise ValueError(f"room {r} ({d[r].tolist()} m) needs a lattice box of {images[r].max().item():.3g} images for {k_taps} taps, "
                             f"above the cap of 2^31")
        geom = torch.cat([d[:, None, :].expand(n, s, 3), m[:, None, :].expand(n, s, 3), src, b[:, None, :].expand(n, s, 6)], dim=2)
        return geom.reshape(n * s, 15).contiguous(), bounds.to(torch.int32).reshape(n * s, 3).contiguous(), table, s

    def sample_room_index(self, batch, generator, group):
        """-> CPU int32 [batch]: consecutive groups of `group` clips share one room of the current make_room_rirs table, drawn
        uniformly, and get distinct sources of it.  Draw order: ONE torch.randint(0, rooms, (batch / group,)), then ONE
        torch.rand(batch / group, S, float64) whose rows' argsort gives each group's sources in clip order (its first `group`
        entries).  With a Mixer whose partners stay inside the group, a target and its interferers are heard in one room."""
        _positive_int("batch", batch)
        _positive_int("group", group)
        if self.rirs is None:
            raise ValueError("no room responses yet: call make_room_rirs first")
        if self.sources_per_room is None:
            raise ValueError("the current table is make_rirs': its rows are unrelated rooms (make_room_rirs makes rooms with several sources)")
        s = self.sources_per_room
        if group > s:
            raise ValueError(f"group = {group} clips need as many distinct sources, the rooms have {s}")
        if batch % group:
            raise ValueError(f"batch = {batch} is no multiple of group = {group}")
        groups = batch // group
        room = torch.randint(0, self.rirs.shape[0] // s, (groups,), generator=generator)
        src = torch.rand(groups, s, generator=generator, dtype=torch.float64).argsort(dim=1)[:, :group]
        return (room[:, None] * s + src).reshape(batch).to(torch.int32)

    def sample_index(self, batch, generator):
        """-> CPU int32 [batch]: one room of the current table per clip, uniformly, one torch.randint(0, n, (batch,))."""
        _positive_int("batch", batch)
        if self.rirs is None:
            raise ValueError("no room responses yet: call make_rirs first")
        return torch.randint(0, self.rirs.shape[0], (batch,), generator=generator, dtype=torch.int32)

    def check_index(self, batch, rir_index, seed):
        """rir_index as given, or drawn from `seed` -> CPU int32 [batch], every entry inside the current table."""
        if self.rirs is None:
            raise ValueError("no room responses yet: call make_rirs first")
        if rir_index is None:
            return self.sample_index(batch, torch.Generator().manual_seed(seed))
        if not isinstance(rir_index, torch.Tensor) or rir_index.dtype != torch.int32 or tuple(rir_index.shape) != (batch,):
            raise ValueError(f"rir_index must be an int32 [{batch}] tensor, got {getattr(rir_index, 'dtype', type(rir_index))} "
                             f"{tuple(getattr(rir_index, 'shape', ()))}")
        if rir_index.is_cuda:
            raise ValueError("rir_index must be a CPU tensor (its values are checked on the host, like crop boxes)")
        n = self.rirs.shape[0]
        if bool(((rir_index < 0) | (rir_index >= n)).any()):
            raise ValueError(f"rir_index entries must be in [0, {n}), got [{int(rir_index.min())}, {int(rir_index.max())}]")
        return rir_index.contiguous()

    def check(self, audio, rir_index=None, seed=0, lead=0):
        """Every refusal of __call__, from shapes, dtypes and values alone (no device work) -> rir_index (CPU int32 [B]).  `audio` is
        the [B, L] tensor or, when it does not exist yet, the pair (B, L)."""
        if isinstance(lead, bool) or not isinstance(lead, int) or lead < 0:
            raise ValueError(f"lead must be a non-negative integer, got {lead!r}")
        if isinstance(audio, torch.Tensor):
            if audio.dim() != 2 or audio.dtype != torch.float32 or (audio.shape[1] > 1 and audio.stride(1) != 1) or audio.stride(0) < 0:
                raise ValueError(f"audio must be float32 [B, L] with unit last stride, got {audio.dtype} {tuple(audio.shape)} strides {audio.stride()}")
            b, length = audio.shape
            if lead > audio.storage_offset():
                raise ValueError(f"lead={lead}: only {audio.storage_offset()} samples of the tensor's storage lie in front of its first row")
        else:
            b, length = audio
            if lead:
                raise ValueError("lead needs the tensor whose storage holds the history")
        if b < 1 or length < 1:
            raise ValueError(f"audio needs at least one clip and one sample, got [B, L] = {(b, length)}")
        return self.check_index(b, rir_index, seed)

    # ---- device work ----------------------------------------------------------------------------------------
    def make_rirs(self, n, seed=0, rt60=None, drr_db=None, predelay=None, noise=None):
        """A table of n room responses [n, K] on the device, kept as `reverb.rirs` and returned.  rt60 (s), drr_db, predelay (samples,
        >= 1): numbers or n values on the CPU; those not given are self.sample(n, torch.Generator().manual_seed(seed))'s.  noise [n, K]
        f32 on the device: the normals g; by default the kernel draws them from `seed` (row r the same whatever n is).  The
        parameters reach the device in one non-blocking copy from pinned memory; one launch on the current stream."""
        _positive_int("n", n)
        if n > 1 << 19:
            raise ValueError(f"a table holds at most {1 << 19} responses, got {n}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        if rt60 is None or drr_db is None or predelay is None:
            drawn = self.sample(n, torch.Generator().manual_seed(seed))
            rt60 = drawn[0] if rt60 is None else rt60
            drr_db = drawn[1] if drr_db is None else drr_db
            predelay = drawn[2] if predelay is None else predelay
        params = self.check_params(n, rt60, drr_db, predelay)
        k = self.rir_len
        if noise is not None and (not isinstance(noise, torch.Tensor) or noise.dtype != torch.float32 or tuple(noise.shape) != (n, k)
                                  or (k > 1 and noise.stride(1) != 1) or noise.stride(0) < (k if n > 1 else 0)):
            raise ValueError(f"noise must be a float32 [{n}, {k}] tensor with unit last stride and rows that do not overlap, got "
                             f"{getattr(noise, 'dtype', type(noise))} {tuple(getattr(noise, 'shape', ()))}")
        rirs = torch.empty(n, k, device=self.device, dtype=torch.float32)
        _lib.require_cuda(rirs, noise)
        staged = torch.empty(n, 3, device=self.device, dtype=torch.float64)
        staged.copy_(params.pin_memory(), non_blocking=True)
        call("maavss_rir_synth", ptr(staged), ptr(noise), (noise.stride(0) if n > 1 else k) if noise is not None else 0, seed, 0, n, k,
             ptr(rirs), k, stream_ptr())
        self.rirs, self.sources_per_room = rirs, None
        return rirs

    def check_measure(self, rirs=None, direct_ms=2.5):
        """Every refusal of measure, from shapes, dtypes and values alone (no device work) -> (rirs, k_direct, k_early)."""
        if isinstance(direct_ms, bool) or not isinstance(direct_ms, (int, float)) or not (math.isfinite(direct_ms) and direct_ms >= 0):
            raise ValueError(f"direct_ms must be a finite non-negative number, got {direct_ms!r}")
        if rirs is None:
            if self.rirs is None:
                raise ValueError("no room responses yet: call make_rirs or make_room_rirs first, or pass rirs")
            rirs = self.rirs
        if not isinstance(rirs, torch.Tensor) or rirs.dtype != torch.float32:
            raise ValueError(f"rirs must be a float32 tensor, got {getattr(rirs, 'dtype', type(rirs))}")
        if rirs.dim() != 2 or rirs.shape[0] < 1 or rirs.shape[1] < 1:
            raise ValueError(f"rirs must be [n, K] with n, K >= 1, got {tuple(rirs.shape)}")
        n, k = rirs.shape
        if k > 32768 or n > 1 << 19:
            raise ValueError(f"a table holds at most {1 << 19} responses of at most 32768 taps, got {(n, k)}")
        if (k > 1 and rirs.stride(1) != 1) or (n > 1 and rirs.stride(0) < k):
            raise ValueError(f"rirs must have unit last stride and a row stride of at least K = {k}, got strides {rirs.stride()}")
        a, b = rirs.device, self.device                     # "cuda" names the current device: it goes with any index
        if a.type != b.type or (a.index is not None and b.index is not None and a.index != b.index):
            raise ValueError(f"rirs is on {rirs.device}, this Reverb on {self.device}")
        k_direct = math.floor(direct_ms * self.sr / 1000.0) + 1
        k_early = round(0.050 * self.sr)
        if k_direct >= 1 << 30 or k_early >= 1 << 30:
            raise ValueError(f"direct_ms = {direct_ms!r} at sr = {self.sr!r} is no tap index")
        return rirs, k_direct, k_early

    def measure(self, rirs=None, *, direct_ms=2.5):
        """The room-acoustic figures of a response table (by default the current one, `reverb.rirs`; any float32 [n, K] with unit last
        stride on this device otherwise) -> a dict of device f64 tensors [n] (columns of one [n, 6] buffer):
            energy   E[0], the sum of the squared taps                   edt      6 x the time the Schroeder curve takes to -10 dB
            t20      3 x its time from -5 to -25 dB                      t30      2 x its time from -5 to -35 dB        (seconds)
            c50_db   10 log10 of the energy in front of tap round(0.050 sr) over the energy from it on
            drr_db   the same at tap floor(direct_ms sr / 1000) + 1: direct_ms = 0 sets tap 0 alone against everything behind it
        A decay time is NaN when the row never falls to its lower level, every figure but energy is NaN for a silent row, and a
        non-finite tap spoils its own row only (maavss_rir_measure, include/maavss.h; tests/rir_measure_twin.py restates the
        definition in float64: energies and crossings bit for bit, times and dB within a few ulp of log10).  Everything is checked
        before any device work; one launch on the current stream, no workspace, no synchronisation."""
        rirs, k_direct, k_early = self.check_measure(rirs, direct_ms)
        _lib.require_cuda(rirs)
        n, k = rirs.shape
        out = torch.empty(n, len(FIGURES), device=rirs.device, dtype=torch.float64)
        levels = (ctypes.c_double * len(LEVELS_DB))(*thresholds())
        call("maavss_rir_measure", ptr(rirs), n, k, rirs.stride(0) if n > 1 else k, float(self.sr), k_direct, k_early,
             ctypes.addressof(levels), len(LEVELS_DB), ptr(out), stream_ptr())
        return {name: out[:, i] for i, name in enumerate(FIGURES)}

    def check_calibration(self, dims, rt60, beta, calibrate, tol, max_iter, measure_len):
        """Every refusal of make_room_rirs' calibration arguments (no device work) -> the scratch table's taps.  By default the
        smallest multiple of 1024 that holds (lower level + 20 dB) / 60 of the longest requested decay, so that the cut does not
        bend the Schroeder curve at the level the figure is read at; independent of rir_len."""
        if calibrate not in CALIBRATE:
            raise ValueError(f"calibrate must be None or one of {sorted(CALIBRATE)}, got {calibrate!r}")
        if beta is not None or rt60 is None:
            raise ValueError("calibrate searches the wall coefficient for a requested rt60: give rt60 and no beta")
        if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not (math.isfinite(tol) and 0.0 < tol < 1.0):
            raise ValueError(f"tol must be a relative tolerance in (0, 1), got {tol!r}")
        _positive_int("max_iter", max_iter)
        if measure_len is None:
            if isinstance(rt60, torch.Tensor) and rt60.is_cuda:
                raise ValueError("rt60 must be a CPU tensor or a number (its values are checked on the host)")
            rt = torch.as_tensor(rt60, dtype=torch.float64).reshape(-1)
            if rt.numel() < 1 or not bool((torch.isfinite(rt) & (rt > 0)).all()):
                raise ValueError("dims and rt60 must be finite and positive")
            frac = (CALIBRATE[calibrate] + 20.0) / 60.0
            measure_len = max(1, math.ceil(frac * float(rt.max()) * self.sr / 1024.0)) * 1024
        else:
            _positive_int("measure_len", measure_len)
        if measure_len > 32768:
            raise ValueError(f"the calibration would measure {measure_len} taps, a table holds at most 32768: pass a shorter measure_len")
        return measure_len

    def make_room_rirs(self, dims, mic, sources, *, beta=None, rt60=None, c=343.0, half_width=8, resolution=32, calibrate=None, tol=0.02,
                       max_iter=12, measure_len=None):
        """A table of image-source responses [n S, K] on the device, kept as `reverb.rirs` and returned; row room * S + j is source j
        of a room and `reverb.sources_per_room` = S.  dims [n, 3], mic [n, 3], sources [n, S, 3]: CPU tensors or nested lists, metres,
        positions strictly inside the room.  Exactly one of beta [n, 6] (pressure reflection coefficients of the walls x0 x1 y0 y1 z0
        z1, in [0, 1]) and rt60 [n] (seconds: eyring_beta's nominal figure on all six walls).  c: speed of sound; half_width H and
        resolution R: the fractional-delay kernel (kernel_table).  Every response is normalised to its direct path, which sits at
        lag 0.  Everything is checked before any device work; kernel table, geometry and lattice bounds reach the device in one
        non-blocking copy from pinned memory; one launch on the current stream, no synchronisation.

        calibrate = "t20" | "t30" | "edt" (with rt60, never with beta) makes rt60 mean that measured figure: per room, the uniform
        wall coefficient is searched (Calibration: from eyring_beta, in x = -1 / ln(beta)) until the figure, averaged over the
        room's S sources, is within `tol` (relative) of the request, at most `max_iter` rounds.  A round fills a scratch table of
        `measure_len` taps for all rooms, measures it and copies ONE column [n S] f64 to the host: calibration synchronises once a
        round; it is table set-up, not a training step.  The table itself is then filled by the path above from the coefficients
        found: `reverb.rirs` has the bytes of make_room_rirs(beta=reverb.room_beta).  reverb.room_beta [n, 6], room_measured [n]
        (the figure at that coefficient, over measure_len taps), room_converged [n] and calibration_rounds say what was found; a
        room that is not within tol after max_iter rounds (or whose scratch rows never reach the level: NaN) keeps its best
        coefficient and is flagged False there, it does not raise."""
        if calibrate is not None:
            return self._calibrated_rooms(dims, mic, sources, beta, rt60, c, half_width, resolution, calibrate, tol, max_iter, measure_len)
        geom, bounds, table, s = self.check_rooms(dims, mic, sources, beta, rt60, c, half_width, resolution)
        rirs = torch.empty(geom.shape[0], self.rir_len, device=self.device, dtype=torch.float32)
        self._fill_rooms(geom, bounds, table, half_width, resolution, c, rirs)
        self.rirs, self.sources_per_room = rirs, s
        return rirs

    def _calibrated_rooms(self, dims, mic, sources, beta, rt60, c, half_width, resolution, calibrate, tol, max_iter, measure_len):
        """make_room_rirs(calibrate=): every refusal (the final table's and the scratch table's) before any device work, then the
        rounds, then the final table through make_room_rirs(beta=)."""
        taps = self.check_calibration(dims, rt60, beta, calibrate, tol, max_iter, measure_len)
        self.check_rooms(dims, mic, sources, None, rt60, c, half_width, resolution)                         # the final table's lattice boxes
        geom, bounds, table, s = self.check_rooms(dims, mic, sources, None, rt60, c, half_width, resolution, taps=taps)
        n = geom.shape[0] // s
        target = torch.as_tensor(rt60, dtype=torch.float64).reshape(-1).expand(n)
        search = Calibration(geom.reshape(n, s, 15)[:, 0, 9], target, tol)
        scratch = torch.empty(n * s, taps, device=self.device, dtype=torch.float32)
        geom = geom.clone()
        for _ in range(max_iter):
            geom.reshape(n, s, 15)[:, :, 9:] = search.beta()[:, None, None]
            self._fill_rooms(geom, bounds, table, half_width, resolution, c, scratch)
            figure = self.measure(scratch)[calibrate].cpu()                                                  # the round's one host copy
            if search.update(figure.reshape(n, s).mean(dim=1)):
                break
        self.room_beta = Calibration.beta_of(search.best_x)[:, None].expand(n, 6).contiguous()
        self.room_measured, self.room_converged, self.calibration_rounds = search.best_t.clone(), search.converged.clone(), search.rounds
        return self.make_room_rirs(dims, mic, sources, beta=self.room_beta, c=c, half_width=half_width, resolution=resolution)

    def _fill_rooms(self, geom, bounds, table, half_width, resolution, c, rirs):
        """The launch behind make_room_rirs: check_rooms' CPU tables into rirs [rows, K] (unit last stride; K = rir_len, or the
        taps of a calibration's scratch table).  Table, geometry and bounds travel as one f64 block (the int32 bounds last, two to a
        slot); the entry point checks the pinned copy."""
        _lib.require_cuda(rirs)
        rows, n_tab, k_taps = geom.shape[0], table.numel(), rirs.shape[1]
        packed = torch.zeros((3 * rows + 1) // 2 * 2, dtype=torch.int32)
        packed[:3 * rows] = bounds.reshape(-1)
        host = torch.cat([table, geom.reshape(-1), packed.view(torch.float64)]).pin_memory()
        staged = torch.empty(host.numel(), device=self.device, dtype=torch.float64)
        staged.copy_(host, non_blocking=True)
        call("maavss_room_rir", ptr(staged[n_tab:]), ptr(staged[n_tab + 15 * rows:]), ptr(host[n_tab:]), ptr(host[n_tab + 15 * rows:]), rows,
             ptr(staged), half_width, resolution, float(self.sr), float(c), k_taps, ptr(rirs), rirs.stride(0) if rows > 1 else k_taps,
             stream_ptr())

    def _convolve(self, src_ptr, n_src, start, floor, index, length, out):
        """The launch behind __call__ and bank_clips: CPU tables start / floor int64 [B] and index int32 [B] in the coordinates of the
        flat buffer at src_ptr.  The tables go to the device in one copy from pinned memory (the int64 ones first: 8-byte aligned);
        the entry point checks the pinned copy."""
        b = start.numel()
        host = torch.cat([start.contiguous().view(torch.int32), floor.contiguous().view(torch.int32), index]).pin_memory()
        staged = torch.empty(5 * b, device=self.device, dtype=torch.int32)
        staged.copy_(host, non_blocking=True)
        call("maavss_reverb", src_ptr, n_src, ptr(staged), ptr(staged[2 * b:]), ptr(host), ptr(host[2 * b:]), b, length, ptr(self.rirs),
             self.rirs.shape[0], self.rirs.stride(0), self.rir_len, ptr(staged[4 * b:]), ptr(host[4 * b:]), ptr(out),
             out.stride(0) if b > 1 else length, stream_ptr())
        return out

    def __call__(self, audio, rir_index=None, *, seed=0, lead=0):
        """audio [B, L] f32 on the device (rows may be strided and may overlap) -> wet [B, L]: row b convolved with room rir_index[b]
        (CPU int32 [B]; by default self.sample_index(B, torch.Generator().manual_seed(seed))).  lead=P: the P samples in front of
        every row (in the tensor's storage, e.g. the row's past in a longer recording) are its history; by default a row starts from
        zero state.  Everything is checked before any device work; no synchronisation; all work goes to the current stream."""
        index = self.check(audio, rir_index, seed, lead)
        _lib.require_cuda(audio, self.rirs)
        b, length = audio.shape
        stride = audio.stride(0) if b > 1 else 0
        floor = torch.arange(b, dtype=torch.int64) * stride
        out = torch.empty(b, length, device=audio.device, dtype=torch.float32)
        return self._convolve(audio.data_ptr() - 4 * lead, lead + (b - 1) * stride + length, floor + lead, floor, index, length, out)

    def check_bank(self, bank, n, rir_index, seed, out=None):
        """bank_clips' refusals behind bank.check_indices -> rir_index (CPU int32 [n])."""
        index = self.check_index(n, rir_index, seed)
        a, b = bank.device, self.device                     # "cuda" names the current device: it goes with any index
        if a.type != b.type or (a.index is not None and b.index is not None and a.index != b.index):
            raise ValueError(f"the bank is on {bank.device}, the room responses on {self.device}")
        length = bank.clip_samples
        if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (n, length) or out.dtype != torch.float32
                                or (length > 1 and out.stride(1) != 1) or (n > 1 and out.stride(0) < length)):
            raise ValueError(f"out must be a float32 {[n, length]} tensor with unit last stride and rows that do not overlap, got "
                             f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
        return index

    def bank_clips(self, bank, indices, rir_index=None, *, seed=0, out=None):
        """The clips `indices` of a ClipBank (as bank.batch takes them), wet: convolved from bank.audio where it lies, each clip hearing
        its own recording's past back to the recording's first sample and never a neighbouring recording -> [B, clip_samples] f32
        (`out`, when given).  With a one-tap table [[1]] these are bank.batch's audio clips bit for bit."""
        _, start = bank.check_indices(indices)
        index = self.check_bank(bank, start.numel(), rir_index, seed, out)
        return self.cut(bank, start, bank_floor(bank, indices), index, out=out)

    def cut(self, bank, start, floor, index, *, out=None):
        """bank_clips behind its checks: CPU tables in bank coordinates."""
        _lib.require_cuda(bank.audio, self.rirs, out)
        if out is None:
            out = torch.empty(start.numel(), bank.clip_samples, device=self.device, dtype=torch.float32)
        return self._convolve(bank.audio.data_ptr(), bank.n_samples, start, floor, index, bank.clip_samples, out)
