"""Which clips of a ClipBank an epoch trains on, and in what order.

The reference shuffles its clips with DataLoader(shuffle=True) (av_dataset.py:580), splits train and validation by file (--split) and
lists "audio thresholding" and "video reject" in its to_do.txt as undone.  `ClipSampler` is all three for a bank resident in HBM:

  selection  ClipBank.activity() (csrc/clip_select.hip) is one pass over the bank that leaves a table of per-clip statistics on the
             device; maavss_bank_clip_select compares it with the thresholds there and writes one byte of reasons per clip.  ONE copy of
             those bytes to the host -- the only synchronisation, once -- gives `accepted` (ascending CPU int64) and `rejected` (a count
             per reason; a clip rejected for two reasons counts in both).
  epochs     `epoch(e)` yields CPU index tensors for ClipBank.batch / ClipPipeline.submit_clips: a permutation of `accepted` drawn
             from a torch.Generator seeded by (seed, e) alone, of which rank `rank` of `world` takes every world-th element.  Every rank
             draws the same permutation and has the same number of steps, as shard_batch's callers need.

Reasons, as bits of the byte and names in `rejected` (include/maavss.h states the comparisons):
  0 too_quiet                rms_db < min_rms_db             (digital silence is -inf dB)
  1 too_quiet_for_recording  rel_db < min_rel_db             (against the mean power of the clip's recording)
  2 few_active_segments      n_active < min_active_fraction * J, J = hops_per_frame * clip_frames segments a clip
  3 static                   motion_mean < min_motion        (mean absolute difference of consecutive maps; frozen video is exactly 0)
  4 scene_cut                motion_peak > max_motion_peak
  5 clipped                  peak >= max_peak                (in f32)
  6 nonfinite                n_bad > 0                       (reject_nonfinite)
A threshold left None is not tested.  The table is bank.activity(range_db=range_db): `range_db` (default 40) is the dynamic range of
the active-segment rule; the bank keeps the table of the range asked for last and computes another range anew (a table given as a dict
was made with a range of its own: `range_db` is not used then).  With every threshold None and reject_nonfinite=False every clip of the
chosen recordings is accepted and no statistic is computed.

Instead of a bank the constructor takes a precomputed activity table: a dict of CPU tensors as ClipBank.activity() names them (only
the columns the thresholds use, and `recording`), plus the int `segments` (J) when min_active_fraction is given.  The same rule then
runs in torch on the host, which is how the host logic is tested without a GPU; nothing is ever computed on the CPU for a bank.
"""
import torch

from ._lib import call, ptr, stream_ptr

REASONS = ("too_quiet", "too_quiet_for_recording", "few_active_segments", "static", "scene_cut", "clipped", "nonfinite")
_COLUMN = ("rms_db", "rel_db", "n_active", "motion_mean", "motion_peak", "peak", "n_bad")          # the statistic reason k reads
_DTYPE = {"rms_db": torch.float64, "rel_db": torch.float64, "motion_mean": torch.float64, "motion_peak": torch.float64,
          "energy": torch.float64, "peak": torch.float32, "n_bad": torch.int32, "n_active": torch.int32, "recording": torch.int32}


def _count(name, v, lo):
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return v


def _threshold(name, v):
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
        raise ValueError(f"{name} must be a number or None, got {v!r}")
    return float(v)


class ClipSampler:
    """`sampler = ClipSampler(bank, batch_size, min_rms_db=-50, min_motion=1e-3, ...)`; `for indices in sampler.epoch(e): ...`;
    `len(sampler)` steps per epoch; `sampler.accepted`, `sampler.rejected`, `sampler.reasons` (CPU uint8, one byte per clip of the
    bank).  See the module docstring."""

    def __init__(self, bank_or_activity, batch_size, *, min_rms_db=None, min_rel_db=None, min_active_fraction=None, min_motion=None,
                 max_motion_peak=None, max_peak=None, reject_nonfinite=True, recordings=None, seed=0, rank=0, world=1, shuffle=True,
                 drop_last=True, range_db=40.0):
        self.batch_size = _count("batch_size", batch_size, 1)
        self.world, self.rank = _count("world", world, 1), _count("rank", rank, 0)
        if self.rank >= self.world:
            raise ValueError(f"rank {rank} is outside [0, world = {world})")
        self.seed = _count("seed", seed, 0)
        if self.seed >= 1 << 31:
            raise ValueError(f"seed must be below 2^31, got {seed}")
        self.shuffle, self.drop_last = bool(shuffle), bool(drop_last)
        thresholds = [_threshold(n, v) for n, v in (("min_rms_db", min_rms_db), ("min_rel_db", min_rel_db),
                                                    ("min_active_fraction", min_active_fraction), ("min_motion", min_motion),
                                                    ("max_motion_peak", max_motion_peak), ("max_peak", max_peak))]
        if thresholds[2] is not None and not 0.0 <= thresholds[2] <= 1.0:
            raise ValueError(f"min_active_fraction must be in [0, 1], got {min_active_fraction!r}")
        enabled = sum(1 << k for k, v in enumerate(thresholds) if v is not None) | (64 if reject_nonfinite else 0)
        self.thresholds = dict(zip(("min_rms_db", "min_rel_db", "min_active_fraction", "min_motion", "max_motion_peak", "max_peak"), thresholds),
                               reject_nonfinite=bool(reject_nonfinite))
        table = isinstance(bank_or_activity, dict)
        if table:
            act = bank_or_activity
            if "recording" not in act:
                raise ValueError("an activity table needs the column 'recording'")
            recording = self._column(act, "recording", None)
            n_clips = recording.numel()
            segments = act.get("segments")
            if enabled & 4:
                _count("the activity table's 'segments' (J, which min_active_fraction needs)", segments, 1)
        else:
            bank = bank_or_activity
            if not hasattr(bank, "activity") or not hasattr(bank, "clip_recordings"):
                raise ValueError(f"expected a ClipBank or a dict of activity columns, got {type(bank).__name__}")
            n_clips, segments = len(bank), bank.hops_per_frame * bank.clip_frames
            if n_clips == 0:
                raise ValueError("the bank holds no clip")
            recording = bank.clip_recordings()
        if n_clips == 0:
            raise ValueError("the activity table is empty")
        n_rec = int(recording.max()) + 1
        if recordings is None:
            chosen = torch.ones(n_clips, dtype=torch.bool)
        else:
            recs = list(recordings)
            if not recs or any(isinstance(q, bool) or not isinstance(q, int) or not 0 <= q < n_rec for q in recs):
                raise ValueError(f"recordings must be a non-empty sequence of recording numbers in [0, {n_rec}), got {recordings!r}")
            chosen = torch.isin(recording, torch.tensor(sorted(set(recs)), dtype=torch.int32))
        self.recordings = None if recordings is None else sorted(set(recs))
        min_active = thresholds[2] * segments if enabled & 4 else 0.0
        if enabled == 0:
            reasons = torch.zeros(n_clips, dtype=torch.uint8)
        elif table:
            reasons = self._select_host(act, n_clips, enabled, thresholds, min_active)
        else:
            a = bank.activity(range_db=range_db)
            dev = torch.empty(n_clips, device=bank.device, dtype=torch.uint8)
            t = [0.0 if v is None else v for v in thresholds]
            call("maavss_bank_clip_select", ptr(a["rms_db"]), ptr(a["rel_db"]), ptr(a["n_active"]), ptr(a["motion_mean"]),
                 ptr(a["motion_peak"]), ptr(a["peak"]), ptr(a["n_bad"]), n_clips, enabled, t[0], t[1], min_active, t[3], t[4], t[5],
                 ptr(dev), stream_ptr())
            reasons = dev.cpu()                      # the one copy, and the one synchronisation
        self.reasons = reasons
        self.accepted = torch.nonzero(chosen & (reasons == 0)).reshape(-1)
        considered = reasons[chosen]
        self.rejected = {name: int(((considered >> k) & 1).sum()) for k, name in enumerate(REASONS)}
        self.n_considered = int(chosen.sum())
        if self.accepted.numel() == 0:
            raise ValueError(f"no clip is accepted: {self.n_considered} clips considered, rejected per reason {self.rejected}")
        a = self.accepted.numel()
        if self.drop_last:
            self._steps = a // (self.world * self.batch_size)
            if self._steps == 0:
                raise ValueError(f"{a} accepted clips do not fill one batch of {self.batch_size} on each of {self.world} ranks "
                                 f"(rejected per reason {self.rejected}); use drop_last=False or a smaller batch")
        else:
            self._steps = -(-(-(-a // self.world)) // self.batch_size)
        self._epoch = self._step = 0
        self._resume = None

    @staticmethod
    def _column(act, name, n):
        t = act.get(name)
        if not isinstance(t, torch.Tensor) or t.is_cuda or t.dim() != 1 or t.dtype != _DTYPE[name] or (n is not None and t.numel() != n):
            raise ValueError(f"activity column {name!r} must be a 1-D CPU {_DTYPE[name]} tensor" + ("" if n is None else f" of {n} clips") +
                             f", got {getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}"
                             + (" on the device (pass the bank itself, or .cpu() the table)" if getattr(t, "is_cuda", False) else ""))
        return t

    @classmethod
    def _select_host(cls, act, n, enabled, th, min_active):
        """The rule of maavss_bank_clip_select on a CPU table, comparison for comparison."""
        col = {name: cls._column(act, name, n) for k, name in enumerate(_COLUMN) if enabled >> k & 1}
        m = torch.zeros(n, dtype=torch.uint8)
        tests = (lambda: col["rms_db"] < th[0], lambda: col["rel_db"] < th[1], lambda: col["n_active"].to(torch.float64) < min_active,
                 lambda: col["motion_mean"] < th[3], lambda: col["motion_peak"] > th[4],
                 lambda: col["peak"] >= torch.tensor(th[5], dtype=torch.float32), lambda: col["n_bad"] > 0)
        for k, test in enumerate(tests):
            if enabled >> k & 1:
                m |= test().to(torch.uint8) << k
        return m

    def __len__(self):
        return self._steps

    def order(self, e):
        """Epoch e's order of `accepted`, the same on every rank."""
        e = _count("epoch", e, 0)
        if e >= 1 << 32:
            raise ValueError(f"epoch must be below 2^32, got {e}")
        if not self.shuffle:
            return self.accepted
        # torch's CPU generator (mt19937) keeps the low 32 bits of its seed: (seed, e) goes through the splitmix64 finaliser first, so
        # that neighbouring seeds and epochs give unrelated draws; nothing else enters
        z = (((self.seed << 32) | e) + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        g = torch.Generator()
        g.manual_seed((z ^ (z >> 31)) & 0xFFFFFFFF)
        return self.accepted[torch.randperm(self.accepted.numel(), generator=g)]

    def share(self, e):
        """This rank's clips of epoch e, in order: every world-th element of the order.  drop_last: of its first
        len(self) * batch_size * world elements.  Otherwise the order is first extended by its own start to a multiple of world (at most
        world - 1 clips twice, as DistributedSampler pads), and the last batch may be short."""
        order = self.order(e)
        if self.drop_last:
            order = order[:self._steps * self.batch_size * self.world]
        else:
            pad = -order.numel() % self.world
            if pad:
                order = torch.cat([order] + [order] * (pad // order.numel()) + [order[:pad % order.numel()]])
        return order[self.rank::self.world]

    def epoch(self, e):
        """Yield the batches of epoch e: CPU int64 tensors of batch_size clip numbers (the last one shorter with drop_last=False).  After
        load_state_dict of a state taken in this epoch, start with the batch that run would have seen next."""
        mine = self.share(e)
        start = 0
        if self._resume is not None and self._resume[0] == e:
            start = self._resume[1]
        self._resume = None
        for i in range(start, self._steps):
            last = i + 1 == self._steps
            self._epoch, self._step = (e + 1, 0) if last else (e, i + 1)          # what a state_dict taken inside the loop body holds
            yield mine[i * self.batch_size:(i + 1) * self.batch_size]
        if start >= self._steps:
            self._epoch, self._step = e + 1, 0

    def state_dict(self):
        """{'epoch', 'step'}: the next batch to draw."""
        return {"epoch": self._epoch, "step": self._step}

    def load_state_dict(self, state):
        e, i = _count("state epoch", state.get("epoch") if isinstance(state, dict) else None, 0), _count("state step", state.get("step"), 0)
        if i >= max(self._steps, 1):
            raise ValueError(f"state step {i} is outside this sampler's {self._steps} steps per epoch (other thresholds, batch size or world?)")
        self._epoch, self._step, self._resume = e, i, (e, i)
